// MM (FSDCodec, kanzi transform id 15) on gfx950, forward and inverse: every block of a batch in the same launches.
//
// Reference being replaced: transform/FSDCodec.cpp:103-291 (forward), :293-386 (inverse), Global.cpp:136-150 (log2_1024),
// :313-329 (computeFirstOrderEntropy1024) and Global::detectSimpleType (datatype.hpp).
//
// Forward: seven sampled histograms and the six large-delta counts in one pass (per-wave LDS histograms, merged with global atomics),
// one workgroup per block for the entropies, the distance and the mode; XOR mode is element-wise, delta mode writes 1 or 2 bytes per
// source byte at offsets from tile sums scanned per block. The tiles stage their output in LDS, write it out in words and count, on
// the way, the output bytes that the reference's final check samples.
//
// Inverse: dst[j] = f_j(dst[j - dist]) runs along `dist` residue classes. XOR mode is a prefix XOR per class (tile totals, a scan per
// block, apply). Delta mode: a 255 is an escape head unless it is the payload of the escape in front of it, so inside a maximal run of
// 255s heads and payloads alternate; with the position behind the last non-255 byte (a max scan, across tiles by look-back) every byte
// knows its kind. Token ends are counted and scanned, and every token becomes a step (add a, then XOR x) in token order. A step is a
// bijection of the 256 byte values and steps do not compose into a small closed form, so a wave carries a stretch's effect as the map
// of all 256 incoming values -- four per lane in one register, SWAR add and XOR, the step broadcast by readlane -- for every class; one
// thread per (block, class) then chains the stretch maps from LDS into the value each stretch starts from, and the stretches are
// walked again from those values. An all-escape block takes exactly this path. Every guard runs before any byte is written.
#include "common.hpp"
#include "stages.hpp"
#include "datatype.hpp"
#include "magic.hpp"

namespace knz {

namespace {

constexpr int MM_T = 256;                        // threads per workgroup
constexpr u32 MM_SEG = 16;                       // source bytes per thread
constexpr u32 MM_TILE = MM_T * MM_SEG;           // source bytes per workgroup
constexpr u32 MM_MIN = 1024;                     // FSDCodec::MIN_LENGTH
constexpr u32 MM_STRETCH = 48 * 128;             // tokens per wave of the inverse delta walk (48: every distance divides it)
constexpr u32 MM_XSEG = 48;                      // output bytes per thread of the inverse XOR mode
constexpr u32 MM_XTILE = MM_T * MM_XSEG;
constexpr u32 MM_CHAIN = 256;                    // stretch maps per LDS load of the chain kernel

enum { MM_NONE = 0, MM_DELTA = 1, MM_XOR = 2, MM_DETECT = 3 };

__device__ static const u16 MM_LOG2_4096[257] = {
#include "mm_log2.inc"
};

struct MmInfo {
    u32 mode;        // MM_*
    u32 dist;
    u32 ent0;        // forward: entropy of the plain samples
    u32 ok;
    u32 total;       // forward: output bytes
    u32 large[6];    // forward: large deltas per candidate distance
    u32 tokens;      // inverse delta: tokens
    u32 dangling;    // inverse delta: the last byte is an escape head
    u32 beg;         // inverse: first payload byte
};

// per-block scratch (u32 words)
constexpr u32 MM_INFO = 0;                       // [64]
constexpr u32 MM_HIST = 64;                      // [8][256]: the seven sampled histograms, the histogram of the final check
constexpr u32 MM_TL = MM_HIST + 8 * 256;         // [tiles] inverse: 1 + index of the tile's last non-255 byte (0: none)

struct MmLayout { u32 tc, p0, xt, inval, maps, steps; size_t stride; };
__host__ __device__ inline MmLayout mm_layout(u32 maxLen)
{
    const u32 nT = maxLen / MM_TILE + 2, nS = maxLen / MM_STRETCH + 2, nX = maxLen / MM_XTILE + 2;
    MmLayout L;
    L.tc = MM_TL + nT;                           // [tiles] token (inverse) / output byte (forward) counts, then offsets
    L.p0 = L.tc + nT;                            // [tiles] inverse delta: the position behind the last non-255 byte in front of the tile
    L.xt = (L.p0 + nT + 3) & ~3u;                // [xtiles][4] inverse XOR: class totals of a tile, then what the tile starts from
    L.inval = L.xt + 4 * nX;                     // [stretches][4] inverse delta: the 16 class values a stretch starts from
    L.maps = L.inval + 4 * nS;                   // [stretches][16][64] the stretch maps
    L.steps = L.maps + 16 * 64 * nS;             // [maxLen] u16 steps
    L.stride = ((size_t)L.steps + maxLen / 2 + 1 + 63) & ~(size_t)63;
    return L;
}

__device__ __forceinline__ u32 mm_max_encoded(u32 n) { return n + (n < 1024 ? 64u : n >> 4); }      // FSDCodec.hpp, = knz_max_encoded_len(KNZ_T_MM, n)

__device__ __forceinline__ MmInfo* mm_info(u32* ws) { return reinterpret_cast<MmInfo*>(ws + MM_INFO); }

__device__ __forceinline__ int mm_log2_1024(u32 x)                 // Global::log2_1024, x > 0
{
    if (x < 256) return (MM_LOG2_4096[x] + 2) >> 2;
    const int lg = ilog2_u32(x);
    if ((x & (x - 1)) == 0) return lg << 10;
    return (lg - 7) * 1024 + ((MM_LOG2_4096[x >> (lg - 7)] + 2) >> 2);
}

// inclusive sum over MM_T threads
__device__ u32 mm_wg_sum(u32 v, u32* sh /* [4] */, u32* total)
{
    const int lane = lane_id(), wave = (int)(threadIdx.x >> 6);
    for (int o = 1; o < 64; o <<= 1) { const u32 t = (u32)__shfl_up((int)v, (unsigned)o, 64); if (lane >= o) v += t; }
    if (lane == 63) sh[wave] = v;
    __syncthreads();
    u32 carry = 0, tot = 0;
    for (int w = 0; w < MM_T / 64; w++) { if (w < wave) carry += sh[w]; tot += sh[w]; }
    __syncthreads();
    *total = tot;
    return carry + v;
}

// exclusive max over MM_T threads
__device__ u32 mm_wg_max_excl(u32 v, u32* sh /* [4] */)
{
    const int lane = lane_id(), wave = (int)(threadIdx.x >> 6);
    for (int o = 1; o < 64; o <<= 1) { const u32 t = (u32)__shfl_up((int)v, (unsigned)o, 64); if (lane >= o) v = max(v, t); }
    if (lane == 63) sh[wave] = v;
    __syncthreads();
    u32 carry = 0;
    for (int w = 0; w < wave; w++) carry = max(carry, sh[w]);
    __syncthreads();
    const u32 prev = (u32)__shfl_up((int)v, 1u, 64);
    return max(carry, lane ? prev : 0u);
}

// Entropy (Global::computeFirstOrderEntropy1024) of nHist histograms of 256 bins in global memory, by one workgroup; thread q < nHist
// returns histogram q's value
__device__ u32 mm_entropy(const u32* hist, int nHist, u32 blockLen, u64* sTerm /* [nHist][256] */)
{
    const int t = (int)threadIdx.x;
    const int logLen = blockLen ? mm_log2_1024(blockLen) : 0;
    for (int q = 0; q < nHist; q++) {
        const u32 h = hist[q * 256 + t];
        sTerm[q * 256 + t] = h ? (((u64)h * (u64)(int64_t)(logLen - mm_log2_1024(h))) >> 3) : 0ull;
    }
    __syncthreads();
    u32 r = 0;
    if (t < nHist && blockLen) {
        u64 sum = 0;
        for (int i = 0; i < 256; i++) sum += sTerm[t * 256 + i];
        r = (u32)(sum / (u64)blockLen);
    }
    __syncthreads();
    return r;
}

// cnt bytes from LDS to dst + base by nThr threads (tid among them): bytes up to a word boundary, words, the bytes left over. With
// hist != nullptr the bytes whose output position falls into [r0, r0 + rl) or [r1, r1 + rl) are counted (LDS atomics).
__device__ __forceinline__ void mm_flush(u8* dst, u32 base, const u8* sOut, u32 cnt, u32 tid, u32 nThr, u32* hist, u32 r0, u32 r1, u32 rl)
{
    u8* p = dst + base;
    const u32 head = min(cnt, (u32)((4 - (reinterpret_cast<uintptr_t>(p) & 3)) & 3));
    const u32 nW = (cnt - head) / 4;
    if (tid < head) stg<u8>(p + tid, sOut[tid]);
    for (u32 i = tid; i < nW; i += nThr) {
        const u32 k = head + 4 * i;
        stg<u32>(p + k, (u32)sOut[k] | ((u32)sOut[k + 1] << 8) | ((u32)sOut[k + 2] << 16) | ((u32)sOut[k + 3] << 24));
    }
    const u32 k0 = head + 4 * nW;
    if (tid < cnt - k0) stg<u8>(p + k0 + tid, sOut[k0 + tid]);
    if (hist != nullptr && base < r1 + rl && base + cnt > r0) {
        for (u32 k = tid; k < cnt; k += nThr) {
            const u32 o = base + k;
            if (o - r0 < rl || o - r1 < rl) atomicAdd(&hist[sOut[k]], 1u);
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// forward
// ---------------------------------------------------------------------------------------------------------------------

// the guards in front of the detection (FSDCodec.cpp:105-146), zeroed histograms
__global__ __launch_bounds__(MM_T) void k_mm_f_init(XfStage st, u32* scratch, size_t stride)
{
    const int b = blockIdx.x;
    u32* ws = scratch + (size_t)b * stride;
    for (u32 i = threadIdx.x; i < 8 * 256; i += MM_T) ws[MM_HIST + i] = 0;
    if (threadIdx.x != 0) return;
    MmInfo* info = mm_info(ws);
    const u32 n = st.len[b];
    u32 mode = MM_DETECT;
    if (n < MM_MIN || (u64)st.cap[b] < (u64)mm_max_encoded(n)) mode = MM_NONE;
    if (mode != MM_NONE && st.dtype) {
        const int dt = st.dtype[b];
        if (dt != DT_UNDEFINED && dt != DT_MULTIMEDIA && dt != DT_BIN) mode = MM_NONE;
    }
    if (mode != MM_NONE) {
        const u32 m = knz_magic::magic_of(st.src[b]);
        if (m != 0 && m != 0x424Du && m != 0x52494646u && m != 0x5034u && m != 0x5035u && m != 0x5036u) mode = MM_NONE;
    }
    info->mode = mode; info->ok = 0; info->dist = 0; info->total = 0;
    for (int q = 0; q < 6; q++) info->large[q] = 0;
    st.ok[b] = (n == 0) ? 1 : 0;            // FSDCodec::forward returns true for an empty block
    st.newLen[b] = 0;
}

// the seven histograms over i in [count10, count5) of the three stretches, and per candidate distance the large deltas over
// [2 count5, 3 count5) (FSDCodec.cpp:148-185, :209-219): workgroup x takes i in [x MM_TILE, (x + 1) MM_TILE)
__global__ __launch_bounds__(MM_T) void k_mm_f_sample(XfStage st, u32* scratch, size_t stride)
{
    const int b = blockIdx.y;
    u32* ws = scratch + (size_t)b * stride;
    MmInfo* info = mm_info(ws);
    if (info->mode != MM_DETECT) return;
    const u32 n = st.len[b];
    const u32 count10 = n / 10, count5 = 2 * count10;
    const u32 j0 = blockIdx.x * MM_TILE;
    if (j0 >= count5) return;
    __shared__ u32 h[MM_T / 64][7][256];
    __shared__ u32 sLarge[6];
    for (u32 i = threadIdx.x; i < (MM_T / 64) * 7 * 256; i += MM_T) (&h[0][0][0])[i] = 0;
    if (threadIdx.x < 6) sLarge[threadIdx.x] = 0;
    __syncthreads();
    const u8* __restrict__ src = st.src[b];
    const int w = (int)(threadIdx.x >> 6);
    const u32 D[6] = { 1, 2, 3, 4, 8, 16 };
    u32 large[6] = { 0, 0, 0, 0, 0, 0 };
    for (u32 k = 0; k < MM_SEG; k++) {
        const u32 j = j0 + threadIdx.x + k * MM_T;
        if (j >= count5) break;
        const u8* p = src + 2 * count5 + j;
        const int s = p[0];
#pragma unroll
        for (int q = 0; q < 6; q++) { const int d = s - (int)p[-(int)D[q]]; large[q] += (d < -127 || d > 127) ? 1u : 0u; }
        if (j < count10) continue;
#pragma unroll
        for (u32 z = 0; z < 3; z++) {
            const u8* in = src + 2 * z * count5 + j;
            const u32 v = in[0];
            atomicAdd(&h[w][0][v], 1u);
#pragma unroll
            for (int q = 0; q < 6; q++) atomicAdd(&h[w][q + 1][v ^ in[-(int)D[q]]], 1u);
        }
    }
#pragma unroll
    for (int q = 0; q < 6; q++) if (large[q]) atomicAdd(&sLarge[q], large[q]);
    __syncthreads();
    for (u32 i = threadIdx.x; i < 7 * 256; i += MM_T) {
        u32 sum = 0;
        for (int v = 0; v < MM_T / 64; v++) sum += (&h[v][0][0])[i];
        if (sum) atomicAdd(&ws[MM_HIST + i], sum);
    }
    if (threadIdx.x < 6 && sLarge[threadIdx.x]) atomicAdd(&info->large[threadIdx.x], sLarge[threadIdx.x]);
}

// entropies, the quick exit with detectSimpleType, the distance and the mode (FSDCodec.cpp:187-226)
__global__ __launch_bounds__(MM_T) void k_mm_f_decide(XfStage st, u32* scratch, size_t stride)
{
    const int b = blockIdx.x;
    u32* ws = scratch + (size_t)b * stride;
    MmInfo* info = mm_info(ws);
    if (info->mode != MM_DETECT) return;
    const u32 n = st.len[b];
    const u32 count10 = n / 10, count5 = 2 * count10;
    __shared__ u64 sTerm[7 * 256];
    __shared__ u32 ent[7];
    const u32 e = mm_entropy(ws + MM_HIST, 7, 3 * count10, sTerm);
    if (threadIdx.x < 7) ent[threadIdx.x] = e;
    __syncthreads();
    if (threadIdx.x != 0) return;
    int minIdx = 0;
    for (int i = 0; i < 7; i++) if ((int)ent[i] < (int)ent[minIdx]) minIdx = i;
    if (ent[minIdx] >= ent[0]) {
        if (st.dtype) st.dtype[b] = (u8)pk_simple_type(3 * count10, ws + MM_HIST);
        info->mode = MM_NONE;
        return;
    }
    if (st.dtype) st.dtype[b] = (u8)DT_MULTIMEDIA;
    const u32 D[7] = { 0, 1, 2, 3, 4, 8, 16 };
    const u32 dist = D[minIdx];
    const u32 mode = info->large[minIdx - 1] > (count5 >> 5) ? MM_XOR : MM_DELTA;
    u8* dst = st.dst[b];
    dst[0] = mode == MM_XOR ? 1 : 0;
    dst[1] = (u8)dist;
    info->mode = mode; info->dist = dist; info->ent0 = ent[0];
    info->total = n + 2;                    // (delta mode: set by the scan)
}

// the output of source byte i (dist <= i): one byte, or the escape pair
__device__ __forceinline__ u32 mm_delta_code(int cur, int prev, u8* out)
{
    const int d = cur - prev;
    if (d >= -127 && d <= 127) { out[0] = (u8)(d < 0 ? -2 * d - 1 : 2 * d); return 1; }
    out[0] = 255; out[1] = (u8)(cur ^ prev);
    return 2;
}

// delta mode: output bytes of every tile
__global__ __launch_bounds__(MM_T) void k_mm_f_count(XfStage st, u32* scratch, size_t stride, MmLayout L)
{
    const int b = blockIdx.y;
    u32* ws = scratch + (size_t)b * stride;
    const MmInfo* info = mm_info(ws);
    if (info->mode != MM_DELTA) return;
    const u32 n = st.len[b], dist = info->dist;
    const u32 a0 = blockIdx.x * MM_TILE;
    if (a0 >= n) return;
    __shared__ u32 sh[4];
    const u8* __restrict__ src = st.src[b];
    u32 c = 0;
    for (u32 k = 0; k < MM_SEG; k++) {
        const u32 i = a0 + threadIdx.x + k * MM_T;
        if (i >= n) break;
        c++;
        if (i >= dist) { const int d = (int)src[i] - (int)src[i - dist]; c += (d < -127 || d > 127) ? 1u : 0u; }
    }
    u32 tot;
    mm_wg_sum(c, sh, &tot);
    if (threadIdx.x == 0) ws[L.tc + blockIdx.x] = tot;
}

// delta mode: tile offsets, and whether the reference's loop (it stops at dstIdx >= dstEnd - 1) reaches the end of the source: it
// does when the LAST token starts below dstEnd - 1 (FSDCodec.cpp:235, :270)
__global__ __launch_bounds__(MM_T) void k_mm_f_scan(XfStage st, u32* scratch, size_t stride, MmLayout L)
{
    const int b = blockIdx.x;
    u32* ws = scratch + (size_t)b * stride;
    MmInfo* info = mm_info(ws);
    if (info->mode != MM_DELTA) return;
    const u32 n = st.len[b], dist = info->dist;
    const u32 nT = (n + MM_TILE - 1) / MM_TILE;
    __shared__ u32 sh[4];
    u32 carry = 0;
    for (u32 base = 0; base < nT; base += MM_T) {
        const u32 j = base + threadIdx.x;
        const u32 v = (j < nT) ? ws[L.tc + j] : 0u;
        u32 tot;
        const u32 inc = mm_wg_sum(v, sh, &tot);
        if (j < nT) ws[L.tc + j] = carry + inc - v;
        carry += tot;
    }
    if (threadIdx.x == 0) {
        const u8* src = st.src[b];
        const int d = (int)src[n - 1] - (int)src[n - 1 - dist];
        const u32 lastLen = (d < -127 || d > 127) ? 2u : 1u;
        const u32 total = 2 + carry;
        const u32 dstEnd = mm_max_encoded(n);
        info->total = total;
        if (!(total - lastLen < dstEnd - 1)) info->mode = MM_NONE;          // (the data type stays MULTIMEDIA)
    }
}

// both modes: the tile's output, and the samples of the final check
__global__ __launch_bounds__(MM_T) void k_mm_f_emit(XfStage st, u32* scratch, size_t stride, MmLayout L)
{
    const int b = blockIdx.y;
    u32* ws = scratch + (size_t)b * stride;
    const MmInfo* info = mm_info(ws);
    const u32 mode = info->mode;
    if (mode != MM_DELTA && mode != MM_XOR) return;
    const u32 n = st.len[b], dist = info->dist;
    const u32 a0 = blockIdx.x * MM_TILE;
    if (a0 >= n) return;
    __shared__ u8 sOut[2 * MM_TILE];
    __shared__ u32 hist[256];
    __shared__ u32 sh[4];
    hist[threadIdx.x] = 0;
    const u8* __restrict__ src = st.src[b];
    const u32 a = min(a0 + threadIdx.x * MM_SEG, n), e = min(a + MM_SEG, n);
    u8 out[2 * MM_SEG];
    u32 c = 0;
    for (u32 i = a; i < e; i++) {
        if (i < dist) out[c++] = src[i];
        else if (mode == MM_XOR) out[c++] = src[i] ^ src[i - dist];
        else c += mm_delta_code(src[i], src[i - dist], out + c);
    }
    u32 tot;
    const u32 off = mm_wg_sum(c, sh, &tot) - c;
    for (u32 k = 0; k < c; k++) sOut[off + k] = out[k];
    __syncthreads();
    const u32 count10 = n / 10, count5 = 2 * count10;
    const u32 base = 2 + (mode == MM_XOR ? a0 : ws[L.tc + blockIdx.x]);
    mm_flush(st.dst[b], base, sOut, tot, threadIdx.x, MM_T, hist, count5, 3 * count5, count10);
    __syncthreads();
    if (hist[threadIdx.x]) atomicAdd(&ws[MM_HIST + 7 * 256 + threadIdx.x], hist[threadIdx.x]);
}

// the final check (FSDCodec.cpp:273-286), ok and the length
__global__ __launch_bounds__(MM_T) void k_mm_f_finish(XfStage st, u32* scratch, size_t stride)
{
    const int b = blockIdx.x;
    u32* ws = scratch + (size_t)b * stride;
    MmInfo* info = mm_info(ws);
    if (info->mode != MM_DELTA && info->mode != MM_XOR) return;
    const u32 n = st.len[b];
    const u32 count5 = 2 * (n / 10);
    __shared__ u64 sTerm[256];
    const u32 e = mm_entropy(ws + MM_HIST + 7 * 256, 1, count5, sTerm);
    if (threadIdx.x != 0) return;
    const u32 ok = (int)e < (int)info->ent0 ? 1u : 0u;
    info->ok = ok;
    st.ok[b] = (u8)ok;
    st.newLen[b] = ok ? info->total : 0u;
}

// ---------------------------------------------------------------------------------------------------------------------
// inverse
// ---------------------------------------------------------------------------------------------------------------------

// the guards (FSDCodec.cpp:295-327, :378-381); XOR mode is decided here
__global__ __launch_bounds__(64) void k_mm_i_head(XfStage st, u32* scratch, size_t stride)
{
    const int b = blockIdx.x;
    if (threadIdx.x != 0) return;
    u32* ws = scratch + (size_t)b * stride;
    MmInfo* info = mm_info(ws);
    const u32 count = st.len[b];
    info->mode = MM_NONE; info->ok = 0; info->tokens = 0; info->dangling = 0;
    st.ok[b] = count == 0 ? 1 : 0;
    st.newLen[b] = 0;
    if (count < 4) return;
    const u8* src = st.src[b];
    const u32 dstEnd = st.cap[b];
    const u32 mode = src[0], dist = src[1];
    if (dist < 1 || (dist > 4 && dist != 8 && dist != 16)) return;
    if (count < dist + 2 || dist > dstEnd) return;
    if (mode > 1) return;
    info->dist = dist; info->beg = dist + 2;
    if (mode == 1) {
        if (count - dist - 2 > dstEnd - dist) return;       // the loops stop at the destination's end: srcIdx != srcEnd
        info->mode = MM_XOR; info->ok = 1; info->tokens = count - dist - 2;
        st.ok[b] = 1; st.newLen[b] = count - 2;
        return;
    }
    info->mode = MM_DELTA;
}

// delta mode: 1 + index of the last non-255 byte of every tile of the payload
__global__ __launch_bounds__(MM_T) void k_mm_i_last(XfStage st, u32* scratch, size_t stride)
{
    const int b = blockIdx.y;
    u32* ws = scratch + (size_t)b * stride;
    const MmInfo* info = mm_info(ws);
    if (info->mode != MM_DELTA) return;
    const u32 count = st.len[b];
    const u32 a0 = info->beg + blockIdx.x * MM_TILE;
    if (a0 >= count) return;
    __shared__ u32 sMax;
    if (threadIdx.x == 0) sMax = 0;
    __syncthreads();
    const u8* __restrict__ src = st.src[b];
    u32 m = 0;
    for (u32 k = 0; k < MM_SEG; k++) {
        const u32 i = a0 + threadIdx.x + k * MM_T;
        if (i < count && src[i] != 255) m = i + 1;
    }
    if (m) atomicMax(&sMax, m);
    __syncthreads();
    if (threadIdx.x == 0) ws[MM_TL + blockIdx.x] = sMax;
}

// The kinds of the thread's bytes [a, e) of tile t: returns the position behind the last non-255 byte in front of a (the start of the
// run of 255s that reaches a, or a itself). Byte i with run = i - P: a 255 at an even run offset is an escape head; any byte at an
// odd offset is a payload; the others are plain tokens.
// p0 holds the tile's look-back result: k_mm_i_count finds and stores it (find = true), k_mm_i_steps reads it.
__device__ u32 mm_run_start(const u8* __restrict__ src, const u32* tl, u32* p0, bool find, u32 t, u32 beg, u32 a, u32 e, u32* sL, u32* sh)
{
    if (threadIdx.x == 0) *sL = 0;
    __syncthreads();
    u32 P0 = find ? 0u : p0[t];
    for (u32 hi = find ? t : 0u; hi > 0 && P0 == 0; hi = hi > (u32)MM_T ? hi - MM_T : 0) {
        if (threadIdx.x < hi) { const u32 v = tl[hi - 1 - threadIdx.x]; if (v) atomicMax(sL, v); }
        __syncthreads();
        P0 = *sL;
        __syncthreads();
    }
    if (P0 == 0) P0 = beg;
    if (find && threadIdx.x == 0) p0[t] = P0;
    u32 m = 0;
    for (u32 i = a; i < e; i++) if (src[i] != 255) m = i + 1;
    return max(P0, mm_wg_max_excl(m, sh));
}

// delta mode: token ends of every tile; the tile that holds the last byte notes a dangling escape head
__global__ __launch_bounds__(MM_T) void k_mm_i_count(XfStage st, u32* scratch, size_t stride, MmLayout L)
{
    const int b = blockIdx.y;
    u32* ws = scratch + (size_t)b * stride;
    MmInfo* info = mm_info(ws);
    if (info->mode != MM_DELTA) return;
    const u32 count = st.len[b], beg = info->beg;
    const u32 a0 = beg + blockIdx.x * MM_TILE;
    if (a0 >= count) return;
    __shared__ u32 sL;
    __shared__ u32 sh[4];
    const u8* __restrict__ src = st.src[b];
    const u32 a = min(a0 + threadIdx.x * MM_SEG, count), e = min(a + MM_SEG, count);
    u32 P = mm_run_start(src, ws + MM_TL, ws + L.p0, true, blockIdx.x, beg, a, e, &sL, sh);
    u32 c = 0;
    for (u32 i = a; i < e; i++) {
        const bool is255 = src[i] == 255, odd = ((i - P) & 1) != 0;
        const bool head = is255 && !odd;
        c += head ? 0u : 1u;
        if (!is255) P = i + 1;
        if (i == count - 1 && head) info->dangling = 1;
    }
    u32 tot;
    mm_wg_sum(c, sh, &tot);
    if (threadIdx.x == 0) ws[L.tc + blockIdx.x] = tot;
}

// delta mode: tile offsets in token order, the verdict (FSDCodec.cpp:336, :348, :385) and the length
__global__ __launch_bounds__(MM_T) void k_mm_i_scan(XfStage st, u32* scratch, size_t stride, MmLayout L)
{
    const int b = blockIdx.x;
    u32* ws = scratch + (size_t)b * stride;
    MmInfo* info = mm_info(ws);
    if (info->mode != MM_DELTA) return;
    const u32 count = st.len[b];
    const u32 nT = (count - info->beg + MM_TILE - 1) / MM_TILE;
    __shared__ u32 sh[4];
    u32 carry = 0;
    for (u32 base = 0; base < nT; base += MM_T) {
        const u32 j = base + threadIdx.x;
        const u32 v = (j < nT) ? ws[L.tc + j] : 0u;
        u32 tot;
        const u32 inc = mm_wg_sum(v, sh, &tot);
        if (j < nT) ws[L.tc + j] = carry + inc - v;
        carry += tot;
    }
    if (threadIdx.x == 0) {
        const u32 dist = info->dist;
        const bool ok = !info->dangling && carry <= st.cap[b] - dist;
        info->tokens = carry;
        info->ok = ok ? 1u : 0u;
        if (!ok) info->mode = MM_NONE;
        st.ok[b] = ok ? 1 : 0;
        st.newLen[b] = ok ? dist + carry : 0u;
    }
}

// delta mode: one step per token, in token order: low byte = what is added, high byte = what is XORed afterwards
__global__ __launch_bounds__(MM_T) void k_mm_i_steps(XfStage st, u32* scratch, size_t stride, MmLayout L)
{
    const int b = blockIdx.y;
    u32* ws = scratch + (size_t)b * stride;
    const MmInfo* info = mm_info(ws);
    if (info->mode != MM_DELTA) return;
    const u32 count = st.len[b], beg = info->beg;
    const u32 a0 = beg + blockIdx.x * MM_TILE;
    if (a0 >= count) return;
    __shared__ u32 sL;
    __shared__ u32 sh[4];
    const u8* __restrict__ src = st.src[b];
    const u32 a = min(a0 + threadIdx.x * MM_SEG, count), e = min(a + MM_SEG, count);
    u32 P = mm_run_start(src, ws + MM_TL, ws + L.p0, false, blockIdx.x, beg, a, e, &sL, sh);
    u16 out[MM_SEG];
    u32 c = 0;
    for (u32 i = a; i < e; i++) {
        const u32 v = src[i];
        const bool is255 = v == 255, odd = ((i - P) & 1) != 0;
        if (odd) out[c++] = (u16)(v << 8);
        else if (!is255) out[c++] = (u16)(((v >> 1) ^ (0u - (v & 1))) & 255u);
        if (!is255) P = i + 1;
    }
    u32 tot;
    const u32 off = ws[L.tc + blockIdx.x] + mm_wg_sum(c, sh, &tot) - c;
    u16* steps = reinterpret_cast<u16*>(ws + L.steps);
    for (u32 k = 0; k < c; k++) steps[off + k] = out[k];
}

// delta mode: a wave per stretch of MM_STRETCH tokens: per class the map of the 256 incoming values (lane l holds values 4l .. 4l + 3)
__global__ __launch_bounds__(MM_T) void k_mm_i_maps(XfStage st, u32* scratch, size_t stride, MmLayout L)
{
    const int b = blockIdx.y;
    u32* ws = scratch + (size_t)b * stride;
    const MmInfo* info = mm_info(ws);
    if (info->mode != MM_DELTA) return;
    const u32 T = info->tokens, dist = info->dist;
    const u32 sId = blockIdx.x * (MM_T / 64) + (threadIdx.x >> 6);
    const u32 k0 = sId * MM_STRETCH;
    if (k0 + MM_STRETCH >= T) return;                       // (nobody starts from the last stretch's map)
    const u32 lane = (u32)lane_id();
    const u16* __restrict__ steps = reinterpret_cast<const u16*>(ws + L.steps);
    for (u32 c = 0; c < dist; c++) {
        const u32 M = MM_STRETCH / dist;
        u32 x = (4 * lane) * 0x01u + (4 * lane + 1) * 0x0100u + (4 * lane + 2) * 0x010000u + (4 * lane + 3) * 0x01000000u;
        for (u32 m0 = 0; m0 < M; m0 += 64) {
            const u32 m = m0 + lane;
            const u32 sv = (m < M) ? steps[k0 + c + m * dist] : 0u;
            const u32 C = (sv & 255u) * 0x01010101u;
            const u32 A = C & 0x7F7F7F7Fu, B = (C & 0x80808080u) ^ ((sv >> 8) * 0x01010101u);
#pragma unroll
            for (int k = 0; k < 64; k++) {
                const u32 ak = rl(A, k), bk = rl(B, k);
                x = (((x & 0x7F7F7F7Fu) + ak) ^ (x & 0x80808080u)) ^ bk;
            }
        }
        ws[L.maps + ((size_t)sId * 16 + c) * 64 + lane] = x;
    }
}

// delta mode: per (block, class) the value every stretch starts from, through the stretch maps staged in LDS
__global__ __launch_bounds__(MM_T) void k_mm_i_chain(XfStage st, u32* scratch, size_t stride, MmLayout L)
{
    const int b = blockIdx.y;
    u32* ws = scratch + (size_t)b * stride;
    const MmInfo* info = mm_info(ws);
    if (info->mode != MM_DELTA) return;
    const u32 c = blockIdx.x, T = info->tokens;
    if (c >= info->dist) return;
    const u32 nS = (T + MM_STRETCH - 1) / MM_STRETCH;
    __shared__ u32 sm[MM_CHAIN * 64];
    u8* inval = reinterpret_cast<u8*>(ws + L.inval);
    u32 v = st.src[b][2 + c];
    for (u32 s0 = 0; s0 < nS; s0 += MM_CHAIN) {
        const u32 cnt = min((u32)MM_CHAIN, nS - s0);
        // (the last stretch has no map: its slot is not read)
        for (u32 i = threadIdx.x; i < cnt * 64; i += MM_T)
            if (s0 + i / 64 + 1 < nS) sm[i] = ws[L.maps + ((size_t)(s0 + i / 64) * 16 + c) * 64 + (i & 63)];
        __syncthreads();
        if (threadIdx.x == 0) {
            const u8* mb = reinterpret_cast<const u8*>(sm);
            for (u32 s = 0; s < cnt; s++) {
                inval[(size_t)(s0 + s) * 16 + c] = (u8)v;
                if (s0 + s + 1 < nS) v = mb[s * 256 + v];
            }
        }
        __syncthreads();
    }
}

// delta mode: a wave per stretch walks its tokens from the known values, class by class, into LDS and writes the stretch out
__global__ __launch_bounds__(MM_T) void k_mm_i_apply(XfStage st, u32* scratch, size_t stride, MmLayout L)
{
    const int b = blockIdx.y;
    u32* ws = scratch + (size_t)b * stride;
    const MmInfo* info = mm_info(ws);
    if (info->mode != MM_DELTA) return;
    const u32 T = info->tokens, dist = info->dist;
    const u32 wave = threadIdx.x >> 6, lane = (u32)lane_id();
    const u32 sId = blockIdx.x * (MM_T / 64) + wave;
    u8* dst = st.dst[b];
    if (sId == 0 && lane < dist) dst[lane] = st.src[b][2 + lane];
    const u32 k0 = sId * MM_STRETCH;
    if (k0 >= T) return;
    const u32 cntS = min(MM_STRETCH, T - k0);
    __shared__ u8 sOut[MM_T / 64][MM_STRETCH];
    const u16* __restrict__ steps = reinterpret_cast<const u16*>(ws + L.steps);
    const u8* inval = reinterpret_cast<const u8*>(ws + L.inval);
    for (u32 c = 0; c < dist && c < cntS; c++) {
        const u32 M = (cntS - c + dist - 1) / dist;
        u32 v = uni((u32)inval[(size_t)sId * 16 + c]);
        for (u32 m0 = 0; m0 < M; m0 += 64) {
            const u32 m = m0 + lane;
            const u32 sv = (m < M) ? steps[k0 + c + m * dist] : 0u;
            const u32 A = sv & 255u, B = sv >> 8;
            u32 mine = 0;
#pragma unroll
            for (int k = 0; k < 64; k++) {
                const u32 ak = rl(A, k), bk = rl(B, k);
                v = ((v + ak) & 255u) ^ bk;
                mine = (lane == (u32)k) ? v : mine;
            }
            if (m < M) sOut[wave][c + m * dist] = (u8)mine;
        }
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    mm_flush(dst, dist + k0, sOut[wave], cntS, lane, 64, nullptr, 0, 0, 0);
}

// XOR mode: the thread's 48 payload bytes (output positions j0 ..), zero behind the end
__device__ __forceinline__ void mm_x_load(const u8* __restrict__ src, u32 j0, u32 n, u8* v /* [48] */)
{
    const u8* p = src + 2 + j0;
    if (j0 + MM_XSEG + 4 <= n && j0 > 0) {
        const uintptr_t a = reinterpret_cast<uintptr_t>(p);
        const u8* w = reinterpret_cast<const u8*>(a & ~(uintptr_t)3);
        const u32 sh = (u32)(a & 3) * 8;
        u32 prev = ldg<u32>(w);
#pragma unroll
        for (int q = 0; q < 12; q++) {
            const u32 next = ldg<u32>(w + 4 * q + 4);
            const u32 x = sh ? ((prev >> sh) | (next << (32 - sh))) : prev;
            v[4 * q] = (u8)x; v[4 * q + 1] = (u8)(x >> 8); v[4 * q + 2] = (u8)(x >> 16); v[4 * q + 3] = (u8)(x >> 24);
            prev = next;
        }
    } else {
#pragma unroll
        for (u32 k = 0; k < MM_XSEG; k++) v[k] = (j0 + k < n) ? p[k] : (u8)0;
    }
}

// class totals of 48 bytes as 16 bytes in four words (classes at or above D stay zero)
template <int D> __device__ __forceinline__ uint4 mm_x_fold(const u8* v)
{
    u8 r[16];
#pragma unroll
    for (int c = 0; c < 16; c++) r[c] = 0;
#pragma unroll
    for (int k = 0; k < 48; k++) r[k % D] ^= v[k];
    uint4 o;
    o.x = r[0] | (r[1] << 8) | (r[2] << 16) | ((u32)r[3] << 24);
    o.y = r[4] | (r[5] << 8) | (r[6] << 16) | ((u32)r[7] << 24);
    o.z = r[8] | (r[9] << 8) | (r[10] << 16) | ((u32)r[11] << 24);
    o.w = r[12] | (r[13] << 8) | (r[14] << 16) | ((u32)r[15] << 24);
    return o;
}
__device__ __forceinline__ uint4 mm_x_fold(const u8* v, u32 dist)
{
    switch (dist) {
    case 1: return mm_x_fold<1>(v);
    case 2: return mm_x_fold<2>(v);
    case 3: return mm_x_fold<3>(v);
    case 4: return mm_x_fold<4>(v);
    case 8: return mm_x_fold<8>(v);
    default: return mm_x_fold<16>(v);
    }
}
// the prefix XOR of 48 bytes in place, from the class values `in`
template <int D> __device__ __forceinline__ void mm_x_run(u8* v, uint4 in)
{
    u8 r[16];
    const u32 w[4] = { in.x, in.y, in.z, in.w };
#pragma unroll
    for (int c = 0; c < 16; c++) r[c] = (u8)(w[c >> 2] >> (8 * (c & 3)));
#pragma unroll
    for (int k = 0; k < 48; k++) { r[k % D] ^= v[k]; v[k] = r[k % D]; }
}
__device__ __forceinline__ void mm_x_run(u8* v, uint4 in, u32 dist)
{
    switch (dist) {
    case 1: mm_x_run<1>(v, in); break;
    case 2: mm_x_run<2>(v, in); break;
    case 3: mm_x_run<3>(v, in); break;
    case 4: mm_x_run<4>(v, in); break;
    case 8: mm_x_run<8>(v, in); break;
    default: mm_x_run<16>(v, in); break;
    }
}
__device__ __forceinline__ uint4 mm_xor4(uint4 a, uint4 b) { return make_uint4(a.x ^ b.x, a.y ^ b.y, a.z ^ b.z, a.w ^ b.w); }

// inclusive XOR scan of one uint4 per thread over MM_T threads (Hillis-Steele in LDS); sh[MM_T - 1] holds the total afterwards
__device__ uint4 mm_wg_xor_scan(uint4 v, uint4* sh)
{
    const int t = (int)threadIdx.x;
    sh[t] = v;
    __syncthreads();
    for (int o = 1; o < MM_T; o <<= 1) {
        const uint4 prev = (t >= o) ? sh[t - o] : make_uint4(0, 0, 0, 0);
        __syncthreads();
        v = mm_xor4(prev, v);
        sh[t] = v;
        __syncthreads();
    }
    return v;
}

// XOR mode: class totals of every tile of MM_XTILE output bytes
__global__ __launch_bounds__(MM_T) void k_mm_i_xtot(XfStage st, u32* scratch, size_t stride, MmLayout L)
{
    const int b = blockIdx.y;
    u32* ws = scratch + (size_t)b * stride;
    const MmInfo* info = mm_info(ws);
    if (info->mode != MM_XOR) return;
    const u32 n = st.len[b] - 2;
    const u32 t0 = blockIdx.x * MM_XTILE;
    if (t0 >= n) return;
    __shared__ uint4 sh[MM_T];
    u8 v[MM_XSEG];
    mm_x_load(st.src[b], t0 + threadIdx.x * MM_XSEG, n, v);
    mm_wg_xor_scan(mm_x_fold(v, info->dist), sh);
    if (threadIdx.x == 0) reinterpret_cast<uint4*>(ws + L.xt)[blockIdx.x] = sh[MM_T - 1];
}

// XOR mode: what every tile starts from
__global__ __launch_bounds__(MM_T) void k_mm_i_xscan(XfStage st, u32* scratch, size_t stride, MmLayout L)
{
    const int b = blockIdx.x;
    u32* ws = scratch + (size_t)b * stride;
    const MmInfo* info = mm_info(ws);
    if (info->mode != MM_XOR) return;
    const u32 n = st.len[b] - 2;
    const u32 nX = (n + MM_XTILE - 1) / MM_XTILE;
    __shared__ uint4 sh[MM_T];
    uint4* xt = reinterpret_cast<uint4*>(ws + L.xt);
    uint4 carry = make_uint4(0, 0, 0, 0);
    for (u32 base = 0; base < nX; base += MM_T) {
        const u32 j = base + threadIdx.x;
        const uint4 v = (j < nX) ? xt[j] : make_uint4(0, 0, 0, 0);
        const uint4 inc = mm_wg_xor_scan(v, sh);
        if (j < nX) xt[j] = mm_xor4(carry, mm_xor4(inc, v));
        carry = mm_xor4(carry, sh[MM_T - 1]);
        __syncthreads();
    }
}

// XOR mode: the output
__global__ __launch_bounds__(MM_T) void k_mm_i_xapply(XfStage st, u32* scratch, size_t stride, MmLayout L)
{
    const int b = blockIdx.y;
    u32* ws = scratch + (size_t)b * stride;
    const MmInfo* info = mm_info(ws);
    if (info->mode != MM_XOR) return;
    const u32 n = st.len[b] - 2, dist = info->dist;
    const u32 t0 = blockIdx.x * MM_XTILE;
    if (t0 >= n) return;
    __shared__ uint4 sh[MM_T];
    u8 v[MM_XSEG];
    const u32 j0 = t0 + threadIdx.x * MM_XSEG;
    mm_x_load(st.src[b], j0, n, v);
    const uint4 mine = mm_x_fold(v, dist);
    const uint4 inc = mm_wg_xor_scan(mine, sh);
    mm_x_run(v, mm_xor4(reinterpret_cast<const uint4*>(ws + L.xt)[blockIdx.x], mm_xor4(inc, mine)), dist);
    if (j0 >= n) return;
    u8* p = st.dst[b] + j0;
    if (j0 + MM_XSEG <= n && (reinterpret_cast<uintptr_t>(p) & 3) == 0) {
#pragma unroll
        for (int q = 0; q < 12; q++) stg<u32>(p + 4 * q, (u32)v[4 * q] | ((u32)v[4 * q + 1] << 8) | ((u32)v[4 * q + 2] << 16) | ((u32)v[4 * q + 3] << 24));
    } else {
#pragma unroll
        for (u32 k = 0; k < MM_XSEG; k++) if (j0 + k < n) p[k] = v[k];
    }
}

}  // namespace

size_t mm_scratch_bytes(int nBlocks, u32 maxLen) { return (size_t)nBlocks * mm_layout(maxLen).stride * 4 + 256; }

void launch_mm_forward(hipStream_t s, const XfStage& st, void* scratch)
{
    u32* ws = reinterpret_cast<u32*>(scratch);
    const MmLayout L = mm_layout(st.maxLen);
    const unsigned nb = (unsigned)st.nBlocks;
    const dim3 grid((st.maxLen + MM_TILE - 1) / MM_TILE, nb);
    const dim3 gridS(st.maxLen / 5 / MM_TILE + 1, nb);
    { KScope ks_("k_mm_f_init"); hipLaunchKernelGGL(k_mm_f_init, dim3(nb), dim3(MM_T), 0, s, st, ws, L.stride); }
    { KScope ks_("k_mm_f_sample"); hipLaunchKernelGGL(k_mm_f_sample, gridS, dim3(MM_T), 0, s, st, ws, L.stride); }
    { KScope ks_("k_mm_f_decide"); hipLaunchKernelGGL(k_mm_f_decide, dim3(nb), dim3(MM_T), 0, s, st, ws, L.stride); }
    { KScope ks_("k_mm_f_count"); hipLaunchKernelGGL(k_mm_f_count, grid, dim3(MM_T), 0, s, st, ws, L.stride, L); }
    { KScope ks_("k_mm_f_scan"); hipLaunchKernelGGL(k_mm_f_scan, dim3(nb), dim3(MM_T), 0, s, st, ws, L.stride, L); }
    { KScope ks_("k_mm_f_emit"); hipLaunchKernelGGL(k_mm_f_emit, grid, dim3(MM_T), 0, s, st, ws, L.stride, L); }
    { KScope ks_("k_mm_f_finish"); hipLaunchKernelGGL(k_mm_f_finish, dim3(nb), dim3(MM_T), 0, s, st, ws, L.stride); }
}

void launch_mm_inverse(hipStream_t s, const XfStage& st, void* scratch)
{
    u32* ws = reinterpret_cast<u32*>(scratch);
    const MmLayout L = mm_layout(st.maxLen);
    const unsigned nb = (unsigned)st.nBlocks;
    const dim3 grid((st.maxLen + MM_TILE - 1) / MM_TILE, nb);
    const dim3 gridW((st.maxLen / MM_STRETCH + 1 + MM_T / 64 - 1) / (MM_T / 64), nb);
    const dim3 gridX((st.maxLen + MM_XTILE - 1) / MM_XTILE, nb);
    { KScope ks_("k_mm_i_head"); hipLaunchKernelGGL(k_mm_i_head, dim3(nb), dim3(64), 0, s, st, ws, L.stride); }
    { KScope ks_("k_mm_i_last"); hipLaunchKernelGGL(k_mm_i_last, grid, dim3(MM_T), 0, s, st, ws, L.stride); }
    { KScope ks_("k_mm_i_count"); hipLaunchKernelGGL(k_mm_i_count, grid, dim3(MM_T), 0, s, st, ws, L.stride, L); }
    { KScope ks_("k_mm_i_scan"); hipLaunchKernelGGL(k_mm_i_scan, dim3(nb), dim3(MM_T), 0, s, st, ws, L.stride, L); }
    { KScope ks_("k_mm_i_steps"); hipLaunchKernelGGL(k_mm_i_steps, grid, dim3(MM_T), 0, s, st, ws, L.stride, L); }
    { KScope ks_("k_mm_i_maps"); hipLaunchKernelGGL(k_mm_i_maps, gridW, dim3(MM_T), 0, s, st, ws, L.stride, L); }
    { KScope ks_("k_mm_i_chain"); hipLaunchKernelGGL(k_mm_i_chain, dim3(16, nb), dim3(MM_T), 0, s, st, ws, L.stride, L); }
    { KScope ks_("k_mm_i_apply"); hipLaunchKernelGGL(k_mm_i_apply, gridW, dim3(MM_T), 0, s, st, ws, L.stride, L); }
    { KScope ks_("k_mm_i_xtot"); hipLaunchKernelGGL(k_mm_i_xtot, gridX, dim3(MM_T), 0, s, st, ws, L.stride, L); }
    { KScope ks_("k_mm_i_xscan"); hipLaunchKernelGGL(k_mm_i_xscan, dim3(nb), dim3(MM_T), 0, s, st, ws, L.stride, L); }
    { KScope ks_("k_mm_i_xapply"); hipLaunchKernelGGL(k_mm_i_xapply, gridX, dim3(MM_T), 0, s, st, ws, L.stride, L); }
}

}  // namespace knz
