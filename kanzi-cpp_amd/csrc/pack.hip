// PACK (AliasCodec, kanzi transform id 18) on gfx950, forward and inverse: every block of a batch in the same launches.
//
// Reference being replaced: transform/AliasCodec.cpp:38-209 (forward), :211-371 (inverse), the alias order
// AliasCodec.hpp:28-35 (frequency descending, then value descending) and Global.cpp:272-306 (the order-1 histogram,
// which also counts the pair (0, src[0])).
//
// Forward modes by the number n0 of absent byte values: one symbol (255), 2-bit packing (>= 252), 4-bit packing (>= 240)
// and digram aliasing (16 .. 239). The packing modes are element-wise. The digram parse is a greedy left-to-right walk
// whose steps move 1 or 2 bytes, so a stretch of positions is a function of its entry state (0: it starts on a token,
// 1: its first byte belongs to the previous token) to its exit state plus a token count. A thread walks 16 positions for
// both entries, a workgroup composes the 256 functions of its chunk, one workgroup per block composes the chunk
// functions, and a second pass re-walks each 16-byte stretch from its known entry and writes at its known offset.
// The top n0 pairs come from a threshold search over the 65,536-bin pair histogram (one workgroup per block).
//
// Inverse: every input byte of the digram mode expands to 1 or 2 bytes with no state, so a prefix sum of the lengths
// places the output; the packing modes are element-wise. The guards of AliasCodec::inverse are evaluated before any
// byte is written, and nothing is written for a block they reject.
#include "common.hpp"
#include "stages.hpp"
#include "datatype.hpp"

namespace knz {

namespace {

constexpr int PK_T = 256;                       // threads per workgroup (chunk kernels)
constexpr int PK_SEG = 16;                      // positions per thread
constexpr u32 PK_CHUNK = PK_T * PK_SEG;         // positions per workgroup
constexpr u32 PK_MIN = 1024;                    // AliasCodec::MIN_BLOCK_SIZE
constexpr int PK_SEL_T = 1024;                  // threads of the pair selection (64 bins each)

enum { PK_NONE = 0, PK_ONE = 1, PK_BITS2 = 2, PK_BITS4 = 3, PK_DIGRAM = 4 };

// per-block scratch (u32 words)
constexpr u32 PK_H0 = 0;                        // [256] order-0 histogram
constexpr u32 PK_PAIRS = 256;                   // [65536] pair histogram, then the alias map (0x200 | alias, 0 = none)
constexpr u32 PK_INFO = PK_PAIRS + 65536;       // [128] see PkInfo
constexpr u32 PK_MAP = PK_INFO + 128;           // [256] map8 (forward) / alias -> pair map (inverse)
constexpr u32 PK_CH = PK_MAP + 256;             // [4 per chunk] chunk function / chunk offset + entry

struct PkInfo {
    u32 mode;       // PK_*
    u32 n0;         // aliases (digram) / absent symbols
    u32 hdr;        // header bytes (forward digram) / first payload byte (inverse)
    u32 end;        // inverse: end of the payload
    u32 total;      // output bytes
    u32 ok;
    u32 adjust;
    u32 absent[240 / 4];   // absent symbols of the digram mode, 4 per word
};
static_assert(sizeof(PkInfo) <= 128 * 4, "PkInfo too large");

__host__ __device__ inline size_t pk_stride_u32(u32 maxLen)
{
    const size_t chunks = (maxLen + PK_CHUNK - 1) / PK_CHUNK + 1;
    return (PK_CH + 4 * chunks + 63) & ~(size_t)63;
}

// the state function of a stretch of the digram parse: entry e -> exit x[e], c[e] tokens
struct PkFn { u32 c0, c1, x0, x1; };
__device__ __forceinline__ PkFn pk_ident() { return PkFn{ 0u, 0u, 0u, 1u }; }
__device__ __forceinline__ PkFn pk_then(const PkFn& f, const PkFn& g)      // f, then g
{
    PkFn r;
    r.x0 = f.x0 ? g.x1 : g.x0; r.c0 = f.c0 + (f.x0 ? g.c1 : g.c0);
    r.x1 = f.x1 ? g.x1 : g.x0; r.c1 = f.c1 + (f.x1 ? g.c1 : g.c0);
    return r;
}
__device__ __forceinline__ u32 pk_x(const PkFn& f, u32 e) { return e ? f.x1 : f.x0; }
__device__ __forceinline__ u32 pk_c(const PkFn& f, u32 e) { return e ? f.c1 : f.c0; }

// inclusive scan of one PkFn per thread over PK_T threads (Hillis-Steele in LDS)
__device__ PkFn pk_wg_scan(PkFn v, PkFn* sh)
{
    const int t = (int)threadIdx.x;
    sh[t] = v;
    __syncthreads();
    for (int o = 1; o < PK_T; o <<= 1) {
        const PkFn prev = (t >= o) ? sh[t - o] : pk_ident();
        __syncthreads();
        if (t >= o) v = pk_then(prev, v);
        sh[t] = v;
        __syncthreads();
    }
    return v;
}

// inclusive sum over PK_T threads
__device__ u32 pk_wg_sum(u32 v, u32* sh /* [4] */, u32* total)
{
    const int lane = lane_id(), wave = (int)(threadIdx.x >> 6);
    for (int o = 1; o < 64; o <<= 1) { const u32 t = (u32)__shfl_up((int)v, (unsigned)o, 64); if (lane >= o) v += t; }
    if (lane == 63) sh[wave] = v;
    __syncthreads();
    u32 carry = 0, tot = 0;
    for (int w = 0; w < PK_T / 64; w++) { if (w < wave) carry += sh[w]; tot += sh[w]; }
    __syncthreads();
    *total = tot;
    return carry + v;
}

// the digram parse over positions [a, b) (b <= L = count - 1) from entry e; alias map in global memory
__device__ __forceinline__ PkFn pk_walk(const u8* __restrict__ src, const u32* __restrict__ amap, u32 a, u32 b)
{
    PkFn f;
    u32 xs[2], cs[2];
#pragma unroll
    for (u32 e = 0; e < 2; e++) {
        u32 p = a + e, c = 0;
        while (p < b) {
            const u32 m = amap[((u32)src[p] << 8) | src[p + 1]];
            p += m ? 2u : 1u;
            c++;
        }
        xs[e] = p - b; cs[e] = c;
    }
    f.x0 = xs[0]; f.x1 = xs[1]; f.c0 = cs[0]; f.c1 = cs[1];
    return f;
}

// ---------------------------------------------------------------------------------------------------------------------
// forward
// ---------------------------------------------------------------------------------------------------------------------

// early refusals (AliasCodec.cpp:40-72) and zeroed histogram
__global__ __launch_bounds__(PK_T) void k_pk_f_init(XfStage st, u32* scratch, size_t stride)
{
    const int b = blockIdx.x;
    u32* ws = scratch + (size_t)b * stride;
    PkInfo* info = reinterpret_cast<PkInfo*>(ws + PK_INFO);
    ws[PK_H0 + threadIdx.x] = 0;
    if (threadIdx.x != 0) return;
    const u32 n = st.len[b];
    u32 mode = PK_DIGRAM;
    if (n == 0 || n < PK_MIN || (u64)st.cap[b] < (u64)n + 1024) mode = PK_NONE;
    if (st.dtype) {
        const int dt = st.dtype[b];
        if (dt == DT_MULTIMEDIA || dt == DT_UTF8 || dt == DT_EXE || dt == DT_BIN) mode = PK_NONE;
        if (st.onlyDNA && dt != DT_UNDEFINED && dt != DT_DNA) mode = PK_NONE;                   // AliasCodec.cpp:66 (the DNA transform)
    }
    info->mode = mode;
    info->ok = 0;
    st.ok[b] = (n == 0) ? 1 : 0;            // AliasCodec::forward returns true for an empty block
    st.newLen[b] = 0;
}

__global__ __launch_bounds__(PK_T) void k_pk_f_hist0(XfStage st, u32* scratch, size_t stride)
{
    const int b = blockIdx.y;
    u32* ws = scratch + (size_t)b * stride;
    if (reinterpret_cast<const PkInfo*>(ws + PK_INFO)->mode == PK_NONE) return;
    const u32 n = st.len[b];
    const u32 a = blockIdx.x * PK_CHUNK;
    if (a >= n) return;
    __shared__ u32 h[256];
    h[threadIdx.x] = 0;
    __syncthreads();
    const u8* __restrict__ src = st.src[b];
    const u32 e = (n - a < PK_CHUNK) ? n : a + PK_CHUNK;
    for (u32 i = a + threadIdx.x; i < e; i += PK_T) atomicAdd(&h[src[i]], 1u);
    __syncthreads();
    if (h[threadIdx.x]) atomicAdd(&ws[PK_H0 + threadIdx.x], h[threadIdx.x]);
}

// n0, the data type, the mode; the header of the packing modes; zeroed pair histogram for the digram mode
__global__ __launch_bounds__(PK_T) void k_pk_f_decide(XfStage st, u32* scratch, size_t stride)
{
    const int b = blockIdx.x;
    u32* ws = scratch + (size_t)b * stride;
    PkInfo* info = reinterpret_cast<PkInfo*>(ws + PK_INFO);
    if (info->mode == PK_NONE) return;
    const u32 n = st.len[b];
    const int t = (int)threadIdx.x;
    __shared__ u32 f0[256];
    __shared__ u32 sh[4];
    __shared__ int s_mode;
    f0[t] = ws[PK_H0 + t];
    __syncthreads();
    u32 nAbsent;
    const u32 absentRank = pk_wg_sum(f0[t] == 0 ? 1u : 0u, sh, &nAbsent) - (f0[t] == 0 ? 1u : 0u);
    u32 nPresent = 256 - nAbsent;
    const u32 presentRank = (u32)t - absentRank;
    if (t == 0) {
        int mode = PK_DIGRAM;
        if (nAbsent < 16) mode = PK_NONE;
        else {
            int dt = st.dtype ? st.dtype[b] : DT_UNDEFINED;
            if (dt == DT_UNDEFINED) {
                dt = pk_simple_type(n, f0);
                if (st.dtype && dt != DT_UNDEFINED) st.dtype[b] = (u8)dt;
                if (st.onlyDNA && dt != DT_DNA) mode = PK_NONE;                                 // AliasCodec.cpp:93: the type is written first
            }
            if (mode == PK_NONE) ;
            else if (nAbsent == 255) mode = PK_ONE;
            else if (nAbsent >= 252) mode = PK_BITS2;
            else if (nAbsent >= 240) mode = PK_BITS4;
        }
        s_mode = mode;
        info->mode = (u32)mode;
        info->n0 = nAbsent;
    }
    __syncthreads();
    const int mode = s_mode;
    if (mode == PK_NONE) return;
    u8* __restrict__ dst = st.dst[b];
    const u8* __restrict__ src = st.src[b];
    if (mode == PK_DIGRAM) {
        if (f0[t] == 0) reinterpret_cast<u8*>(info->absent)[absentRank] = (u8)t;
        for (u32 i = (u32)t; i < 65536; i += PK_T) ws[PK_PAIRS + i] = 0;
        return;
    }
    // packing modes (AliasCodec.cpp:83-128): header, map8, output length
    u32 total;
    if (mode == PK_ONE) {
        if (t == 0) {
            dst[0] = (u8)nAbsent; dst[1] = src[0];
            dst[2] = (u8)n; dst[3] = (u8)(n >> 8); dst[4] = (u8)(n >> 16); dst[5] = (u8)(n >> 24);
        }
        total = 6;
    } else {
        if (f0[t] != 0) { dst[1 + presentRank] = (u8)t; ws[PK_MAP + t] = presentRank; }
        const u32 h = 1 + nPresent;
        if (t == 0) dst[0] = (u8)nAbsent;
        if (mode == PK_BITS2) {
            const u32 c3 = n & 3;
            if (t == 0) dst[h] = (u8)c3;
            if ((u32)t < c3) dst[h + 1 + t] = src[t];
            total = h + 1 + c3 + (n - c3) / 4;
        } else {
            const u32 c1 = n & 1;
            if (t == 0) { dst[h] = (u8)c1; if (c1) dst[h + 1] = src[0]; }
            total = h + 1 + c1 + (n - c1) / 2;
        }
        if (t == 0) info->hdr = h + 1 + ((mode == PK_BITS2) ? (n & 3) : (n & 1));
    }
    if (t == 0) {
        info->total = total;
        info->ok = total < n ? 1u : 0u;
        st.ok[b] = (u8)info->ok;
        st.newLen[b] = info->ok ? total : 0u;
    }
}

// packed payload of the 2-bit and 4-bit modes
__global__ __launch_bounds__(PK_T) void k_pk_f_pack(XfStage st, u32* scratch, size_t stride)
{
    const int b = blockIdx.y;
    const u32* ws = scratch + (size_t)b * stride;
    const PkInfo* info = reinterpret_cast<const PkInfo*>(ws + PK_INFO);
    const u32 mode = info->mode;
    if ((mode != PK_BITS2 && mode != PK_BITS4) || !info->ok) return;
    __shared__ u32 map8[256];
    map8[threadIdx.x] = ws[PK_MAP + threadIdx.x];
    __syncthreads();
    const u32 n = st.len[b];
    const u8* __restrict__ src = st.src[b];
    u8* __restrict__ dst = st.dst[b] + info->hdr;
    if (mode == PK_BITS2) {
        const u32 c3 = n & 3, m = (n - c3) / 4;
        for (u32 j = blockIdx.x * PK_T + threadIdx.x; j < m; j += gridDim.x * PK_T) {
            const u8* s = src + c3 + 4 * j;
            dst[j] = (u8)((map8[s[0]] << 6) | (map8[s[1]] << 4) | (map8[s[2]] << 2) | map8[s[3]]);
        }
    } else {
        const u32 c1 = n & 1, m = (n - c1) / 2;
        for (u32 j = blockIdx.x * PK_T + threadIdx.x; j < m; j += gridDim.x * PK_T) {
            const u8* s = src + c1 + 2 * j;
            dst[j] = (u8)((map8[s[0]] << 4) | map8[s[1]]);
        }
    }
}

// order-1 histogram of the digram mode, phantom pair (0, src[0]) included
__global__ __launch_bounds__(PK_T) void k_pk_f_hist1(XfStage st, u32* scratch, size_t stride)
{
    const int b = blockIdx.y;
    u32* ws = scratch + (size_t)b * stride;
    if (reinterpret_cast<const PkInfo*>(ws + PK_INFO)->mode != PK_DIGRAM) return;
    const u32 n = st.len[b];
    const u8* __restrict__ src = st.src[b];
    for (u32 i = blockIdx.x * PK_CHUNK + threadIdx.x; i < n && i < (blockIdx.x + 1) * PK_CHUNK; i += PK_T) {
        const u32 prev = i ? src[i - 1] : 0u;
        atomicAdd(&ws[PK_PAIRS + ((prev << 8) | src[i])], 1u);
    }
}

__device__ u32 pk_sel_sum(u32 v, u32* sh /* [16] */)
{
    const int lane = lane_id(), wave = (int)(threadIdx.x >> 6);
    for (int o = 32; o > 0; o >>= 1) v += (u32)__shfl_xor((int)v, o, 64);
    if (lane == 0) sh[wave] = v;
    __syncthreads();
    u32 tot = 0;
    for (int w = 0; w < PK_SEL_T / 64; w++) tot += sh[w];
    __syncthreads();
    return tot;
}

// the n0 most frequent pairs in sdAlias order (AliasCodec.cpp:131-186), the savings test, the header and the alias map
__global__ __launch_bounds__(PK_SEL_T) void k_pk_f_select(XfStage st, u32* scratch, size_t stride)
{
    const int b = blockIdx.x;
    u32* ws = scratch + (size_t)b * stride;
    PkInfo* info = reinterpret_cast<PkInfo*>(ws + PK_INFO);
    if (info->mode != PK_DIGRAM) return;
    const int t = (int)threadIdx.x;
    const u32 n = st.len[b];
    __shared__ u32 sh[16];
    __shared__ u32 selVal[256], selFreq[256], order[256];
    __shared__ u32 nSel;
    __shared__ u32 tiesAbove[PK_SEL_T];
    const uint4* bins = reinterpret_cast<const uint4*>(ws + PK_PAIRS + 64 * t);
    u32 nz = 0, mx = 0;
    for (int q = 0; q < 16; q++) {
        const uint4 v = bins[q];
        nz += (v.x != 0) + (v.y != 0) + (v.z != 0) + (v.w != 0);
        mx = max(mx, max(max(v.x, v.y), max(v.z, v.w)));
    }
    const u32 n1 = pk_sel_sum(nz, sh);
    for (int o = 32; o > 0; o >>= 1) mx = max(mx, (u32)__shfl_xor((int)mx, o, 64));
    if (lane_id() == 0) sh[t >> 6] = mx;
    __syncthreads();
    u32 maxF = 0;
    for (int w = 0; w < PK_SEL_T / 64; w++) maxF = max(maxF, sh[w]);
    __syncthreads();
    u32 k = info->n0;
    if (n1 < k) k = n1;
    if (k < 16) {
        if (t == 0) { info->mode = PK_NONE; info->ok = 0; }
        return;
    }
    // largest T with at least k bins >= T
    u32 lo = 1, hi = maxF;
    while (lo < hi) {
        const u32 mid = lo + (hi - lo + 1) / 2;
        u32 c = 0;
        for (int q = 0; q < 16; q++) {
            const uint4 v = bins[q];
            c += (v.x >= mid) + (v.y >= mid) + (v.z >= mid) + (v.w >= mid);
        }
        if (pk_sel_sum(c, sh) >= k) lo = mid; else hi = mid - 1;
    }
    const u32 T = lo;
    u32 gt = 0, eq = 0;
    for (int q = 0; q < 16; q++) {
        const uint4 v = bins[q];
        gt += (v.x > T) + (v.y > T) + (v.z > T) + (v.w > T);
        eq += (v.x == T) + (v.y == T) + (v.z == T) + (v.w == T);
    }
    const u32 nGt = pk_sel_sum(gt, sh);
    const u32 need = k - nGt;               // ties taken by value, largest first
    tiesAbove[t] = eq;
    if (t == 0) nSel = 0;
    __syncthreads();
    // ties held by higher threads (higher values): suffix sum
    for (int o = 1; o < PK_SEL_T; o <<= 1) {
        const u32 add = (t + o < PK_SEL_T) ? tiesAbove[t + o] : 0u;
        __syncthreads();
        tiesAbove[t] += add;
        __syncthreads();
    }
    u32 above = tiesAbove[t] - eq;
    for (int j = 63; j >= 0; j--) {
        const u32 v = 64u * (u32)t + (u32)j;
        const u32 f = ws[PK_PAIRS + v];
        bool take = f > T;
        if (f == T) { take = above < need; above++; }
        if (take) { const u32 s = atomicAdd(&nSel, 1u); if (s < 256) { selVal[s] = v; selFreq[s] = f; } }
    }
    __syncthreads();
    u32 savings = 0;
    if ((u32)t < k) {
        const u32 fi = selFreq[t], vi = selVal[t];
        u32 r = 0;
        for (u32 m = 0; m < k; m++) r += (selFreq[m] > fi || (selFreq[m] == fi && selVal[m] > vi)) ? 1u : 0u;
        order[r] = (u32)t;
        savings = fi;
    }
    savings = pk_sel_sum(savings, sh);
    if (savings < n / 20) {
        if (t == 0) { info->mode = PK_NONE; info->ok = 0; }
        return;
    }
    u8* __restrict__ dst = st.dst[b];
    const u8* absent = reinterpret_cast<const u8*>(info->absent);
    for (int j = 0; j < 64; j++) ws[PK_PAIRS + 64 * t + j] = 0;
    __syncthreads();
    if ((u32)t < k) {
        const u32 v = selVal[order[t]];
        const u8 al = absent[t];
        ws[PK_PAIRS + v] = 0x200u | al;
        dst[2 + 3 * t] = (u8)(v >> 8);
        dst[3 + 3 * t] = (u8)v;
        dst[4 + 3 * t] = al;
    }
    if (t == 0) {
        dst[0] = (u8)k;
        dst[1] = 0;
        info->n0 = k;
        info->hdr = 2 + 3 * k;
    }
}

// pass 1: the state function of every chunk of parse positions [0, n - 1)
__global__ __launch_bounds__(PK_T) void k_pk_f_parse_fn(XfStage st, u32* scratch, size_t stride)
{
    const int b = blockIdx.y;
    u32* ws = scratch + (size_t)b * stride;
    if (reinterpret_cast<const PkInfo*>(ws + PK_INFO)->mode != PK_DIGRAM) return;
    const u32 L = st.len[b] - 1;
    const u32 c0 = blockIdx.x * PK_CHUNK;
    if (c0 >= L) return;
    __shared__ PkFn sh[PK_T];
    const u32 a = min(c0 + threadIdx.x * PK_SEG, L), e = min(a + PK_SEG, L);
    const PkFn f = pk_wg_scan(pk_walk(st.src[b], ws + PK_PAIRS, a, e), sh);
    if (threadIdx.x == PK_T - 1) {
        u32* o = ws + PK_CH + 4 * blockIdx.x;
        o[0] = f.c0; o[1] = f.c1; o[2] = f.x0; o[3] = f.x1;
    }
}

// pass 2 (one workgroup per block): every chunk's entry state and token offset, the trailing byte, ok and length
__global__ __launch_bounds__(PK_T) void k_pk_f_parse_scan(XfStage st, u32* scratch, size_t stride)
{
    const int b = blockIdx.x;
    u32* ws = scratch + (size_t)b * stride;
    PkInfo* info = reinterpret_cast<PkInfo*>(ws + PK_INFO);
    if (info->mode != PK_DIGRAM) return;
    const u32 n = st.len[b], L = n - 1;
    const u32 nCh = (L + PK_CHUNK - 1) / PK_CHUNK;
    __shared__ PkFn sh[PK_T];
    u32 state = 0, cnt = 0;
    for (u32 base = 0; base < nCh; base += PK_T) {
        const u32 j = base + threadIdx.x;
        PkFn f = pk_ident();
        if (j < nCh) { const u32* o = ws + PK_CH + 4 * j; f = PkFn{ o[0], o[1], o[2], o[3] }; }
        pk_wg_scan(f, sh);
        const PkFn exc = threadIdx.x ? sh[threadIdx.x - 1] : pk_ident();
        if (j < nCh) {
            u32* o = ws + PK_CH + 4 * j;
            o[0] = cnt + pk_c(exc, state);
            o[1] = pk_x(exc, state);
        }
        const PkFn all = sh[PK_T - 1];
        __syncthreads();
        cnt += pk_c(all, state);
        state = pk_x(all, state);
    }
    if (threadIdx.x == 0) {
        const u32 hdr = info->hdr;
        const u32 total = hdr + cnt + (state == 0 ? 1u : 0u);
        const u32 ok = total < n ? 1u : 0u;
        if (ok && state == 0) {             // the parse stopped on the last byte: adjust (AliasCodec.cpp:199-202)
            u8* dst = st.dst[b];
            dst[1] = 1;
            dst[hdr + cnt] = st.src[b][n - 1];
        }
        info->ok = ok;
        info->total = total;
        st.ok[b] = (u8)ok;
        st.newLen[b] = ok ? total : 0u;
    }
}

// pass 3: the aliased bytes
__global__ __launch_bounds__(PK_T) void k_pk_f_parse_emit(XfStage st, u32* scratch, size_t stride)
{
    const int b = blockIdx.y;
    const u32* ws = scratch + (size_t)b * stride;
    const PkInfo* info = reinterpret_cast<const PkInfo*>(ws + PK_INFO);
    if (info->mode != PK_DIGRAM || !info->ok) return;
    const u32 L = st.len[b] - 1;
    const u32 c0 = blockIdx.x * PK_CHUNK;
    if (c0 >= L) return;
    __shared__ PkFn sh[PK_T];
    const u8* __restrict__ src = st.src[b];
    const u32* __restrict__ amap = ws + PK_PAIRS;
    const u32 a = min(c0 + threadIdx.x * PK_SEG, L), e = min(a + PK_SEG, L);
    pk_wg_scan(pk_walk(src, amap, a, e), sh);
    const PkFn exc = threadIdx.x ? sh[threadIdx.x - 1] : pk_ident();
    const u32 chOff = ws[PK_CH + 4 * blockIdx.x], chEntry = ws[PK_CH + 4 * blockIdx.x + 1];
    u32 o = info->hdr + chOff + pk_c(exc, chEntry);
    u32 p = a + pk_x(exc, chEntry);
    u8* __restrict__ dst = st.dst[b];
    while (p < e) {
        const u32 m = amap[((u32)src[p] << 8) | src[p + 1]];
        dst[o++] = m ? (u8)m : src[p];
        p += m ? 2u : 1u;
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// inverse
// ---------------------------------------------------------------------------------------------------------------------

// header, guards and the mode (AliasCodec.cpp:211-280, :316-333); for the digram mode the alias map
__global__ __launch_bounds__(64) void k_pk_i_head(XfStage st, u32* scratch, size_t stride)
{
    const int b = blockIdx.x;
    u32* ws = scratch + (size_t)b * stride;
    PkInfo* info = reinterpret_cast<PkInfo*>(ws + PK_INFO);
    const u32 count = st.len[b];
    if (threadIdx.x == 0) info->mode = PK_NONE;
    if (count == 0) { if (threadIdx.x == 0) { st.ok[b] = 1; st.newLen[b] = 0; } return; }
    const u8* __restrict__ src = st.src[b];
    const u32 dstEnd = st.cap[b];
    const u32 n0 = src[0];
    if (n0 >= 16 && n0 < 240) {
        if (count < 2 || src[1] > 1) { if (threadIdx.x == 0) { st.ok[b] = 0; st.newLen[b] = 0; } return; }
        const u32 adjust = src[1];
        const u32 end = count - adjust;
        if (2 + 3 * n0 > end) { if (threadIdx.x == 0) { st.ok[b] = 0; st.newLen[b] = 0; } return; }
        for (u32 i = threadIdx.x; i < 256; i += 64) ws[PK_MAP + i] = 0x10000u | i;
        __syncthreads();
        if (threadIdx.x == 0) {
            for (u32 i = 0; i < n0; i++) {           // later entries win, as in the reference
                const u8* e = src + 2 + 3 * i;
                ws[PK_MAP + e[2]] = 0x20000u | e[0] | ((u32)e[1] << 8);
            }
            info->mode = PK_DIGRAM; info->hdr = 2 + 3 * n0; info->end = end; info->adjust = adjust; info->ok = 0;
        }
        return;
    }
    if (threadIdx.x != 0) return;
    bool ok = false;
    u32 mode = PK_NONE, total = 0, hdr = 0, adjust = 0;
    if (n0 >= 240) {
        const u32 n = 256 - n0;
        if (n == 1) {
            if (count >= 6) {
                const int oSize = (int)((u32)src[2] | ((u32)src[3] << 8) | ((u32)src[4] << 16) | ((u32)src[5] << 24));
                if (oSize >= 0 && (u32)oSize <= dstEnd) { ok = true; mode = PK_ONE; total = (u32)oSize; hdr = 1; }
            }
        } else if (1 + n + 1 <= count) {
            for (u32 i = 0; i < 16; i++) ws[PK_MAP + i] = (i < n) ? src[1 + i] : 0u;
            adjust = src[1 + n];
            u32 si = 2 + n;
            if (adjust < 4) {
                if (n <= 4) {
                    if (si + adjust <= count && adjust <= dstEnd && (count - si - adjust) <= ((dstEnd - adjust) >> 2)) {
                        ok = true; mode = PK_BITS2; hdr = si; total = adjust + 4 * (count - si - adjust);
                    }
                } else {
                    const u32 lead = adjust ? 1u : 0u;
                    if ((!lead || (si < count && dstEnd > 0)) && (count - si - lead) <= ((dstEnd - lead) >> 1)) {
                        ok = true; mode = PK_BITS4; hdr = si; adjust = lead; total = lead + 2 * (count - si - lead);
                    }
                }
            }
        }
    }
    info->mode = ok ? mode : PK_NONE;
    info->hdr = hdr; info->adjust = adjust; info->total = total; info->ok = ok ? 1u : 0u;
    st.ok[b] = ok ? 1 : 0;
    st.newLen[b] = ok ? total : 0u;
}

// digram mode: output bytes of every chunk of the payload
__global__ __launch_bounds__(PK_T) void k_pk_i_count(XfStage st, u32* scratch, size_t stride)
{
    const int b = blockIdx.y;
    u32* ws = scratch + (size_t)b * stride;
    const PkInfo* info = reinterpret_cast<const PkInfo*>(ws + PK_INFO);
    if (info->mode != PK_DIGRAM) return;
    const u32 beg = info->hdr, end = info->end;
    const u32 c0 = beg + blockIdx.x * PK_CHUNK;
    if (c0 >= end) return;
    __shared__ u32 map[256];
    __shared__ u32 sh[4];
    map[threadIdx.x] = ws[PK_MAP + threadIdx.x];
    __syncthreads();
    const u8* __restrict__ src = st.src[b];
    u32 c = 0;
    for (u32 i = c0 + threadIdx.x; i < end && i < c0 + PK_CHUNK; i += PK_T) c += map[src[i]] >> 16;
    u32 tot;
    pk_wg_sum(c, sh, &tot);
    if (threadIdx.x == 0) ws[PK_CH + blockIdx.x] = tot;
}

// digram mode: chunk offsets, the size guards and the trailing byte (AliasCodec.cpp:335-364)
__global__ __launch_bounds__(PK_T) void k_pk_i_scan(XfStage st, u32* scratch, size_t stride)
{
    const int b = blockIdx.x;
    u32* ws = scratch + (size_t)b * stride;
    PkInfo* info = reinterpret_cast<PkInfo*>(ws + PK_INFO);
    if (info->mode != PK_DIGRAM) return;
    const u32 nCh = (info->end - info->hdr + PK_CHUNK - 1) / PK_CHUNK;
    __shared__ u32 sh[4];
    u64 carry = 0;
    for (u32 base = 0; base < nCh; base += PK_T) {
        const u32 j = base + threadIdx.x;
        const u32 v = (j < nCh) ? ws[PK_CH + j] : 0u;
        u32 tot;
        const u32 inc = pk_wg_sum(v, sh, &tot);
        if (j < nCh) ws[PK_CH + j] = (u32)(carry + inc - v);
        carry += tot;
    }
    if (threadIdx.x == 0) {
        const u64 dstEnd = st.cap[b];
        bool ok = carry <= dstEnd;
        u64 total = carry;
        if (ok && info->adjust) {
            ok = carry < dstEnd;
            if (ok) { st.dst[b][carry] = st.src[b][st.len[b] - 1]; total++; }
        }
        info->ok = ok ? 1u : 0u;
        info->total = (u32)total;
        st.ok[b] = ok ? 1 : 0;
        st.newLen[b] = ok ? (u32)total : 0u;
    }
}

__global__ __launch_bounds__(PK_T) void k_pk_i_emit(XfStage st, u32* scratch, size_t stride)
{
    const int b = blockIdx.y;
    const u32* ws = scratch + (size_t)b * stride;
    const PkInfo* info = reinterpret_cast<const PkInfo*>(ws + PK_INFO);
    const u32 mode = info->mode;
    if (mode == PK_NONE || !info->ok) return;
    const u8* __restrict__ src = st.src[b];
    u8* __restrict__ dst = st.dst[b];
    const u32 count = st.len[b];
    const u32 gsz = gridDim.x * PK_T;
    const u32 g = blockIdx.x * PK_T + threadIdx.x;
    if (mode == PK_ONE) {
        const u8 v = src[1];
        for (u32 i = g; i < info->total; i += gsz) dst[i] = v;
        return;
    }
    if (mode == PK_BITS2 || mode == PK_BITS4) {
        u8 sym[16];
#pragma unroll
        for (int i = 0; i < 16; i++) sym[i] = (u8)ws[PK_MAP + i];
        const u32 hdr = info->hdr, adj = info->adjust;
        for (u32 i = g; i < adj; i += gsz) dst[i] = src[hdr + i];
        const u32 p0 = hdr + adj;
        if (mode == PK_BITS2) {
            for (u32 i = g; p0 + i < count; i += gsz) {
                const u32 v = src[p0 + i];
                u8* d = dst + adj + 4 * i;
                d[0] = sym[(v >> 6) & 3]; d[1] = sym[(v >> 4) & 3]; d[2] = sym[(v >> 2) & 3]; d[3] = sym[v & 3];
            }
        } else {
            for (u32 i = g; p0 + i < count; i += gsz) {
                const u32 v = src[p0 + i];
                dst[adj + 2 * i] = sym[v >> 4];
                dst[adj + 2 * i + 1] = sym[v & 15];
            }
        }
        return;
    }
    // digram
    const u32 beg = info->hdr, end = info->end;
    const u32 c0 = beg + blockIdx.x * PK_CHUNK;
    if (c0 >= end) return;
    __shared__ u32 map[256];
    __shared__ u32 sh[4];
    map[threadIdx.x] = ws[PK_MAP + threadIdx.x];
    __syncthreads();
    const u32 a = min(c0 + threadIdx.x * PK_SEG, end), e = min(a + PK_SEG, end);
    u32 c = 0;
    for (u32 i = a; i < e; i++) c += map[src[i]] >> 16;
    u32 tot;
    u32 o = ws[PK_CH + blockIdx.x] + pk_wg_sum(c, sh, &tot) - c;
    for (u32 i = a; i < e; i++) {
        const u32 v = map[src[i]];
        dst[o] = (u8)v;
        if (v >> 17) dst[o + 1] = (u8)(v >> 8);
        o += v >> 16;
    }
}

}  // namespace

size_t pack_scratch_bytes(int nBlocks, u32 maxLen) { return (size_t)nBlocks * pk_stride_u32(maxLen) * 4 + 256; }

void launch_pack_forward(hipStream_t s, const XfStage& st, void* scratch)
{
    u32* ws = reinterpret_cast<u32*>(scratch);
    const size_t stride = pk_stride_u32(st.maxLen);
    const dim3 grid((st.maxLen + PK_CHUNK - 1) / PK_CHUNK, (unsigned)st.nBlocks);
    hipLaunchKernelGGL(k_pk_f_init, dim3(st.nBlocks), dim3(PK_T), 0, s, st, ws, stride);
    hipLaunchKernelGGL(k_pk_f_hist0, grid, dim3(PK_T), 0, s, st, ws, stride);
    hipLaunchKernelGGL(k_pk_f_decide, dim3(st.nBlocks), dim3(PK_T), 0, s, st, ws, stride);
    hipLaunchKernelGGL(k_pk_f_pack, grid, dim3(PK_T), 0, s, st, ws, stride);
    hipLaunchKernelGGL(k_pk_f_hist1, grid, dim3(PK_T), 0, s, st, ws, stride);
    hipLaunchKernelGGL(k_pk_f_select, dim3(st.nBlocks), dim3(PK_SEL_T), 0, s, st, ws, stride);
    hipLaunchKernelGGL(k_pk_f_parse_fn, grid, dim3(PK_T), 0, s, st, ws, stride);
    hipLaunchKernelGGL(k_pk_f_parse_scan, dim3(st.nBlocks), dim3(PK_T), 0, s, st, ws, stride);
    hipLaunchKernelGGL(k_pk_f_parse_emit, grid, dim3(PK_T), 0, s, st, ws, stride);
}

void launch_pack_inverse(hipStream_t s, const XfStage& st, void* scratch)
{
    u32* ws = reinterpret_cast<u32*>(scratch);
    const size_t stride = pk_stride_u32(st.maxLen);
    const dim3 grid((st.maxLen + PK_CHUNK - 1) / PK_CHUNK, (unsigned)st.nBlocks);
    // (the one-symbol mode writes up to cap bytes from 6: the emit grid follows the output bound when the host knows it)
    const u32 outMax = st.maxCap > st.maxLen ? st.maxCap : st.maxLen;
    const dim3 gridOut((outMax + PK_CHUNK - 1) / PK_CHUNK, (unsigned)st.nBlocks);
    hipLaunchKernelGGL(k_pk_i_head, dim3(st.nBlocks), dim3(64), 0, s, st, ws, stride);
    hipLaunchKernelGGL(k_pk_i_count, grid, dim3(PK_T), 0, s, st, ws, stride);
    hipLaunchKernelGGL(k_pk_i_scan, dim3(st.nBlocks), dim3(PK_T), 0, s, st, ws, stride);
    hipLaunchKernelGGL(k_pk_i_emit, gridOut, dim3(PK_T), 0, s, st, ws, stride);
}

}  // namespace knz
