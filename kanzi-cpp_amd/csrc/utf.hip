// UTF (UTFCodec, kanzi transform id 17) on gfx950, forward and inverse: every block of a batch in the same launches, many workgroups
// per block.
//
// Reference being replaced: transform/UTFCodec.cpp:48-204 (forward), :206-298 (inverse), :303-422 (validate), UTFCodec.hpp:26-37 (the
// alias order: frequency descending, then value descending), :71-154 (pack / unpack).
//
// Forward. The reference walks the block from `start`, one symbol of pack()'s length (1..4 bytes, by the lead byte's top nibble alone)
// after the other while the position is below count - 4. That walk does not resynchronise: what is a symbol start depends on every byte
// in front of it. It is a transducer with five states -- "k bytes still to skip", k = 0..3, and "failed" (a lead in 0x80..0xBF where a
// symbol should start) -- so a stretch of bytes is a map from entry state to exit state (15 bits), and maps compose associatively. A
// thread walks its 16 bytes from the four entries, a workgroup scans the 256 maps of its chunk of 4,096 bytes, one workgroup per block
// scans the chunk maps from state 0: every stretch then knows its entry state exactly, and the state behind the last byte is the overrun
// of header byte 1 (or the failure). The later passes re-walk each stretch from its known entry.
//   distinct symbols   a presence bitmap of the 2^22 packed values (512 KiB per block) and the running popcount of its words: the rank of
//                      a value among the present ones is its index into the frequency table (fewer than 32,768 entries, else refused)
//   alias order        keys (frequency << 22 | value) of every block, 32,768 slots each, through the segmented radix sort of prims.hpp;
//                      read from the top they are the reference's order
//   output             alias sizes (1 or 2 bytes) summed per stretch, scanned inside the chunk and over the chunks; the aliases are
//                      written only when the block's final length passes the last check (dstIdx < count - count / 10 <= cap)
// Every refusal of the parse path refuses the whole block, so the order in which the passes find them does not matter. The data type
// becomes UTF8 once validation has passed or been skipped and stays so whatever happens later.
//
// Inverse. The alias stream does not resynchronise either (a first byte >= 128 takes the next byte whatever it is): two states, the
// same scan. Output offsets are the prefix sums of the symbol lengths; an alias >= n or an output beyond the capacity refuses the block
// wherever it occurs, so both are decided from the totals before a byte is written, and nothing is written behind the capacity.
#include "common.hpp"
#include "stages.hpp"
#include "datatype.hpp"
#include "prims.hpp"

namespace knz {

namespace {

constexpr int UT_T = 256;                         // threads per workgroup
constexpr u32 UT_SEG = 16;                        // bytes per thread
constexpr u32 UT_CHUNK = UT_T * UT_SEG;           // bytes per workgroup
constexpr u32 UT_MIN = 1024;                      // UTFCodec::MIN_BLOCK_SIZE
constexpr u32 UT_MAXSYM = 32768;                  // distinct symbols: fewer than this
constexpr u32 UT_BMW = (1u << 22) / 32;           // words of the presence bitmap
constexpr u32 UT_VALMASK = (1u << 22) - 1;

// per-block scratch (u32 words)
constexpr u32 UT_INFO = 0;                        // [64] UtInfo
constexpr u32 UT_BITS = 64;                       // [UT_BMW] presence bitmap
constexpr u32 UT_FREQ = UT_BITS + UT_BMW;         // [32768] forward: frequency by rank of value; inverse: the symbols' bytes
constexpr u32 UT_ALIAS = UT_FREQ + UT_MAXSYM;     // [16384] forward: u16 alias by rank of value; inverse: u8 symbol lengths
constexpr u32 UT_RANK = UT_ALIAS + UT_MAXSYM / 2; // [UT_BMW] present values below the word
constexpr u32 UT_CH = UT_RANK + UT_BMW;           // [2 per chunk] (map, then entry state), (size sum, then offset); then one word per stretch

struct UtInfo {
    u32 active;     // the block is still being transformed
    u32 start;      // forward: raw bytes in front of the first symbol; inverse: the same, from the header
    u32 validate;
    u32 bad;        // validation: a forbidden byte or pair was seen
    u32 cont;       // validation: bytes in 0x80..0xBF
    u32 end;        // forward: overrun of the last symbol (0..3); inverse: state behind the alias stream (1: the last alias took src[srcEnd])
    u32 fail;       // a later symbol check failed / an alias >= n
    u32 n;          // distinct symbols
    u32 ok;
    u32 total;      // bytes of all aliases (forward) / of all symbols (inverse)
    u32 a0;         // inverse: first byte of the alias stream
    u32 srcEnd;     // inverse
    u32 adjust;     // inverse
};
static_assert(sizeof(UtInfo) <= 64 * 4, "UtInfo too large");

__host__ __device__ inline size_t ut_chunks(u32 maxLen) { return (size_t)maxLen / UT_CHUNK + 2; }
__host__ __device__ inline size_t ut_stride_u32(u32 maxLen) { return (UT_CH + (2 + (size_t)UT_T) * ut_chunks(maxLen) + 63) & ~(size_t)63; }
__device__ __forceinline__ u32* ut_chw(u32* ws) { return ws + UT_CH; }
__device__ __forceinline__ u16* ut_stx(u32* ws, u32 maxLen) { return reinterpret_cast<u16*>(ws + UT_CH + 2 * ut_chunks(maxLen)); }            // [stretch] map in front of it
__device__ __forceinline__ u16* ut_sto(u32* ws, u32 maxLen) { return ut_stx(ws, maxLen) + (size_t)UT_T * ut_chunks(maxLen); }                 // [stretch] bytes in front of it

// state maps: 3 bits per entry state
constexpr u32 UT_ID = 0u | (1u << 3) | (2u << 6) | (3u << 9) | (4u << 12);
constexpr u32 UT_FAILED = 4;
__device__ __forceinline__ u32 ut_at(u32 f, u32 e) { return (f >> (3 * e)) & 7u; }
__device__ __forceinline__ u32 ut_then(u32 f, u32 g)          // f, then g
{
    u32 r = 0;
#pragma unroll
    for (u32 e = 0; e < 5; e++) r |= ut_at(g, ut_at(f, e)) << (3 * e);
    return r;
}

// inclusive scan of one map per thread over UT_T threads (Hillis-Steele in LDS)
__device__ u32 ut_wg_scan(u32 v, u32* sh)
{
    const int t = (int)threadIdx.x;
    sh[t] = v;
    __syncthreads();
    for (int o = 1; o < UT_T; o <<= 1) {
        const u32 prev = (t >= o) ? sh[t - o] : UT_ID;
        __syncthreads();
        if (t >= o) v = ut_then(prev, v);
        sh[t] = v;
        __syncthreads();
    }
    return v;
}

// pack()'s length by the lead byte's top nibble: 0..7 -> 1, 8..11 -> 0, 12 / 13 -> 2, 14 -> 3, 15 -> 4
__device__ __forceinline__ u32 ut_len(u32 c) { return (u32)(0x4322000011111111ull >> (4 * (c >> 4))) & 7u; }

__device__ __forceinline__ u32 ut_pack(const u8* src, u32 p, u32 s)
{
    const u32 c0 = ldg<u8>(src + p);
    if (s == 1) return c0;
    const u32 c1 = ldg<u8>(src + p + 1);
    if (s == 2) return (1u << 19) | (c0 << 8) | c1;
    const u32 c2 = ldg<u8>(src + p + 2);
    if (s == 3) return (2u << 19) | ((c0 & 0x0F) << 12) | ((c1 & 0x3F) << 6) | (c2 & 0x3F);
    const u32 c3 = ldg<u8>(src + p + 3);
    return (4u << 19) | ((c0 & 0x07) << 18) | ((c1 & 0x3F) << 12) | ((c2 & 0x3F) << 6) | (c3 & 0x3F);
}

// the map of the symbol walk over [a, b)
__device__ __forceinline__ u32 ut_walk_fn(const u8* src, u32 a, u32 b)
{
    u32 f = UT_FAILED << 12;
#pragma unroll
    for (u32 e = 0; e < 4; e++) {
        u32 p = a + e;
        bool failed = false;
        while (p < b) {
            const u32 s = ut_len(ldg<u8>(src + p));
            if (s == 0) { failed = true; break; }
            p += s;
        }
        f |= (failed ? UT_FAILED : p - b) << (3 * e);
    }
    return f;
}

// validate()'s predicates (UTFCodec.cpp:356-415) on one byte and on one (lead, next) pair
__device__ __forceinline__ bool ut_bad_byte(u32 c) { return c == 0xC0 || c == 0xC1 || c >= 0xF5; }
__device__ __forceinline__ bool ut_bad_pair(u32 lead, u32 nx)
{
    if (lead < 0xC2 || lead > 0xF4) return false;
    if (lead == 0xE0) return nx < 0xA0 || nx > 0xBF;
    if (lead == 0xED) return nx < 0x80 || nx > 0x9F;
    if (lead == 0xF0) return nx < 0x90 || nx > 0xBF;
    if (lead == 0xF4) return nx < 0x80 || nx > 0x8F;
    return nx < 0x80 || nx > 0xBF;
}

// rank of a present value among the present values
__device__ __forceinline__ u32 ut_rank(const u32* ws, u32 val)
{
    const u32 w = val >> 5;
    return ws[UT_RANK + w] + (u32)__popc(ws[UT_BITS + w] & ((1u << (val & 31)) - 1u));
}

// the part [a, b) of the symbol walk that belongs to this thread, and its entry state
struct UtSpan { u32 a, b, e; };
__device__ __forceinline__ UtSpan ut_span(u32* ws, u32 maxLen, u32 lo, u32 hi)
{
    UtSpan sp;
    const u32 a0 = blockIdx.x * UT_CHUNK + threadIdx.x * UT_SEG;
    sp.a = a0 < lo ? lo : (a0 < hi ? a0 : hi);
    sp.b = a0 + UT_SEG < hi ? a0 + UT_SEG : hi;
    if (sp.b < sp.a) sp.b = sp.a;
    sp.e = ut_at(ut_stx(ws, maxLen)[(size_t)blockIdx.x * UT_T + threadIdx.x], ut_chw(ws)[2 * blockIdx.x]);
    return sp;
}

// ---------------------------------------------------------------------------------------------------------------------
// forward
// ---------------------------------------------------------------------------------------------------------------------

// the first bytes whose LEN_SEQ is 0 (UTFCodec.cpp:28-46: 0x80..0xC1 and 0xF5..0xFF)
__device__ __forceinline__ bool ut_len_seq0(u32 c) { return (c >= 0x80 && c < 0xC2) || c >= 0xF5; }

// guards and the start offset (UTFCodec.cpp:50-88); clears the bitmap and the frequencies
__global__ __launch_bounds__(UT_T) void k_utf_f_init(XfStage st, u32* scratch, size_t stride)
{
    const int b = blockIdx.y;
    const u32 count = st.len[b];
    if (count == 0) return;
    u32* ws = scratch + (size_t)b * stride;
    uint4* z = reinterpret_cast<uint4*>(ws + UT_BITS);
    for (u32 i = blockIdx.x * UT_T + threadIdx.x; i < (UT_BMW + UT_MAXSYM) / 4; i += gridDim.x * UT_T) z[i] = make_uint4(0u, 0u, 0u, 0u);
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    UtInfo* info = reinterpret_cast<UtInfo*>(ws + UT_INFO);
    UtInfo v = {};
    const int dt = st.dtype ? (int)st.dtype[b] : (int)DT_UNDEFINED;
    v.active = (count >= UT_MIN && (u64)st.cap[b] >= (u64)count + 8192 && (dt == DT_UNDEFINED || dt == DT_UTF8)) ? 1u : 0u;
    v.validate = dt != DT_UTF8 ? 1u : 0u;
    if (v.active) {
        const u8* src = st.src[b];
        if (ldg<u8>(src) == 0xEF && ldg<u8>(src + 1) == 0xBB && ldg<u8>(src + 2) == 0xBF) v.start = 3;
        else while (v.start < 4 && ut_len_seq0(ldg<u8>(src + v.start))) v.start++;
    }
    *info = v;
    st.ok[b] = 0;
    st.newLen[b] = 0;
}

// validation counters and the map of every chunk of [start, count - 4)
__global__ __launch_bounds__(UT_T) void k_utf_f_scan(XfStage st, u32* scratch, size_t stride)
{
    const int b = blockIdx.y;
    const u32 count = st.len[b];
    if (count == 0) return;
    u32* ws = scratch + (size_t)b * stride;
    UtInfo* info = reinterpret_cast<UtInfo*>(ws + UT_INFO);
    if (!info->active) return;
    const u32 lo = info->start, hi = count - 4;
    if (blockIdx.x * UT_CHUNK >= hi) return;
    __shared__ u32 sh[UT_T];
    const u8* __restrict__ src = st.src[b];
    const u32 a0 = blockIdx.x * UT_CHUNK + threadIdx.x * UT_SEG;
    const u32 a = a0 < lo ? lo : (a0 < hi ? a0 : hi);
    u32 e = a0 + UT_SEG < hi ? a0 + UT_SEG : hi;
    if (e < a) e = a;
    if (info->validate) {
        u32 cont = 0;
        bool bad = false;
        u32 prv = a > lo ? ldg<u8>(src + a - 1) : 0u;
        for (u32 p = a; p < e; p++) {
            const u32 c = ldg<u8>(src + p);
            bad = bad || ut_bad_byte(c) || ut_bad_pair(prv, c);
            cont += (c & 0xC0) == 0x80 ? 1u : 0u;
            prv = c;
        }
        const u32 wc = wave_sum(cont);
        if (lane_id() == 0 && wc) atomicAdd(&info->cont, wc);
        if (bad) atomicOr(&info->bad, 1u);
    }
    const u32 f = ut_walk_fn(src, a, e);
    const u32 incl = ut_wg_scan(f, sh);
    ut_stx(ws, st.maxLen)[(size_t)blockIdx.x * UT_T + threadIdx.x] = (u16)(threadIdx.x ? sh[threadIdx.x - 1] : UT_ID);
    if (threadIdx.x == UT_T - 1) ut_chw(ws)[2 * blockIdx.x] = incl;
}

// one workgroup per block: validate()'s verdict, the data type, every chunk's entry state, the state behind the last symbol
__global__ __launch_bounds__(UT_T) void k_utf_f_chunks(XfStage st, u32* scratch, size_t stride)
{
    const int b = blockIdx.x;
    const u32 count = st.len[b];
    if (count == 0) return;
    u32* ws = scratch + (size_t)b * stride;
    UtInfo* info = reinterpret_cast<UtInfo*>(ws + UT_INFO);
    const u32 m = count - info->start - 4;
    const bool go = info->active && !(info->validate && (info->bad || info->cont < m / 8));
    __syncthreads();
    if (!go) { if (threadIdx.x == 0) info->active = 0; return; }
    if (threadIdx.x == 0 && st.dtype) st.dtype[b] = (u8)DT_UTF8;
    const u32 hi = count - 4;
    const u32 nCh = (hi + UT_CHUNK - 1) / UT_CHUNK;
    __shared__ u32 sh[UT_T];
    u32* ch = ut_chw(ws);
    u32 state = 0;
    for (u32 base = 0; base < nCh; base += UT_T) {
        const u32 j = base + threadIdx.x;
        ut_wg_scan(j < nCh ? ch[2 * j] : UT_ID, sh);
        if (j < nCh) ch[2 * j] = ut_at(threadIdx.x ? sh[threadIdx.x - 1] : UT_ID, state);
        const u32 all = sh[UT_T - 1];
        __syncthreads();
        state = ut_at(all, state);
    }
    if (threadIdx.x == 0) {
        info->end = state;
        if (state == UT_FAILED) info->active = 0;
    }
}

// the symbols' later checks (third byte, third and fourth byte) and their presence bits
__global__ __launch_bounds__(UT_T) void k_utf_f_mark(XfStage st, u32* scratch, size_t stride)
{
    const int b = blockIdx.y;
    const u32 count = st.len[b];
    if (count == 0) return;
    u32* ws = scratch + (size_t)b * stride;
    UtInfo* info = reinterpret_cast<UtInfo*>(ws + UT_INFO);
    if (!info->active) return;
    const u32 hi = count - 4;
    if (blockIdx.x * UT_CHUNK >= hi) return;
    const u8* __restrict__ src = st.src[b];
    const UtSpan sp = ut_span(ws, st.maxLen, info->start, hi);
    bool bad = false;
    for (u32 p = sp.a + sp.e; p < sp.b;) {
        const u32 s = ut_len(ldg<u8>(src + p));
        if (s == 0) break;                                    // (cannot happen in a block that is still active)
        if (s >= 3) bad = bad || (ldg<u8>(src + p + 2) & 0xC0) != 0x80;
        if (s == 4) bad = bad || (ldg<u8>(src + p + 3) & 0xC0) != 0x80;
        const u32 val = ut_pack(src, p, s);
        const u32 bit = 1u << (val & 31);
        u32* w = ws + UT_BITS + (val >> 5);
        if (!(*w & bit)) atomicOr(w, bit);
        p += s;
    }
    if (bad) atomicOr(&info->fail, 1u);
}

// one workgroup per block: the running popcount of the bitmap's words, the number of distinct symbols and what it refuses
__global__ __launch_bounds__(UT_T) void k_utf_f_rank(XfStage st, u32* scratch, size_t stride)
{
    const int b = blockIdx.x;
    const u32 count = st.len[b];
    if (count == 0) return;
    u32* ws = scratch + (size_t)b * stride;
    UtInfo* info = reinterpret_cast<UtInfo*>(ws + UT_INFO);
    const bool go = info->active && !info->fail;
    __syncthreads();
    if (!go) { if (threadIdx.x == 0) info->active = 0; return; }
    __shared__ u32 wsum[4];
    __shared__ u32 inclAll[UT_T];
    constexpr u32 PER = UT_BMW / UT_T;
    const u32* bits = ws + UT_BITS + threadIdx.x * PER;
    u32 acc = 0;
    for (u32 k = 0; k < PER; k++) acc += (u32)__popc(bits[k]);
    u32 tot;
    inclAll[threadIdx.x] = prims::sc_block_incl<prims::SCAN_SUM_EXCL>(acc, wsum, &tot);
    __syncthreads();
    u32 run = threadIdx.x ? inclAll[threadIdx.x - 1] : 0u;
    u32* rank = ws + UT_RANK + threadIdx.x * PER;
    for (u32 k = 0; k < PER; k++) { rank[k] = run; run += (u32)__popc(bits[k]); }
    if (threadIdx.x == 0) {
        const u32 n = tot, maxTarget = count - count / 10;
        info->n = n;
        if (n == 0 || n >= UT_MAXSYM || 3 * n + 6 >= maxTarget) info->active = 0;
    }
}

// frequencies by rank (the one-byte symbols of a workgroup through LDS)
__global__ __launch_bounds__(UT_T) void k_utf_f_hist(XfStage st, u32* scratch, size_t stride)
{
    const int b = blockIdx.y;
    const u32 count = st.len[b];
    if (count == 0) return;
    u32* ws = scratch + (size_t)b * stride;
    UtInfo* info = reinterpret_cast<UtInfo*>(ws + UT_INFO);
    if (!info->active) return;
    const u32 hi = count - 4;
    if (blockIdx.x * UT_CHUNK >= hi) return;
    __shared__ u32 h1[128];
    if (threadIdx.x < 128) h1[threadIdx.x] = 0;
    __syncthreads();
    const u8* __restrict__ src = st.src[b];
    const UtSpan sp = ut_span(ws, st.maxLen, info->start, hi);
    for (u32 p = sp.a + sp.e; p < sp.b;) {
        const u32 s = ut_len(ldg<u8>(src + p));
        if (s == 0) break;
        const u32 val = ut_pack(src, p, s);
        if (s == 1) atomicAdd(&h1[val], 1u);
        else atomicAdd(ws + UT_FREQ + ut_rank(ws, val), 1u);
        p += s;
    }
    __syncthreads();
    if (threadIdx.x < 128 && h1[threadIdx.x]) atomicAdd(ws + UT_FREQ + ut_rank(ws, threadIdx.x), h1[threadIdx.x]);
}

// sort keys of the present values: frequency << 22 | value; the slots behind the n-th stay zero (cleared by the launcher)
__global__ __launch_bounds__(UT_T) void k_utf_f_keys(XfStage st, u32* scratch, size_t stride, u64* __restrict__ keys)
{
    const int b = blockIdx.y;
    const u32* ws = scratch + (size_t)b * stride;
    if (st.len[b] == 0 || !reinterpret_cast<const UtInfo*>(ws + UT_INFO)->active) return;
    u64* k = keys + (size_t)b * UT_MAXSYM;
    constexpr u32 PER = UT_BMW / 32;                              // words per workgroup (gridDim.x == 32)
    for (u32 i = threadIdx.x; i < PER; i += UT_T) {
        const u32 w = blockIdx.x * PER + i;
        u32 bits = ws[UT_BITS + w];
        u32 idx = ws[UT_RANK + w];
        while (bits) {
            const u32 j = (u32)__ffs((int)bits) - 1u;
            bits &= bits - 1u;
            k[idx] = ((u64)ws[UT_FREQ + idx] << 22) | (u64)(w * 32u + j);
            idx++;
        }
    }
}

// one workgroup per block: the map in the reference's order, the alias of every value, the size estimate and what it refuses
__global__ __launch_bounds__(UT_T) void k_utf_f_map(XfStage st, u32* scratch, size_t stride, const u64* __restrict__ keys)
{
    const int b = blockIdx.x;
    const u32 count = st.len[b];
    if (count == 0) return;
    u32* ws = scratch + (size_t)b * stride;
    UtInfo* info = reinterpret_cast<UtInfo*>(ws + UT_INFO);
    if (!info->active) return;
    __shared__ u32 wsum[4];
    const u64* k = keys + (size_t)b * UT_MAXSYM;
    u16* alias = reinterpret_cast<u16*>(ws + UT_ALIAS);
    u8* dst = st.dst[b];
    const u32 n = info->n;
    u32 est = 0;
    for (u32 i = threadIdx.x; i < n; i += UT_T) {
        const u64 key = k[UT_MAXSYM - 1 - i];
        const u32 val = (u32)key & UT_VALMASK, fr = (u32)(key >> 22);
        est += i < 128 ? fr : 2 * fr;
        alias[ut_rank(ws, val)] = (u16)i;
        dst[4 + 3 * i] = (u8)(val >> 16); dst[5 + 3 * i] = (u8)(val >> 8); dst[6 + 3 * i] = (u8)val;
    }
    u32 tot;
    prims::sc_block_incl<prims::SCAN_SUM_EXCL>(est, wsum, &tot);
    if (threadIdx.x == 0 && 10 + tot >= count - count / 10) info->active = 0;
}

// bytes of the aliases of every stretch, in front of it inside its chunk, and of every chunk
__global__ __launch_bounds__(UT_T) void k_utf_f_sizes(XfStage st, u32* scratch, size_t stride)
{
    const int b = blockIdx.y;
    const u32 count = st.len[b];
    if (count == 0) return;
    u32* ws = scratch + (size_t)b * stride;
    UtInfo* info = reinterpret_cast<UtInfo*>(ws + UT_INFO);
    if (!info->active) return;
    const u32 hi = count - 4;
    if (blockIdx.x * UT_CHUNK >= hi) return;
    __shared__ u32 wsum[4];
    const u8* __restrict__ src = st.src[b];
    const u16* alias = reinterpret_cast<const u16*>(ws + UT_ALIAS);
    const UtSpan sp = ut_span(ws, st.maxLen, info->start, hi);
    u32 bytes = 0;
    for (u32 p = sp.a + sp.e; p < sp.b;) {
        const u32 s = ut_len(ldg<u8>(src + p));
        if (s == 0) break;
        bytes += alias[ut_rank(ws, ut_pack(src, p, s))] < 128 ? 1u : 2u;
        p += s;
    }
    u32 tot;
    const u32 incl = prims::sc_block_incl<prims::SCAN_SUM_EXCL>(bytes, wsum, &tot);
    ut_sto(ws, st.maxLen)[(size_t)blockIdx.x * UT_T + threadIdx.x] = (u16)(incl - bytes);
    if (threadIdx.x == 0) ut_chw(ws)[2 * blockIdx.x + 1] = tot;
}

// one workgroup per block: every chunk's offset, the final length and its check, the header, the raw bytes at both ends
__global__ __launch_bounds__(UT_T) void k_utf_f_offsets(XfStage st, u32* scratch, size_t stride)
{
    const int b = blockIdx.x;
    const u32 count = st.len[b];
    if (count == 0) return;
    u32* ws = scratch + (size_t)b * stride;
    UtInfo* info = reinterpret_cast<UtInfo*>(ws + UT_INFO);
    if (!info->active) return;
    const u32 hi = count - 4;
    const u32 nCh = (hi + UT_CHUNK - 1) / UT_CHUNK;
    __shared__ u32 wsum[4];
    u32* ch = ut_chw(ws);
    u32 run = 0;
    for (u32 base = 0; base < nCh; base += UT_T) {
        const u32 j = base + threadIdx.x;
        const u32 v = j < nCh ? ch[2 * j + 1] : 0u;
        u32 tot;
        const u32 incl = prims::sc_block_incl<prims::SCAN_SUM_EXCL>(v, wsum, &tot);
        if (j < nCh) ch[2 * j + 1] = run + incl - v;
        run += tot;
    }
    if (threadIdx.x == 0) {
        const u32 n = info->n, start = info->start, over = info->end;
        const u64 total = 4ull + 3ull * n + start + run + (4u - over);
        const u32 ok = total < (u64)(count - count / 10) ? 1u : 0u;
        info->total = run;
        info->ok = ok;
        if (ok) {
            const u8* src = st.src[b];
            u8* dst = st.dst[b];
            dst[0] = (u8)start; dst[1] = (u8)over; dst[2] = (u8)(n >> 8); dst[3] = (u8)n;
            for (u32 i = 0; i < start; i++) dst[4 + 3 * n + i] = ldg<u8>(src + i);
            for (u32 i = 0; i < 4u - over; i++) dst[4 + 3 * n + start + run + i] = ldg<u8>(src + hi + over + i);
        }
        st.ok[b] = (u8)ok;
        st.newLen[b] = ok ? (u32)total : 0u;
    }
}

__global__ __launch_bounds__(UT_T) void k_utf_f_emit(XfStage st, u32* scratch, size_t stride)
{
    const int b = blockIdx.y;
    const u32 count = st.len[b];
    if (count == 0) return;
    u32* ws = scratch + (size_t)b * stride;
    const UtInfo* info = reinterpret_cast<const UtInfo*>(ws + UT_INFO);
    if (!info->active || !info->ok) return;
    const u32 hi = count - 4;
    if (blockIdx.x * UT_CHUNK >= hi) return;
    const u8* __restrict__ src = st.src[b];
    u8* __restrict__ dst = st.dst[b];
    const u16* alias = reinterpret_cast<const u16*>(ws + UT_ALIAS);
    const UtSpan sp = ut_span(ws, st.maxLen, info->start, hi);
    u32 o = 4 + 3 * info->n + info->start + ut_chw(ws)[2 * blockIdx.x + 1] + ut_sto(ws, st.maxLen)[(size_t)blockIdx.x * UT_T + threadIdx.x];
    for (u32 p = sp.a + sp.e; p < sp.b;) {
        const u32 s = ut_len(ldg<u8>(src + p));
        if (s == 0) break;
        const u32 al = alias[ut_rank(ws, ut_pack(src, p, s))];
        if (al < 128) dst[o++] = (u8)al;
        else { dst[o] = (u8)(0x80u | (al & 0x7Fu)); dst[o + 1] = (u8)(al >> 7); o += 2; }
        p += s;
    }
}

static __global__ void k_utf_seg_base(u32* base, int nBlocks)
{
    for (int i = (int)threadIdx.x; i <= nBlocks; i += (int)blockDim.x) base[i] = (u32)i * UT_MAXSYM;
}

// ---------------------------------------------------------------------------------------------------------------------
// inverse
// ---------------------------------------------------------------------------------------------------------------------

// the map of the alias walk over [a, b): two states (0: an alias starts here, 1: this byte is an alias' second one)
__device__ __forceinline__ u32 ut_alias_fn(const u8* src, u32 a, u32 b)
{
    u32 f = (2u << 6) | (3u << 9) | (4u << 12);
#pragma unroll
    for (u32 e = 0; e < 2; e++) {
        u32 p = a + e;
        while (p < b) p += ldg<u8>(src + p) >= 128 ? 2u : 1u;
        f |= (p - b) << (3 * e);
    }
    return f;
}

// header, guards and the symbol table (UTFCodec.cpp:208-265)
__global__ __launch_bounds__(UT_T) void k_utf_i_head(XfStage st, u32* scratch, size_t stride)
{
    const int b = blockIdx.x;
    const u32 count = st.len[b];
    if (count == 0) return;
    u32* ws = scratch + (size_t)b * stride;
    UtInfo* info = reinterpret_cast<UtInfo*>(ws + UT_INFO);
    const u8* __restrict__ src = st.src[b];
    const u32 cap = st.cap[b] > st.capModel ? st.cap[b] : st.capModel;
    __shared__ u32 badSym;
    if (threadIdx.x == 0) { badSym = 0; st.ok[b] = 0; st.newLen[b] = 0; }
    u32 start = 0, adjust = 0, n = 0;
    bool go = count >= 4;
    if (go) {
        start = ldg<u8>(src) & 3u; adjust = ldg<u8>(src + 1) & 3u;
        n = ((u32)ldg<u8>(src + 2) << 8) + ldg<u8>(src + 3);
        go = n != 0 && n < UT_MAXSYM && 3 * n <= count - 4;
    }
    const u32 srcEnd = count - 4 + adjust;
    // (srcEnd <= count - 1; the table ends at 4 + 3 n <= count)
    go = go && cap >= 4 && 4 + 3 * n + start <= srcEnd && start <= cap;
    __syncthreads();
    if (go) {
        u32* sym = ws + UT_FREQ;
        u8* slen = reinterpret_cast<u8*>(ws + UT_ALIAS);
        bool bad = false;
        for (u32 i = threadIdx.x; i < n; i += UT_T) {
            const u32 v = ((u32)ldg<u8>(src + 4 + 3 * i) << 16) | ((u32)ldg<u8>(src + 5 + 3 * i) << 8) | ldg<u8>(src + 6 + 3 * i);
            u32 bytes = 0, l = 0;
            switch (v >> 19) {
            case 0: bytes = v & 0xFF; l = 1; break;
            case 1: bytes = ((v >> 8) & 0xFF) | ((v & 0xFF) << 8); l = 2; break;
            case 2: bytes = (0xE0 | ((v >> 12) & 0x0F)) | ((0x80 | ((v >> 6) & 0x3F)) << 8) | ((0x80 | (v & 0x3F)) << 16); l = 3; break;
            case 4: case 5: case 6: case 7:
                bytes = (0xF0 | ((v >> 18) & 0x07)) | ((0x80 | ((v >> 12) & 0x3F)) << 8) | ((0x80 | ((v >> 6) & 0x3F)) << 16) | ((0x80 | (v & 0x3F)) << 24); l = 4; break;
            default: bad = true; break;
            }
            sym[i] = bytes; slen[i] = (u8)l;
        }
        if (bad) atomicOr(&badSym, 1u);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        UtInfo v = {};
        v.active = go && !badSym ? 1u : 0u;
        v.start = start; v.adjust = adjust; v.n = n; v.srcEnd = srcEnd; v.a0 = 4 + 3 * n + start;
        *info = v;
    }
}

__global__ __launch_bounds__(UT_T) void k_utf_i_scan(XfStage st, u32* scratch, size_t stride)
{
    const int b = blockIdx.y;
    if (st.len[b] == 0) return;
    u32* ws = scratch + (size_t)b * stride;
    const UtInfo* info = reinterpret_cast<const UtInfo*>(ws + UT_INFO);
    if (!info->active) return;
    const u32 lo = info->a0, hi = info->srcEnd;
    if (blockIdx.x * UT_CHUNK >= hi) return;
    __shared__ u32 sh[UT_T];
    const u32 a0 = blockIdx.x * UT_CHUNK + threadIdx.x * UT_SEG;
    const u32 a = a0 < lo ? lo : (a0 < hi ? a0 : hi);
    u32 e = a0 + UT_SEG < hi ? a0 + UT_SEG : hi;
    if (e < a) e = a;
    const u32 incl = ut_wg_scan(ut_alias_fn(st.src[b], a, e), sh);
    ut_stx(ws, st.maxLen)[(size_t)blockIdx.x * UT_T + threadIdx.x] = (u16)(threadIdx.x ? sh[threadIdx.x - 1] : UT_ID);
    if (threadIdx.x == UT_T - 1) ut_chw(ws)[2 * blockIdx.x] = incl;
}

__global__ __launch_bounds__(UT_T) void k_utf_i_chunks(XfStage st, u32* scratch, size_t stride)
{
    const int b = blockIdx.x;
    if (st.len[b] == 0) return;
    u32* ws = scratch + (size_t)b * stride;
    UtInfo* info = reinterpret_cast<UtInfo*>(ws + UT_INFO);
    if (!info->active) return;
    const u32 nCh = (info->srcEnd + UT_CHUNK - 1) / UT_CHUNK;
    __shared__ u32 sh[UT_T];
    u32* ch = ut_chw(ws);
    u32 state = 0;
    for (u32 base = 0; base < nCh; base += UT_T) {
        const u32 j = base + threadIdx.x;
        ut_wg_scan(j < nCh ? ch[2 * j] : UT_ID, sh);
        if (j < nCh) ch[2 * j] = ut_at(threadIdx.x ? sh[threadIdx.x - 1] : UT_ID, state);
        const u32 all = sh[UT_T - 1];
        __syncthreads();
        state = ut_at(all, state);
    }
    if (threadIdx.x == 0) info->end = state;
}

// the alias at p (its first byte; a first byte >= 128 takes the next byte whatever it is); *step = its bytes
__device__ __forceinline__ u32 ut_alias_at(const u8* src, u32 p, u32* step)
{
    u32 al = ldg<u8>(src + p);
    *step = 1;
    if (al >= 128) { al = ((u32)ldg<u8>(src + p + 1) << 7) + (al & 0x7Fu); *step = 2; }
    return al;
}

__global__ __launch_bounds__(UT_T) void k_utf_i_sizes(XfStage st, u32* scratch, size_t stride)
{
    const int b = blockIdx.y;
    if (st.len[b] == 0) return;
    u32* ws = scratch + (size_t)b * stride;
    UtInfo* info = reinterpret_cast<UtInfo*>(ws + UT_INFO);
    if (!info->active) return;
    const u32 hi = info->srcEnd;
    if (blockIdx.x * UT_CHUNK >= hi) return;
    __shared__ u32 wsum[4];
    const u8* __restrict__ src = st.src[b];
    const u8* slen = reinterpret_cast<const u8*>(ws + UT_ALIAS);
    const UtSpan sp = ut_span(ws, st.maxLen, info->a0, hi);
    const u32 n = info->n;
    u32 bytes = 0;
    bool bad = false;
    for (u32 p = sp.a + sp.e; p < sp.b;) {
        u32 step;
        const u32 al = ut_alias_at(src, p, &step);
        if (al >= n) bad = true; else bytes += slen[al];
        p += step;
    }
    if (bad) atomicOr(&info->fail, 1u);
    u32 tot;
    const u32 incl = prims::sc_block_incl<prims::SCAN_SUM_EXCL>(bytes, wsum, &tot);
    ut_sto(ws, st.maxLen)[(size_t)blockIdx.x * UT_T + threadIdx.x] = (u16)(incl - bytes);
    if (threadIdx.x == 0) ut_chw(ws)[2 * blockIdx.x + 1] = tot;
}

// one workgroup per block: every chunk's offset and the verdict (UTFCodec.cpp:271-297); the raw bytes at both ends
__global__ __launch_bounds__(UT_T) void k_utf_i_offsets(XfStage st, u32* scratch, size_t stride)
{
    const int b = blockIdx.x;
    const u32 count = st.len[b];
    if (count == 0) return;
    u32* ws = scratch + (size_t)b * stride;
    UtInfo* info = reinterpret_cast<UtInfo*>(ws + UT_INFO);
    if (!info->active) return;
    const u32 nCh = (info->srcEnd + UT_CHUNK - 1) / UT_CHUNK;
    __shared__ u32 wsum[4];
    u32* ch = ut_chw(ws);
    u64 run = 0;
    for (u32 base = 0; base < nCh; base += UT_T) {
        const u32 j = base + threadIdx.x;
        const u32 v = j < nCh ? ch[2 * j + 1] : 0u;
        u32 tot;
        const u32 incl = prims::sc_block_incl<prims::SCAN_SUM_EXCL>(v, wsum, &tot);
        if (j < nCh) ch[2 * j + 1] = (u32)run + incl - v;
        run += tot;
    }
    if (threadIdx.x == 0) {
        // (the verdict by the capacity the reference's buffer has; a block that passes it and does not fit the destination is refused too:
        // it is larger than a block may be)
        const u32 room = st.cap[b], cap = room > st.capModel ? room : st.capModel;
        const u32 start = info->start, adjust = info->adjust;
        const u64 dstIdx = start + run;
        u32 ok = (!info->fail && dstIdx <= cap) ? 1u : 0u;
        u32 tail = 0;
        if (ok) {
            if (info->end == 0) {                              // the alias loop ended exactly at srcEnd
                if (dstIdx < (u64)cap - 4 + adjust) tail = 4 - adjust; else ok = 0;
            } else ok = info->srcEnd + 1 == count ? 1u : 0u;  // the last alias took the byte at srcEnd: no tail is copied
        }
        if (ok && dstIdx + tail > room) ok = 0;
        info->ok = ok;
        if (ok) {
            const u8* src = st.src[b];
            u8* dst = st.dst[b];
            for (u32 i = 0; i < start; i++) dst[i] = ldg<u8>(src + 4 + 3 * info->n + i);
            for (u32 i = 0; i < tail; i++) dst[dstIdx + i] = ldg<u8>(src + info->srcEnd + i);
        }
        st.ok[b] = (u8)ok;
        st.newLen[b] = ok ? (u32)(dstIdx + tail) : 0u;
    }
}

__global__ __launch_bounds__(UT_T) void k_utf_i_emit(XfStage st, u32* scratch, size_t stride)
{
    const int b = blockIdx.y;
    if (st.len[b] == 0) return;
    u32* ws = scratch + (size_t)b * stride;
    const UtInfo* info = reinterpret_cast<const UtInfo*>(ws + UT_INFO);
    if (!info->active || !info->ok) return;
    const u32 hi = info->srcEnd;
    if (blockIdx.x * UT_CHUNK >= hi) return;
    const u8* __restrict__ src = st.src[b];
    u8* __restrict__ dst = st.dst[b];
    const u32* sym = ws + UT_FREQ;
    const u8* slen = reinterpret_cast<const u8*>(ws + UT_ALIAS);
    const UtSpan sp = ut_span(ws, st.maxLen, info->a0, hi);
    u32 o = info->start + ut_chw(ws)[2 * blockIdx.x + 1] + ut_sto(ws, st.maxLen)[(size_t)blockIdx.x * UT_T + threadIdx.x];
    for (u32 p = sp.a + sp.e; p < sp.b;) {
        u32 step;
        const u32 al = ut_alias_at(src, p, &step);
        const u32 l = slen[al];
        u32 v = sym[al];
        for (u32 k = 0; k < l; k++) { dst[o + k] = (u8)v; v >>= 8; }
        o += l;
        p += step;
    }
}

// the part of the scratch all blocks share: segment bases, the sort's workspace, two key arrays
struct UtShared { u32* base; void* rsMem; u64* ka; u64* kb; u32* blocks; };
inline size_t ut_align(size_t x) { return (x + 255) & ~(size_t)255; }
inline size_t ut_shared_bytes(int nBlocks)
{
    return ut_align(4ull * ((size_t)nBlocks + 1)) + ut_align(prims::rs_ws_bytes((size_t)nBlocks * UT_MAXSYM, nBlocks + 1)) + 2 * ut_align(8ull * (size_t)nBlocks * UT_MAXSYM);
}
inline UtShared ut_carve(void* scratch, int nBlocks)
{
    u8* p = reinterpret_cast<u8*>(scratch);
    UtShared w;
    w.base = reinterpret_cast<u32*>(p); p += ut_align(4ull * ((size_t)nBlocks + 1));
    w.rsMem = p; p += ut_align(prims::rs_ws_bytes((size_t)nBlocks * UT_MAXSYM, nBlocks + 1));
    w.ka = reinterpret_cast<u64*>(p); p += ut_align(8ull * (size_t)nBlocks * UT_MAXSYM);
    w.kb = reinterpret_cast<u64*>(p); p += ut_align(8ull * (size_t)nBlocks * UT_MAXSYM);
    w.blocks = reinterpret_cast<u32*>(p);
    return w;
}

int ut_bits(u32 v) { int n = 0; while (v) { n++; v >>= 1; } return n; }

}  // namespace

// Per block: 64 words of bookkeeping, the presence bitmap and its running popcounts (512 KiB each), 32,768 frequencies (128 KiB) and
// aliases (64 KiB), two sort keys of 8 bytes per slot (512 KiB) and the block's share of the sort's workspace (a few KiB) -- about
// 1.8 MiB whatever the length -- plus 8 bytes per chunk of 4,096 bytes and 4 bytes per stretch of 16: len / 4 + len / 512 bytes.
// The inverse uses the same layout (symbol bytes and lengths where the frequencies and aliases are).
size_t utf_scratch_bytes(int nBlocks, u32 maxLen)
{
    return ut_shared_bytes(nBlocks) + (size_t)nBlocks * ut_stride_u32(maxLen) * 4 + 256;
}

#define UT_LAUNCH(k, grid, ...) do { KScope ks_(#k); hipLaunchKernelGGL(k, grid, dim3(UT_T), 0, s, __VA_ARGS__); } while (0)

void launch_utf_forward(hipStream_t s, const XfStage& st, void* scratch)
{
    if (st.nBlocks <= 0) return;
    const UtShared w = ut_carve(scratch, st.nBlocks);
    const size_t stride = ut_stride_u32(st.maxLen);
    const dim3 grid((st.maxLen + UT_CHUNK - 1) / UT_CHUNK, (unsigned)st.nBlocks), one((unsigned)st.nBlocks), g32(32, (unsigned)st.nBlocks);
    UT_LAUNCH(k_utf_f_init, g32, st, w.blocks, stride);
    UT_LAUNCH(k_utf_f_scan, grid, st, w.blocks, stride);
    UT_LAUNCH(k_utf_f_chunks, one, st, w.blocks, stride);
    UT_LAUNCH(k_utf_f_mark, grid, st, w.blocks, stride);
    UT_LAUNCH(k_utf_f_rank, one, st, w.blocks, stride);
    UT_LAUNCH(k_utf_f_hist, grid, st, w.blocks, stride);
    (void)hipMemsetAsync(w.ka, 0, 8ull * (size_t)st.nBlocks * UT_MAXSYM, s);
    UT_LAUNCH(k_utf_f_keys, g32, st, w.blocks, stride, w.ka);
    int r;
    {
        KScope ks_("k_utf_f_sort");
        hipLaunchKernelGGL(k_utf_seg_base, dim3(1), dim3(256), 0, s, w.base, st.nBlocks);
        const prims::RsWs rs = prims::rs_carve(w.rsMem, (size_t)st.nBlocks * UT_MAXSYM, st.nBlocks + 1, w.base, st.nBlocks);
        prims::rs_launch_layout(s, rs);
        // (a frequency is below maxLen: the key has 22 + bits(maxLen) bits)
        r = prims::rs_sort<u64, false>(s, rs, w.ka, w.kb, nullptr, nullptr, UT_MAXSYM, 0, 22 + ut_bits(st.maxLen));
    }
    UT_LAUNCH(k_utf_f_map, one, st, w.blocks, stride, r ? w.kb : w.ka);
    UT_LAUNCH(k_utf_f_sizes, grid, st, w.blocks, stride);
    UT_LAUNCH(k_utf_f_offsets, one, st, w.blocks, stride);
    UT_LAUNCH(k_utf_f_emit, grid, st, w.blocks, stride);
}

void launch_utf_inverse(hipStream_t s, const XfStage& st, void* scratch)
{
    if (st.nBlocks <= 0) return;
    const UtShared w = ut_carve(scratch, st.nBlocks);
    const size_t stride = ut_stride_u32(st.maxLen);
    const dim3 grid((st.maxLen + UT_CHUNK - 1) / UT_CHUNK, (unsigned)st.nBlocks), one((unsigned)st.nBlocks);
    UT_LAUNCH(k_utf_i_head, one, st, w.blocks, stride);
    UT_LAUNCH(k_utf_i_scan, grid, st, w.blocks, stride);
    UT_LAUNCH(k_utf_i_chunks, one, st, w.blocks, stride);
    UT_LAUNCH(k_utf_i_sizes, grid, st, w.blocks, stride);
    UT_LAUNCH(k_utf_i_offsets, one, st, w.blocks, stride);
    UT_LAUNCH(k_utf_i_emit, grid, st, w.blocks, stride);
}

}  // namespace knz
