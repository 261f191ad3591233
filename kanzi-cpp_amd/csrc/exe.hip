// EXE (EXECodec, kanzi transform id 9) on gfx950, forward and inverse: every block of a batch in the same launches.
//
// Reference being replaced: transform/EXECodec.cpp:63-112 (forward), :114-215 and :217-312 (forward x86 / ARM64), :314-518 (inverse),
// :520-625 (detectType), :627-849 (parseHeader) and EXECodec.hpp:96-100 (getMaxEncodedLength).
//
// Every serial loop of the codec is a byte-level (ARM64: word-level) finite-state parse with a lookahead of at most 5 bytes, so a
// stretch of positions is a function from its entry state to its exit state, as in pack.hip. A state function of up to 8 states is one
// u32 (3 bits per entry). A thread walks 16 positions for every entry state, a workgroup composes the 256 functions of its chunk
// (k_ex_fn), one workgroup per block composes the chunk functions (k_ex_scan), a second pass composes the threads' functions again
// (kept from the first), walks each stretch from its known entry and counts (k_ex_count), one workgroup per block sums the counts and
// gives the verdict (k_ex_*_verdict), and a last pass walks again and writes at the known offsets (k_ex_emit). The parses:
//   detection scan  3 states: visit, skip 1, skip 2 (a visited 0F jumps over the next byte, or the next two behind 38 / 3A)
//   forward x86     7 states: at an opcode, behind a 0F, inside the 4 address bytes (4), stopped (boundaryReached: the rest is copied)
//   inverse x86     8 states: the first six, behind an escape, failed
//   forward ARM64   1 state (the words only need a prefix sum of the escape pairs)
//   inverse ARM64   2 states: normal, second word of an escape pair
// The verdict of a block is known before a byte of it is written, and nothing is written for a block that is refused.
#include "common.hpp"
#include "stages.hpp"
#include "datatype.hpp"
#include "magic.hpp"

namespace knz {

namespace {

constexpr int EX_T = 256;                       // threads per workgroup
constexpr int EX_SEG = 16;                      // positions (bytes, or words of the ARM64 parses) per thread
constexpr u32 EX_CHUNK = EX_T * EX_SEG;         // positions per workgroup
constexpr u32 EX_LOOK = 8;                      // bytes staged behind a chunk (the parses look at most 5 bytes ahead)
constexpr u32 EX_SB_WORDS = EX_CHUNK + 4;       // LDS words of a staged chunk of 4-byte positions, its lookahead and 3 bytes of misalignment
constexpr u32 EX_MIN = 4096;                    // EXECodec::MIN_BLOCK_SIZE
constexpr u32 EX_MAX = (1u << 28) - 1;          // EXECodec::MAX_BLOCK_SIZE

enum { EK_NONE = 0, EK_DET, EK_X86F, EK_ARMF, EK_X86I, EK_ARMI };
enum { EA_RAW = 0, EA_ESC = 1, EA_JUMP = 2, EA_SKIP = 3 };    // what a position does (ex_step): plain copy; an escape more (forward) or
                                                              // a byte / word less (inverse); a rewritten address; written by the jump before it
constexpr u32 ES_STOP = 6;                      // forward x86: boundaryReached
constexpr u32 ES_ESC = 6, ES_FAIL = 7;          // inverse x86
constexpr u32 EX_X86 = 0x40, EX_ARM64 = 0x20;   // mode bytes

// per-block scratch (u32 words)
constexpr u32 EX_INFO = 0;                      // [32] ExInfo
constexpr u32 EX_HIST = 32;                     // [256] histogram of the detection scan
constexpr u32 EX_CH = EX_HIST + 256;            // [4 per chunk] state function, then entry state; count 0, then its offset; count 1
                                                // behind them [EX_T per chunk]: every thread's state function, then its entry state

struct ExInfo {
    u32 det;            // EK_DET while the detection scan has to run
    u32 kind;           // EK_* of the code parse (EK_NONE: the block takes no part or is refused)
    u32 lo, hi;         // the parse covers the bytes [lo, hi)
    u32 codeStart, codeEnd;
    u32 count;          // detectType's count
    u32 stop;           // forward x86: srcIdx when the loop ended
    u32 last;           // exit state of the parse
    u32 c0, c1;         // totals of the two counts (detection scan: x86 jumps, ARM64 jumps; code: escapes, rewritten addresses)
    u32 ok;
};
static_assert(sizeof(ExInfo) <= 32 * 4, "ExInfo too large");

__host__ __device__ inline u32 ex_chunks(u32 maxLen) { return maxLen / EX_CHUNK + 1; }
__host__ __device__ inline size_t ex_stride_u32(u32 maxLen) { return (EX_CH + (size_t)(4 + EX_T) * ex_chunks(maxLen) + 63) & ~(size_t)63; }
__device__ __forceinline__ u32* ex_threads(u32* ws, u32 maxLen, u32 chunk) { return ws + EX_CH + 4 * (size_t)ex_chunks(maxLen) + (size_t)chunk * EX_T; }

template <int K> struct ExKind;
template <> struct ExKind<EK_DET>  { static constexpr u32 U = 1, NS = 3; };
template <> struct ExKind<EK_X86F> { static constexpr u32 U = 1, NS = 7; };
template <> struct ExKind<EK_ARMF> { static constexpr u32 U = 4, NS = 1; };
template <> struct ExKind<EK_X86I> { static constexpr u32 U = 1, NS = 8; };
template <> struct ExKind<EK_ARMI> { static constexpr u32 U = 4, NS = 2; };

// state functions: entry e -> exit (f >> 3 e) & 7
constexpr u32 EX_IDENT = 0u | (1u << 3) | (2u << 6) | (3u << 9) | (4u << 12) | (5u << 15) | (6u << 18) | (7u << 21);
__device__ __forceinline__ u32 ex_at(u32 f, u32 e) { return (f >> (3 * e)) & 7u; }
__device__ __forceinline__ u32 ex_then(u32 f, u32 g)        // f, then g
{
    u32 r = 0;
#pragma unroll
    for (u32 e = 0; e < 8; e++) r |= ex_at(g, ex_at(f, e)) << (3 * e);
    return r;
}

// inclusive composition over EX_T threads; every thread's result is left in all[]
__device__ u32 ex_wg_scan(u32 v, u32* sh /* [4] */, u32* all /* [EX_T] */)
{
    const int lane = lane_id(), wave = (int)(threadIdx.x >> 6);
    for (int o = 1; o < 64; o <<= 1) { const u32 t = (u32)__shfl_up((int)v, (unsigned)o, 64); if (lane >= o) v = ex_then(t, v); }
    if (lane == 63) sh[wave] = v;
    __syncthreads();
    u32 carry = EX_IDENT;
    for (int w = 0; w < wave; w++) carry = ex_then(carry, sh[w]);
    v = ex_then(carry, v);
    all[threadIdx.x] = v;
    __syncthreads();
    return v;
}

// inclusive sum over EX_T threads
__device__ u32 ex_wg_sum(u32 v, u32* sh /* [4] */, u32* total)
{
    const int lane = lane_id(), wave = (int)(threadIdx.x >> 6);
    v = wave_incl_scan(v);
    if (lane == 63) sh[wave] = v;
    __syncthreads();
    u32 carry = 0, tot = 0;
    for (int w = 0; w < EX_T / 64; w++) { if (w < wave) carry += sh[w]; tot += sh[w]; }
    __syncthreads();
    *total = tot;
    return carry + v;
}

// The bytes [base, base + bytes) of a block of n bytes in LDS (zero at and behind n), read as aligned words where whole words lie
// inside the block. Returns the address of byte `base`: the copy keeps the misalignment of the source, so words stay words.
__device__ const u8* ex_stage(u32* sw, const u8* __restrict__ src, u32 base, u32 bytes, u32 n)
{
    const u32 mis = (u32)(reinterpret_cast<uintptr_t>(src + base) & 3);
    u8* sb = reinterpret_cast<u8*>(sw) + mis;
    const u32 avail = base < n ? min(bytes, n - base) : 0u;
    const u32 head = min(avail, (4 - mis) & 3);
    const u32 words = (avail - head) >> 2;
    const u32 t = threadIdx.x;
    for (u32 i = t; i < words; i += EX_T) sw[((mis + head) >> 2) + i] = ldg<u32>(src + base + head + 4 * i);
    if (t < head) sb[t] = ldg<u8>(src + base + t);
    for (u32 i = head + 4 * words + t; i < bytes; i += EX_T) sb[i] = i < avail ? ldg<u8>(src + base + i) : (u8)0;
    __syncthreads();
    return sb;
}

__device__ __forceinline__ u32 ex_le32(const u8* q) { return (u32)q[0] | ((u32)q[1] << 8) | ((u32)q[2] << 16) | ((u32)q[3] << 24); }
__device__ __forceinline__ u32 ex_be32(const u8* q) { return (u32)q[3] | ((u32)q[2] << 8) | ((u32)q[1] << 16) | ((u32)q[0] << 24); }
__device__ __forceinline__ bool ex_is_bl(u32 instr) { const u32 op = instr & 0xFC000000u; return op == 0x14000000u || op == 0x94000000u; }

// One position p (q: its bytes, hi: end of the parse) in state s: the next state, and in bits 4-5 what the position does (EA_*).
template <int K> __device__ __forceinline__ u32 ex_step(const u8* q, u32 p, u32 s, u32 hi);

// detection scan (EXECodec.cpp:560-584): a position is visited or jumped over
template <> __device__ __forceinline__ u32 ex_step<EK_DET>(const u8* q, u32 p, u32 s, u32 hi)
{
    if (s) return s - 1;
    const u32 b = q[0];
    if (p + 4 < hi && (b & 0xFE) == 0xE8) return 0;             // the E8 / E9 arm: whatever the sign byte is, the 0F arm is not tried
    if (b == 0x0F && p + 1 < hi) return ((q[1] == 0x38 || q[1] == 0x3A) && p + 2 < hi) ? 2u : 1u;
    return 0;
}

// forward x86 (EXECodec.cpp:137-195)
template <> __device__ __forceinline__ u32 ex_step<EK_X86F>(const u8* q, u32 p, u32 s, u32 hi)
{
    if (s == ES_STOP) return ES_STOP;
    if (s >= 2) return (s == 5 ? 0u : s + 1) | (EA_SKIP << 4);
    const u32 b = q[0];
    if (s == 0) {
        if (b == 0x0F) {
            if (p + 1 >= hi) return ES_STOP;                                     // a lone trailing 0F
            if ((q[1] & 0xF0) == 0x80 && p + 5 >= hi) return ES_STOP;            // 0F 8x with fewer than 5 bytes left
            return 1;
        }
        if ((b & 0xFE) != 0xE8) return b == 0x9B ? (EA_ESC << 4) : 0u;
    } else if ((b & 0xF0) != 0x80) return b == 0x9B ? (EA_ESC << 4) : 0u;
    if (p + 4 >= hi) return ES_STOP;                                             // E8 / E9 with fewer than 4 bytes left
    const u32 sgn = q[4];
    if ((sgn != 0 && sgn != 0xFF) || ex_le32(q + 1) == 0xFF000000u) return EA_ESC << 4;
    return 2u | (EA_JUMP << 4);
}

// inverse x86 (EXECodec.cpp:360-422)
template <> __device__ __forceinline__ u32 ex_step<EK_X86I>(const u8* q, u32 p, u32 s, u32 hi)
{
    if (s == ES_FAIL) return ES_FAIL;
    if (s == ES_ESC) return 0;
    if (s >= 2) return (s == 5 ? 0u : s + 1) | (EA_SKIP << 4);
    const u32 b = q[0];
    if (s == 0) {
        if (b == 0x0F) return p + 1 >= hi ? 0u : 1u;                             // (the legacy trailing 0F is copied and ends the code)
        if ((b & 0xFE) != 0xE8) return b == 0x9B ? (ES_ESC | (EA_ESC << 4)) : 0u;
    } else if ((b & 0xF0) != 0x80) return b == 0x9B ? (ES_ESC | (EA_ESC << 4)) : 0u;
    if (p + 4 >= hi) return ES_FAIL;                                             // a jump with fewer than 4 bytes left
    return 2u | (EA_JUMP << 4);
}

// forward ARM64 (EXECodec.cpp:239-292): B / BL with a target at or below 0 become an escape pair
__device__ __forceinline__ int ex_arm_target(u32 instr, u32 p)
{
    const int offset = (int)(instr & 0x03FFFFFFu);
    const int addr = (int)p + 4 * ((instr & 0x02000000u) == 0 ? offset : -(-offset & 0x03FFFFFF));
    return addr < 0 ? 0 : addr;
}
template <> __device__ __forceinline__ u32 ex_step<EK_ARMF>(const u8* q, u32 p, u32, u32)
{
    const u32 instr = ex_le32(q);
    if (!ex_is_bl(instr)) return 0;
    return (ex_arm_target(instr, p) == 0 ? EA_ESC : EA_JUMP) << 4;
}

// inverse ARM64 (EXECodec.cpp:458-505)
template <> __device__ __forceinline__ u32 ex_step<EK_ARMI>(const u8* q, u32, u32 s, u32)
{
    if (s) return 0;
    const u32 instr = ex_le32(q);
    if (!ex_is_bl(instr)) return 0;
    return (instr & 0x03FFFFFFu) == 0 ? (1u | (EA_ESC << 4)) : (EA_JUMP << 4);
}

// the state function of positions [a, e) of a staged chunk
template <int K> __device__ __forceinline__ u32 ex_walk_fn(const u8* sb, u32 base, u32 lo, u32 hi, u32 a, u32 e)
{
    constexpr u32 U = ExKind<K>::U, NS = ExKind<K>::NS;
    u32 f = EX_IDENT;
    if (NS == 1) return f;
#pragma unroll
    for (u32 s = 0; s < NS; s++) {
        u32 x = s;
        for (u32 u = a; u < e; u++) { const u32 p = lo + u * U; x = ex_step<K>(sb + (p - base), p, x, hi) & 15u; }
        f = (f & ~(7u << (3 * s))) | (x << (3 * s));
    }
    return f;
}

struct ExLds { u32 sw[EX_SB_WORDS]; u32 all[EX_T]; u32 hist[256]; u32 sh[4]; };

// pass 1: the state function of a chunk
template <int K> __device__ void ex_fn_body(const XfStage& st, int b, u32* ws, const ExInfo* info, ExLds& L)
{
    constexpr u32 U = ExKind<K>::U;
    if (ExKind<K>::NS == 1) return;
    const u32 lo = info->lo, hi = info->hi, nUnits = (hi - lo) / U;
    const u32 u0 = blockIdx.x * EX_CHUNK;
    if (u0 >= nUnits) return;
    const u32 base = lo + u0 * U;
    const u8* sb = ex_stage(L.sw, st.src[b], base, EX_CHUNK * U + EX_LOOK, st.len[b]);
    const u32 a = min(u0 + threadIdx.x * EX_SEG, nUnits), e = min(a + EX_SEG, nUnits);
    const u32 own = ex_walk_fn<K>(sb, base, lo, hi, a, e);
    ex_threads(ws, st.maxLen, blockIdx.x)[threadIdx.x] = own;
    const u32 f = ex_wg_scan(own, L.sh, L.all);
    if (threadIdx.x == EX_T - 1) ws[EX_CH + 4 * blockIdx.x] = f;
}

// pass 3: the entry state of every thread, and the counts of its stretch from that entry
template <int K> __device__ void ex_count_body(const XfStage& st, int b, u32* ws, ExInfo* info, ExLds& L)
{
    constexpr u32 U = ExKind<K>::U;
    const u32 lo = info->lo, hi = info->hi, nUnits = (hi - lo) / U;
    const u32 u0 = blockIdx.x * EX_CHUNK;
    if (u0 >= nUnits) return;
    const u32 base = lo + u0 * U;
    const u32 t = threadIdx.x;
    if (K == EK_DET) L.hist[t] = 0;
    const u8* sb = ex_stage(L.sw, st.src[b], base, EX_CHUNK * U + EX_LOOK, st.len[b]);
    const u32 a = min(u0 + t * EX_SEG, nUnits), e = min(a + EX_SEG, nUnits);
    u32 x = 0;
    if (ExKind<K>::NS > 1) {
        u32* own = ex_threads(ws, st.maxLen, blockIdx.x) + t;       // (what pass 1 walked)
        ex_wg_scan(*own, L.sh, L.all);
        x = ex_at(t ? L.all[t - 1] : EX_IDENT, ws[EX_CH + 4 * blockIdx.x]);
        *own = x;
    }
    u32 c0 = 0, c1 = 0;
    for (u32 u = a; u < e; u++) {
        const u32 p = lo + u * U;
        const u8* q = sb + (p - base);
        if (K == EK_DET) {                                       // EXECodec.cpp:560-597, for the visited positions
            if (x) { x--; continue; }
            const u32 v = q[0];
            atomicAdd(&L.hist[v], 1u);
            u32 i = p;
            if (p + 4 < hi && (v & 0xFE) == 0xE8) {
                if (q[4] == 0 || q[4] == 0xFF) { c0++; continue; }
            } else if (v == 0x0F && p + 1 < hi) {
                const u32 j = ((q[1] == 0x38 || q[1] == 0x3A) && p + 2 < hi) ? 2u : 1u;
                x = j;
                i = p + j;
                if ((q[j] & 0xF0) == 0x80) { c0++; continue; }
            }
            if ((i & 3) != 0 || i + 4 > hi) continue;            // (i counts from the block's first byte)
            const u32 instr = ex_le32(q + (i - p));
            const u32 op2 = instr & 0x7F000000u;
            if (ex_is_bl(instr) || op2 == 0x34000000u || op2 == 0x35000000u) c1++;
        } else {
            const u32 r = ex_step<K>(q, p, x, hi);
            if (K == EK_X86F && x != ES_STOP && (r & 15u) == ES_STOP) info->stop = p;
            x = r & 15u;
            const u32 act = r >> 4;
            c0 += act == EA_ESC;
            c1 += act == EA_JUMP;
        }
    }
    u32 t0, t1;
    ex_wg_sum(c0, L.sh, &t0);
    ex_wg_sum(c1, L.sh, &t1);
    if (K == EK_DET && L.hist[t]) atomicAdd(&ws[EX_HIST + t], L.hist[t]);
    if (t == 0) { ws[EX_CH + 4 * blockIdx.x + 1] = t0; ws[EX_CH + 4 * blockIdx.x + 2] = t1; }
}

__device__ __forceinline__ void ex_put_le32(u8* d, u32 v) { d[0] = (u8)v; d[1] = (u8)(v >> 8); d[2] = (u8)(v >> 16); d[3] = (u8)(v >> 24); }

// pass 5: the bytes of a chunk, and this workgroup's share of the bytes copied in front of the code and behind it
template <int K> __device__ void ex_emit_body(const XfStage& st, int b, const u32* ws, const ExInfo* info, ExLds& L)
{
    constexpr u32 U = ExKind<K>::U;
    constexpr bool FWD = K == EK_X86F || K == EK_ARMF;
    const u32 lo = info->lo, hi = info->hi, nUnits = (hi - lo) / U, n = st.len[b];
    const u8* __restrict__ src = st.src[b];
    u8* __restrict__ dst = st.dst[b];
    const u32 t = threadIdx.x;
    // forward: src[0, lo) -> dst[9..], src[end, n) -> behind the code; inverse: src[9, lo) -> dst[0..], src[end, n) -> behind the code
    const u32 end = lo + nUnits * U, from = FWD ? 0u : 9u;
    const u32 tailOut = FWD ? 9 + end + U * info->c0 : end - 9 - U * info->c0;
    for (u32 i = from + blockIdx.x * EX_T + t; i < lo; i += gridDim.x * EX_T) dst[FWD ? i + 9 : i - 9] = ldg<u8>(src + i);
    for (u32 i = end + blockIdx.x * EX_T + t; i < n; i += gridDim.x * EX_T) dst[tailOut + (i - end)] = ldg<u8>(src + i);
    const u32 u0 = blockIdx.x * EX_CHUNK;
    if (u0 >= nUnits) return;
    const u32 base = lo + u0 * U;
    const u8* sb = ex_stage(L.sw, src, base, EX_CHUNK * U + EX_LOOK, n);
    const u32 a = min(u0 + t * EX_SEG, nUnits), e = min(a + EX_SEG, nUnits);
    const u32 entry = ExKind<K>::NS > 1 ? ex_threads(const_cast<u32*>(ws), st.maxLen, blockIdx.x)[t] : 0u;
    u32 x = entry, c0 = 0;
    for (u32 u = a; u < e; u++) {
        const u32 p = lo + u * U;
        const u32 r = ex_step<K>(sb + (p - base), p, x, hi);
        x = r & 15u;
        c0 += (r >> 4) == EA_ESC;
    }
    u32 tot;
    u32 before = ws[EX_CH + 4 * blockIdx.x + 1] + ex_wg_sum(c0, L.sh, &tot) - c0;             // escapes in front of the position
    x = entry;
    for (u32 u = a; u < e; u++) {
        const u32 p = lo + u * U;
        const u8* q = sb + (p - base);
        const u32 r = ex_step<K>(q, p, x, hi);
        x = r & 15u;
        const u32 act = r >> 4;
        if (K == EK_X86F) {
            u8* d = dst + 9 + p + before;
            if (act == EA_ESC) { d[0] = 0x9B; d[1] = q[0]; }
            else if (act == EA_RAW) d[0] = q[0];
            else if (act == EA_JUMP) {
                const int offset = (int)ex_le32(q + 1);
                const int addr = (int)p + (q[4] == 0 ? offset : -(-offset & 0x00FFFFFF));
                const u32 v = (u32)addr ^ 0xF0F0F0F0u;
                d[0] = q[0]; d[1] = (u8)(v >> 24); d[2] = (u8)(v >> 16); d[3] = (u8)(v >> 8); d[4] = (u8)v;
            }
        } else if (K == EK_X86I) {
            const u32 o = p - 9 - before;
            if (act == EA_RAW) dst[o] = q[0];
            else if (act == EA_JUMP) {
                const int addr = (int)(ex_be32(q + 1) ^ 0xF0F0F0F0u);
                const int64_t offset = (int64_t)addr - (int64_t)o;
                const int enc = offset >= 0 ? (int)offset : -(int)((-offset) & 0x00FFFFFF);
                dst[o] = q[0];
                ex_put_le32(dst + o + 1, (u32)enc);
            }
        } else if (K == EK_ARMF) {
            u8* d = dst + 9 + p + 4 * before;
            const u32 instr = ex_le32(q);
            if (act == EA_RAW) ex_put_le32(d, instr);
            else {
                const u32 val = (instr & 0xFC000000u) | ((u32)ex_arm_target(instr, p) >> 2);
                ex_put_le32(d, val);
                if (act == EA_ESC) ex_put_le32(d + 4, instr);    // address 0 marks the pair
            }
        } else if (K == EK_ARMI) {
            const u32 o = p - 9 - 4 * before;
            const u32 instr = ex_le32(q);
            if (act == EA_RAW) ex_put_le32(dst + o, instr);
            else if (act == EA_JUMP) {
                const int addr = (int)((instr & 0x03FFFFFFu) << 2);
                const int offset = (addr - (int)o) >> 2;
                ex_put_le32(dst + o, (instr & 0xFC000000u) | ((u32)offset & 0x03FFFFFFu));
            }
        }
        before += act == EA_ESC;
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// header parse (one thread per block)
// ---------------------------------------------------------------------------------------------------------------------

struct ExReader {
    const u8* src;
    __device__ u32 b(int64_t i) const { return ldg<u8>(src + i); }
    __device__ int le16(int64_t i) const { return (int)(int16_t)(b(i) | (b(i + 1) << 8)); }
    __device__ int be16(int64_t i) const { return (int)(int16_t)(b(i + 1) | (b(i) << 8)); }
    __device__ int le32(int64_t i) const { return (int)(b(i) | (b(i + 1) << 8) | (b(i + 2) << 16) | (b(i + 3) << 24)); }
    __device__ int be32(int64_t i) const { return (int)(b(i + 3) | (b(i + 2) << 8) | (b(i + 1) << 16) | (b(i) << 24)); }
    __device__ int64_t le64(int64_t i) const { return (int64_t)((u64)(u32)le32(i) | ((u64)(u32)le32(i + 4) << 32)); }
    __device__ int64_t be64(int64_t i) const { return (int64_t)((u64)(u32)be32(i + 4) | ((u64)(u32)be32(i) << 32)); }
};

__device__ inline bool ex_set_range(int count, int& codeStart, int& codeEnd, int64_t start, int64_t length)
{
    if (start < 0 || length < 0 || start > (int64_t)count || length > (int64_t)count - start) return false;
    if (codeStart == 0) codeStart = (int)start;
    codeEnd = (int)(start + length);
    return true;
}

// EXECodec::parseHeader for count >= 64 (a block below 4,096 bytes never gets here). A false return may have moved the range.
__device__ bool ex_parse_header(const u8* src, int count, u32 magic, int& arch, int& codeStart, int& codeEnd)
{
    const ExReader r{ src };
    if (magic == 0x4D5Au) {                                      // MZ
        const int posPE = r.le32(60);
        if (posPE > 0 && posPE <= count - 48 && r.le32(posPE) == 0x00004550) {
            if (!ex_set_range(count, codeStart, codeEnd, (int64_t)r.le32(posPE + 44), (int64_t)r.le32(posPE + 28))) return false;
            arch = r.le16(posPE + 4);
        }
        return true;
    }
    if (magic == 0x7F454C46u) {                                  // ELF, 32 / 64 bits in both byte orders
        const bool le = r.b(5) == 1, is64 = r.b(4) == 2;
        codeStart = 0;
        auto r16 = [&](int64_t i) { return le ? r.le16(i) : r.be16(i); };
        auto r32 = [&](int64_t i) { return le ? r.le32(i) : r.be32(i); };
        auto r64 = [&](int64_t i) { return le ? r.le64(i) : r.be64(i); };
        const int nbEntries = r16(is64 ? 0x3C : 0x30), szEntry = r16(is64 ? 0x3A : 0x2E);
        const int64_t posSection = is64 ? r64(0x28) : (int64_t)r32(0x20);
        const int hs = is64 ? 0x28 : 0x18;
        if (szEntry <= 0 || posSection < 0 || posSection > (int64_t)count - hs) return false;
        for (int i = 0; i < nbEntries; i++) {
            const int64_t startEntry = posSection + (int64_t)i * (int64_t)szEntry;
            if (startEntry > (int64_t)count - hs) return false;
            const int typeSection = r32(startEntry + 4);
            const int64_t offSection = is64 ? r64(startEntry + 0x18) : (int64_t)r32(startEntry + 0x10);
            const int64_t lenSection = is64 ? r64(startEntry + 0x20) : (int64_t)r32(startEntry + 0x14);
            if (typeSection == 1 && lenSection >= 64 && !ex_set_range(count, codeStart, codeEnd, offSection, lenSection)) return false;
        }
        arch = r16(18);
        codeStart = min(codeStart, count);
        codeEnd = min(codeEnd, count);
        return true;
    }
    if (magic == 0xFEEDFACEu || magic == 0xCEFAEDFEu || magic == 0xFEEDFACFu || magic == 0xCFFAEDFEu) {      // Mach-O
        const bool is64 = magic == 0xFEEDFACFu || magic == 0xCFFAEDFEu;
        codeStart = 0;
        if (r.le32(12) != 0x02) return false;                    // MH_EXECUTE
        arch = r.le32(4);
        const int nbCmds = r.le32(0x10);
        int pos = is64 ? 0x20 : 0x1C;
        const int szSegHdr = is64 ? 0x48 : 0x38, minSectionSize = is64 ? 0x38 : 0x30;
        const u8 seg[6] = { '_', '_', 'T', 'E', 'X', 'T' }, sec[6] = { '_', '_', 't', 'e', 'x', 't' };
        for (int cmd = 0; cmd < nbCmds; cmd++) {
            if (pos < 0 || pos > count - 8) return false;
            const int ldCmd = r.le32(pos), szCmd = r.le32(pos + 4);
            if (szCmd < 8 || szCmd > count - pos) return false;
            if (ldCmd == 0x01 || ldCmd == 0x19) {
                if (pos > count - 14 || pos > count - szSegHdr) return false;
                bool same = true;
                for (int k = 0; k < 6; k++) same = same && r.b(pos + 8 + k) == seg[k];
                if (same) {
                    const int posSection = pos + szSegHdr;
                    if (posSection > count - minSectionSize) return false;
                    same = true;
                    for (int k = 0; k < 6; k++) same = same && r.b(posSection + k) == sec[k];
                    if (same) {                                  // the text section of the TEXT segment
                        const int64_t start = is64 ? r.le64(posSection + 0x30) : (int64_t)r.le32(posSection + 0x2C);
                        if (!ex_set_range(count, codeStart, codeEnd, start, (int64_t)r.le32(posSection + 0x28))) return false;
                        break;
                    }
                }
            }
            pos += szCmd;
        }
        codeStart = min(codeStart, count);
        codeEnd = min(codeEnd, count);
        return true;
    }
    return false;
}

__device__ __forceinline__ bool ex_bad_range(int codeStart, int codeEnd, int blockSize)
{
    return codeStart < 0 || codeStart > blockSize || codeEnd < codeStart || codeEnd > blockSize;
}

// ---------------------------------------------------------------------------------------------------------------------
// forward
// ---------------------------------------------------------------------------------------------------------------------

// the gates of EXECodec::forward, parseHeader and the part of detectType in front of the scan
__global__ __launch_bounds__(EX_T) void k_ex_f_head(XfStage st, u32* scratch, size_t stride)
{
    const int b = blockIdx.x;
    u32* ws = scratch + (size_t)b * stride;
    ExInfo* info = reinterpret_cast<ExInfo*>(ws + EX_INFO);
    ws[EX_HIST + threadIdx.x] = 0;
    if (threadIdx.x != 0) return;
    const u32 n = st.len[b];
    ExInfo o = {};
    st.ok[b] = n == 0 ? 1 : 0;
    st.newLen[b] = 0;
    bool go = n >= EX_MIN && n <= EX_MAX && (u64)st.cap[b] >= (u64)n + n / 8;
    const int dt = st.dtype ? st.dtype[b] : DT_UNDEFINED;
    if (dt != DT_UNDEFINED && dt != DT_EXE && dt != DT_BIN) go = false;
    if (go) {
        const u8* src = st.src[b];
        const int count = (int)n;
        int codeStart = 0, codeEnd = count, arch = 0, cnt = count;
        u8 hd[4];
        for (int k = 0; k < 4; k++) hd[k] = ldg<u8>(src + k);
        int verdict = -1;                                        // -1: scan, 0: NOT_EXE | UNDEFINED, else the mode
        if (ex_parse_header(src, count, knz_magic::magic_of(hd), arch, codeStart, codeEnd)) {
            if (ex_bad_range(codeStart, codeEnd, count)) verdict = 0;
            else switch (arch) {
                case 0x03: case 0x3E: case 0x014C: case 0x8664: case 0x01000007: verdict = EX_X86; break;
                case 0xB7: case 0xAA64: case 0x0100000C: verdict = EX_ARM64; break;
                default: cnt = codeEnd - codeStart;              // a known header of an unknown architecture
            }
        }
        if (verdict < 0 && (ex_bad_range(codeStart, codeEnd, count) || cnt <= 0)) verdict = 0;
        o.codeStart = (u32)codeStart; o.codeEnd = (u32)codeEnd; o.count = (u32)cnt;
        o.lo = (u32)codeStart; o.hi = (u32)codeEnd; o.stop = (u32)codeEnd;
        if (verdict < 0) o.det = EK_DET;
        else if (verdict == 0) { if (st.dtype) st.dtype[b] = DT_UNDEFINED; }
        else o.kind = verdict == (int)EX_X86 ? EK_X86F : EK_ARMF;
    }
    *info = o;
}

// pass 4 (one workgroup per block): the offset of every chunk's first escape and the totals; thread 0 goes on to the verdict. The totals
// are complete for thread 0 alone when this returns
__device__ void ex_sum_chunks(u32* ws, ExInfo* info, u32 U)
{
    const u32 nUnits = (info->hi - info->lo) / U, nCh = (nUnits + EX_CHUNK - 1) / EX_CHUNK;
    __shared__ u32 sh[4];
    u32 run0 = 0, run1 = 0;
    for (u32 base = 0; base < nCh; base += EX_T) {
        const u32 j = base + threadIdx.x;
        const u32 v0 = j < nCh ? ws[EX_CH + 4 * j + 1] : 0u, v1 = j < nCh ? ws[EX_CH + 4 * j + 2] : 0u;
        u32 t0, t1;
        const u32 incl = ex_wg_sum(v0, sh, &t0);
        ex_wg_sum(v1, sh, &t1);
        if (j < nCh) ws[EX_CH + 4 * j + 1] = run0 + incl - v0;
        run0 += t0; run1 += t1;
    }
    if (threadIdx.x == 0) { info->c0 = run0; info->c1 = run1; }
}

// the thresholds of detectType behind the scan (EXECodec.cpp:599-624)
__global__ __launch_bounds__(EX_T) void k_ex_f_decide(XfStage st, u32* scratch, size_t stride)
{
    const int b = blockIdx.x;
    u32* ws = scratch + (size_t)b * stride;
    ExInfo* info = reinterpret_cast<ExInfo*>(ws + EX_INFO);
    if (info->det != EK_DET) return;
    ex_sum_chunks(ws, info, 1);                                  // c0: x86 jumps, c1: ARM64 jumps
    if (threadIdx.x != 0) return;
    const u32* histo = ws + EX_HIST;
    const u32 count = info->count;
    const int dt = pk_simple_type(count, histo);
    u32 kind = EK_NONE;
    if (dt == DT_BIN && histo[0] >= count / 10 && histo[255] >= count / 100) {
        u32 smallVals = 0;
        for (int i = 0; i < 16; i++) smallVals += histo[i];
        if (smallVals <= count / 2) {
            if (info->c0 >= count / 200) kind = EK_X86F;
            else if (info->c1 >= count / 200) kind = EK_ARMF;
        }
    }
    info->kind = kind;
    if (kind == EK_NONE && st.dtype) st.dtype[b] = (u8)dt;       // a NOT_EXE verdict overwrites the type, UNDEFINED included
}

__global__ __launch_bounds__(EX_T) void k_ex_fn(XfStage st, u32* scratch, size_t stride, int det)
{
    const int b = blockIdx.y;
    u32* ws = scratch + (size_t)b * stride;
    const ExInfo* info = reinterpret_cast<const ExInfo*>(ws + EX_INFO);
    __shared__ ExLds L;
    switch (det ? info->det : info->kind) {
    case EK_DET: ex_fn_body<EK_DET>(st, b, ws, info, L); break;
    case EK_X86F: ex_fn_body<EK_X86F>(st, b, ws, info, L); break;
    case EK_X86I: ex_fn_body<EK_X86I>(st, b, ws, info, L); break;
    case EK_ARMI: ex_fn_body<EK_ARMI>(st, b, ws, info, L); break;
    default: break;
    }
}

// pass 2 (one workgroup per block): every chunk's entry state, the exit state of the parse
__global__ __launch_bounds__(EX_T) void k_ex_scan(XfStage st, u32* scratch, size_t stride, int det)
{
    const int b = blockIdx.x;
    u32* ws = scratch + (size_t)b * stride;
    ExInfo* info = reinterpret_cast<ExInfo*>(ws + EX_INFO);
    const u32 kind = det ? info->det : info->kind;
    if (kind == EK_NONE || kind == EK_ARMF) return;
    const u32 U = kind == EK_ARMI ? 4u : 1u;
    const u32 nUnits = (info->hi - info->lo) / U, nCh = (nUnits + EX_CHUNK - 1) / EX_CHUNK;
    __shared__ u32 all[EX_T];
    __shared__ u32 sh[4];
    u32 state = 0;
    for (u32 base = 0; base < nCh; base += EX_T) {
        const u32 j = base + threadIdx.x;
        ex_wg_scan(j < nCh ? ws[EX_CH + 4 * j] : EX_IDENT, sh, all);
        if (j < nCh) ws[EX_CH + 4 * j] = ex_at(threadIdx.x ? all[threadIdx.x - 1] : EX_IDENT, state);
        state = ex_at(all[EX_T - 1], state);
        __syncthreads();
    }
    if (threadIdx.x == 0) info->last = state;
}

__global__ __launch_bounds__(EX_T) void k_ex_count(XfStage st, u32* scratch, size_t stride, int det)
{
    const int b = blockIdx.y;
    u32* ws = scratch + (size_t)b * stride;
    ExInfo* info = reinterpret_cast<ExInfo*>(ws + EX_INFO);
    __shared__ ExLds L;
    switch (det ? info->det : info->kind) {
    case EK_DET: ex_count_body<EK_DET>(st, b, ws, info, L); break;
    case EK_X86F: ex_count_body<EK_X86F>(st, b, ws, info, L); break;
    case EK_ARMF: ex_count_body<EK_ARMF>(st, b, ws, info, L); break;
    case EK_X86I: ex_count_body<EK_X86I>(st, b, ws, info, L); break;
    case EK_ARMI: ex_count_body<EK_ARMI>(st, b, ws, info, L); break;
    default: break;
    }
}

__global__ __launch_bounds__(EX_T) void k_ex_f_verdict(XfStage st, u32* scratch, size_t stride)
{
    const int b = blockIdx.x;
    u32* ws = scratch + (size_t)b * stride;
    ExInfo* info = reinterpret_cast<ExInfo*>(ws + EX_INFO);
    const u32 kind = info->kind;
    if (kind != EK_X86F && kind != EK_ARMF) return;
    const u32 U = kind == EK_ARMF ? 4u : 1u;
    ex_sum_chunks(ws, info, U);
    if (threadIdx.x != 0) return;
    // The reference's loops also end when dstIdx reaches dstEnd = capacity - 5 (ARM64: - 8). That exit needs no model: the gate gave
    // capacity >= n + n / 8, so dstIdx >= n + n / 8 - 8 there, and the final length is no smaller. With n >= 4096, n / 8 - n / 50 >=
    // 0.105 n - 1 >= 429 > 8, so that length exceeds n + n / 50 and the block is refused by the cap on the expansion below, as it is
    // by the reference (at the loop's exit, or at that cap).
    const u32 n = st.len[b], cap = st.cap[b];
    const u32 grow = U * info->c0;                               // escapes (x86), 4 bytes per escape pair (ARM64)
    const u32 srcIdx = kind == EK_X86F ? info->stop : info->lo + (info->hi - info->lo) / 4 * 4;
    const u64 total = 9ull + n + grow;
    const u32 dstEnd = cap - (kind == EK_X86F ? 5u : 8u);
    const bool ok = info->c1 >= 16 && total <= dstEnd && total <= (u64)n + n / 50;
    info->ok = ok ? 1u : 0u;
    st.ok[b] = ok ? 1 : 0;
    st.newLen[b] = ok ? (u32)total : 0u;
    if (!ok) return;                                             // (the type stays as it is)
    u8* dst = st.dst[b];
    dst[0] = (u8)(kind == EK_X86F ? EX_X86 : EX_ARM64);
    ex_put_le32(dst + 1, info->codeStart);
    ex_put_le32(dst + 5, 9 + srcIdx + grow);
    if (st.dtype) st.dtype[b] = DT_EXE;
}

__global__ __launch_bounds__(EX_T) void k_ex_emit(XfStage st, u32* scratch, size_t stride)
{
    const int b = blockIdx.y;
    const u32* ws = scratch + (size_t)b * stride;
    const ExInfo* info = reinterpret_cast<const ExInfo*>(ws + EX_INFO);
    if (!info->ok) return;
    __shared__ ExLds L;
    switch (info->kind) {
    case EK_X86F: ex_emit_body<EK_X86F>(st, b, ws, info, L); break;
    case EK_ARMF: ex_emit_body<EK_ARMF>(st, b, ws, info, L); break;
    case EK_X86I: ex_emit_body<EK_X86I>(st, b, ws, info, L); break;
    case EK_ARMI: ex_emit_body<EK_ARMI>(st, b, ws, info, L); break;
    default: break;
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// inverse
// ---------------------------------------------------------------------------------------------------------------------

// the capacity the verdict goes by (XfStage::capModel: the last inverse stage of a stream writes into a destination smaller than its
// input, the reference into a buffer with slack)
__device__ __forceinline__ u32 ex_judged_cap(const XfStage& st, int b) { const u32 room = st.cap[b]; return room > st.capModel ? room : st.capModel; }

// EXECodec::inverse and the header sanity of inverseX86 / inverseARM (EXECodec.cpp:314-352, :444-450)
__global__ __launch_bounds__(64) void k_ex_i_head(XfStage st, u32* scratch, size_t stride)
{
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= st.nBlocks) return;
    u32* ws = scratch + (size_t)b * stride;
    ExInfo* info = reinterpret_cast<ExInfo*>(ws + EX_INFO);
    const u32 count = st.len[b];
    ExInfo o = {};
    st.ok[b] = count == 0 ? 1 : 0;
    st.newLen[b] = 0;
    if (count >= 9) {
        const ExReader r{ st.src[b] };
        const u32 mode = r.b(0);
        const int codeStart = r.le32(1), codeEnd = r.le32(5);
        const bool bad = codeStart < 0 || codeEnd < 9 || (u32)codeEnd > count || codeStart > codeEnd - 9 || (u32)codeStart > ex_judged_cap(st, b);
        if (!bad && (mode == EX_X86 || mode == EX_ARM64)) {
            o.kind = mode == EX_X86 ? EK_X86I : EK_ARMI;
            o.codeStart = (u32)codeStart; o.codeEnd = (u32)codeEnd;
            o.lo = 9 + (u32)codeStart; o.hi = (u32)codeEnd;
        }
    }
    *info = o;
}

__global__ __launch_bounds__(EX_T) void k_ex_i_verdict(XfStage st, u32* scratch, size_t stride)
{
    const int b = blockIdx.x;
    u32* ws = scratch + (size_t)b * stride;
    ExInfo* info = reinterpret_cast<ExInfo*>(ws + EX_INFO);
    const u32 kind = info->kind;
    if (kind != EK_X86I && kind != EK_ARMI) return;
    const u32 U = kind == EK_ARMI ? 4u : 1u;
    ex_sum_chunks(ws, info, U);
    if (threadIdx.x != 0) return;
    // Every capacity guard of the reference's loops covers bytes that the output holds, and the last one covers all of them, so
    // together they ask that the whole output fits. x86: an escape as the last byte of the code and a jump with fewer than 4 bytes
    // left are exit states of the parse. ARM64: a code length that is no multiple of 4 runs into srcIdx + 4 > codeEnd, an escape in the
    // last word into srcIdx + 8 > codeEnd.
    const u32 count = st.len[b];
    const u32 total = count - 9 - U * info->c0;
    const bool fail = kind == EK_X86I ? info->last != 0 : (((info->hi - info->lo) & 3) != 0 || info->last != 0);
    // (a block that passes by the reference's capacity and does not fit the destination is refused too: it is larger than a block may be)
    const bool ok = !fail && total <= ex_judged_cap(st, b) && total <= st.cap[b];
    info->ok = ok ? 1u : 0u;
    st.ok[b] = ok ? 1 : 0;
    st.newLen[b] = ok ? total : 0u;
}

}  // namespace

size_t exe_scratch_bytes(int nBlocks, u32 maxLen) { return (size_t)nBlocks * ex_stride_u32(maxLen) * 4 + 256; }

#define EX_LAUNCH(name, k, grid, threads, ...) do { KScope ks_(name); hipLaunchKernelGGL(k, grid, dim3(threads), 0, s, __VA_ARGS__); } while (0)

void launch_exe_forward(hipStream_t s, const XfStage& st, void* scratch)
{
    u32* ws = reinterpret_cast<u32*>(scratch);
    const size_t stride = ex_stride_u32(st.maxLen);
    const dim3 grid(ex_chunks(st.maxLen), (unsigned)st.nBlocks), one((unsigned)st.nBlocks), few((unsigned)(st.nBlocks + 63) / 64);
    EX_LAUNCH("k_ex_f_head", k_ex_f_head, one, EX_T, st, ws, stride);
    EX_LAUNCH("k_ex_det_fn", k_ex_fn, grid, EX_T, st, ws, stride, 1);
    EX_LAUNCH("k_ex_det_scan", k_ex_scan, one, EX_T, st, ws, stride, 1);
    EX_LAUNCH("k_ex_det_count", k_ex_count, grid, EX_T, st, ws, stride, 1);
    EX_LAUNCH("k_ex_f_decide", k_ex_f_decide, one, EX_T, st, ws, stride);
    EX_LAUNCH("k_ex_f_fn", k_ex_fn, grid, EX_T, st, ws, stride, 0);
    EX_LAUNCH("k_ex_f_scan", k_ex_scan, one, EX_T, st, ws, stride, 0);
    EX_LAUNCH("k_ex_f_count", k_ex_count, grid, EX_T, st, ws, stride, 0);
    EX_LAUNCH("k_ex_f_verdict", k_ex_f_verdict, one, EX_T, st, ws, stride);
    EX_LAUNCH("k_ex_f_emit", k_ex_emit, grid, EX_T, st, ws, stride);
}

void launch_exe_inverse(hipStream_t s, const XfStage& st, void* scratch)
{
    u32* ws = reinterpret_cast<u32*>(scratch);
    const size_t stride = ex_stride_u32(st.maxLen);
    const dim3 grid(ex_chunks(st.maxLen), (unsigned)st.nBlocks), one((unsigned)st.nBlocks), few((unsigned)(st.nBlocks + 63) / 64);
    EX_LAUNCH("k_ex_i_head", k_ex_i_head, few, 64, st, ws, stride);
    EX_LAUNCH("k_ex_i_fn", k_ex_fn, grid, EX_T, st, ws, stride, 0);
    EX_LAUNCH("k_ex_i_scan", k_ex_scan, one, EX_T, st, ws, stride, 0);
    EX_LAUNCH("k_ex_i_count", k_ex_count, grid, EX_T, st, ws, stride, 0);
    EX_LAUNCH("k_ex_i_verdict", k_ex_i_verdict, one, EX_T, st, ws, stride);
    EX_LAUNCH("k_ex_i_emit", k_ex_emit, grid, EX_T, st, ws, stride);
}

}  // namespace knz
