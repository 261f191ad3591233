// LZP (LZPCodec, kanzi transform id 14) on gfx950, forward and inverse: one wave per block.
//
// Reference being replaced: transform/LZCodec.cpp:763-879 (forward), :881-992 (inverse), LZCodec.hpp:158-161 (getMaxEncodedLength),
// :251-267 (findMatch). 16-bit hash of a 4-byte context, matches of 64 bytes and more only, written as 0xFC, one 0xFE per 254 bytes
// beyond 64 and the remainder; a literal 0xFC whose bucket is filled is followed by 0xFF.
//
// Both directions are one dependent chain per block through a table of 65,536 positions (256 KiB: the stage's scratch, cleared by the
// launcher on the stream). The table belongs to one wave, so plain loads and stores agree (same CU, same L1). The wave walks the chain
// with uniform control flow and spends its lanes under every decision:
//   forward  the next 64 positions of a literal stretch at once. Lane i forms the context position s + i would have after i literals,
//            reads its bucket (a lane whose bucket an earlier lane of the batch would have stored takes that lane's position), runs the
//            8-byte pre-check and the 64-byte compare. The first lane with a match decides; the lanes in front of it are literals: their
//            buckets are stored (the latest position of a bucket stays), their bytes and escapes go out by ballot and prefix count. The
//            match is measured 512 bytes per step with the reference's whole-word stopping rule, its 0xFE run written 512 bytes per step.
//   inverse  bytes other than 0xFC are literals whatever the table holds: the wave copies up to the next 0xFC, stores those positions'
//            buckets from the contexts of the bytes written, then resolves the flag with one lookup behind those stores. A match is
//            copied by the whole wave, as a modulo gather when it overlaps itself (dst[p] = dst[p - distance] for every byte).
// The context is no plain function of the position (LZCodec.cpp:813, :830, :844): it is reloaded as the little-endian word in front of
// the position at the block start and after a match and then shifted left by one byte per literal, so for the first three literals
// after a reload it mixes both byte orders. `run` (literals since the reload, 4 = four or more) is part of the walk's state.
// The forward's refusals inside the loop all mean "the output reached dstEnd": dstIdx only grows and the result is false once it gets
// there, so the walk stops at the first batch that reaches it. Nothing is written at or behind dstEnd (forward) or the capacity (inverse).
#include "common.hpp"
#include "stages.hpp"

namespace knz {

namespace {

constexpr u32 LZP_HASH_LOG = 16;
constexpr u32 LZP_TABLE = 1u << LZP_HASH_LOG;             // positions per block
constexpr u32 LZP_MIN_MATCH = 64;
constexpr u32 LZP_MIN_BLOCK = 128;
constexpr u32 LZP_FLAG = 0xFC;

__host__ __device__ inline u32 lzp_max_encoded(u32 n) { return (n <= 1024) ? n + 16 : n + n / 64; }      // = knz_max_encoded_len(KNZ_T_LZP, n)

__device__ __forceinline__ u32 lzp_hash(u32 ctx) { return (0x7FEB352Du * ctx) >> (32 - LZP_HASH_LOG); }

// The context the reference holds when it visits position p (>= 4) with `run` literals behind the last reload (4 = four or more):
// the little-endian word at p - run - 4, shifted left by `run` bytes, with the `run` literals below it, newest lowest.
__device__ __forceinline__ u32 lzp_ctx(const u8* t, u32 p, u32 run)
{
    u64 w = 0;                                            // byte k = t[p - 1 - k]
    if (p >= 8) w = __builtin_bswap64(ldg_u<u64>(t + p - 8));
    else for (u32 k = 0; k < p; k++) w |= (u64)ldg<u8>(t + p - 1 - k) << (8 * k);
    if (run >= 4) return (u32)w;
    const u32 word = __builtin_bswap32((u32)(w >> (8 * run)));
    return (u32)(((u64)word << (8 * run)) | (w & ((1ull << (8 * run)) - 1)));
}

// true when two lanes of `act` share their hash (the filter has one bit per hash value, so it is exact); leaves the filter clear
__device__ __forceinline__ bool lzp_dups(u32* seen /* [2048] in LDS */, u32 h, bool act)
{
    const u32 fbit = 1u << (h & 31), fidx = h >> 5;
    const u32 old = act ? atomicOr(&seen[fidx], fbit) : 0u;
    KNZ_WAVE_ORDER();                                     // every lane's OR before any lane's AND (one instruction each on the GPU)
    if (act) atomicAnd(&seen[fidx], ~fbit);
    return __ballot(act && (old & fbit)) != 0;
}

// table[h] = p for every lane of `act`, in lane order: with equal hashes the highest lane (the latest position) stays
__device__ __forceinline__ void lzp_put_wave(u32* table, u32 h, u32 p, bool act, bool dups, int lane)
{
    bool lose = false;
    if (dups) {
#pragma unroll 9
        for (int j = 1; j < 64; j++) {
            const u32 hj = (u32)__builtin_amdgcn_readlane((int)h, j);
            const int aj = __builtin_amdgcn_readlane(act ? 1 : 0, j);
            if (aj && j > lane && hj == h) lose = true;
        }
    }
    if (act && !lose) table[h] = p;
}

// LZPCodec::findMatch with the whole wave from offset n on: whole 8-byte words only, so the result may stop up to 7 bytes short of `limit`
__device__ u32 lzp_match(const u8* s, u32 a, u32 b, u32 limit, int lane, u32 n)
{
    for (;;) {
        const u32 o = n + 8u * (u32)lane;
        const bool valid = o + 8 <= limit && o + 8 > o;
        u64 x = 0;
        if (valid) x = ldg_u<u64>(s + a + o) ^ ldg_u<u64>(s + b + o);
        const u64 stop = __ballot(!valid || x != 0);
        if (stop) {
            const int f = __ffsll((long long)stop) - 1;
            const u32 xl = rl((u32)x, f);
            const u32 xh = rl((u32)(x >> 32), f);
            const int vf = __builtin_amdgcn_readlane(valid ? 1 : 0, f);
            if (!vf) return n + 8u * (u32)f;
            return n + 8u * (u32)f + (u32)(xl ? (__ffs((int)xl) - 1) >> 3 : 4 + ((__ffs((int)xh) - 1) >> 3));
        }
        n += 512;
    }
}

__global__ __launch_bounds__(64) void k_lzp_forward(XfStage st, u32* __restrict__ tables)
{
    const int b = blockIdx.x;
    const int lane = lane_id();
    const u32 count = st.len[b];
    if (count == 0) return;
    const u8* __restrict__ src = st.src[b];
    u8* __restrict__ dst = st.dst[b];
    u32* table = tables + (size_t)b * LZP_TABLE;
    __shared__ u32 seen[2048];
    for (int i = lane; i < 2048; i += 64) seen[i] = 0;
    __syncthreads();
    u32 ok = 0, d = 0;
    if (count >= 4 && st.cap[b] >= lzp_max_encoded(count) && count >= LZP_MIN_BLOCK) {
        const u32 dstEnd = count - (count >> 6);
        if (lane < 4) dst[lane] = src[lane];
        u32 s = 4, run = 0;
        d = 4;
        ok = 1;
        while (s < count) {
            KNZ_WAVE_ORDER();
            // ---- the next (up to 64) positions as if all of them were literals
            const u32 p = s + (u32)lane;
            const bool act = p < count;
            const u32 r = run + (u32)lane;
            u32 h = 0, ref = 0;
            if (act) { h = lzp_hash(lzp_ctx(src, p, r < 4 ? r : 4u)); ref = table[h]; }
            const bool dups = lzp_dups(seen, h, act);
            if (dups) {
#pragma unroll 9
                for (int j = 0; j < 63; j++) {
                    const u32 hj = (u32)__builtin_amdgcn_readlane((int)h, j);
                    const int aj = __builtin_amdgcn_readlane(act ? 1 : 0, j);
                    if (aj && lane > j && hj == h) ref = s + (u32)j;
                }
            }
            bool hit = false;
            if (act && ref != 0 && p + LZP_MIN_MATCH < count && ldg_u<u64>(src + ref + 56) == ldg_u<u64>(src + p + 56)) {
                hit = true;
#pragma unroll
                for (u32 k = 0; k < 56; k += 8) hit = hit && ldg_u<u64>(src + ref + k) == ldg_u<u64>(src + p + k);
            }
            const u64 hitMask = __ballot(hit);
            const u32 nAct = count - s < 64u ? count - s : 64u;
            const u32 m = hitMask ? (u32)(__ffsll((long long)hitMask) - 1) : 64u;
            const u32 f = m < nAct ? m : nAct;                                    // literals in front of the match / of the batch's end
            // ---- their bytes and escapes
            const bool lit = (u32)lane < f;
            const u32 v = lit ? ldg<u8>(src + p) : 0u;
            const bool esc = lit && v == LZP_FLAG && ref != 0;
            const u64 escMask = __ballot(esc);
            const u32 off = d + (u32)lane + (u32)__popcll(escMask & __lanemask_lt());
            if (lit && off < dstEnd) dst[off] = (u8)v;
            if (esc && off + 1 < dstEnd) dst[off + 1] = 0xFF;
            // ---- every visited position is stored, the match's own included
            lzp_put_wave(table, h, p, act && (u32)lane <= m, dups, lane);
            s += f;
            d += f + (u32)__popcll(escMask);
            run = run + f < 4 ? run + f : 4u;
            if (d >= dstEnd) { ok = 0; break; }
            if (m >= nAct) continue;
            // ---- the match at s
            const u32 mref = rl(ref, m);
            const u32 len = lzp_match(src, s, mref, count - s, lane, LZP_MIN_MATCH);
            const u32 rest = len - LZP_MIN_MATCH;
            const u32 nFE = rest / 254;
            if ((u64)d + 1 + nFE >= dstEnd) { ok = 0; break; }
            if (lane == 0) { dst[d] = (u8)LZP_FLAG; dst[d + 1 + nFE] = (u8)(rest - 254 * nFE); }
            u8* fe = dst + d + 1;
            const u32 bulk = nFE & ~7u;
            for (u32 i = 8u * (u32)lane; i < bulk; i += 512) st_u<u64>(fe + i, 0xFEFEFEFEFEFEFEFEull);
            if ((u32)lane < nFE - bulk) fe[bulk + lane] = 0xFE;
            d += nFE + 2;
            s += len;
            run = 0;
        }
        if (ok && !(s == count && d < dstEnd)) ok = 0;
    }
    if (lane == 0) { st.ok[b] = (u8)ok; st.newLen[b] = ok ? d : 0u; }
}

__global__ __launch_bounds__(64) void k_lzp_inverse(XfStage st, u32* __restrict__ tables)
{
    const int b = blockIdx.x;
    const int lane = lane_id();
    const u32 count = st.len[b];
    if (count == 0) return;
    const u8* __restrict__ src = st.src[b];
    u8* dst = st.dst[b];
    u32* table = tables + (size_t)b * LZP_TABLE;
    const u32 dstEnd = st.cap[b];
    __shared__ u32 seen[2048];
    for (int i = lane; i < 2048; i += 64) seen[i] = 0;
    __syncthreads();
    u32 ok = 0, di = 0;
    if (count >= 4 && dstEnd >= count) {
        if (lane < 4) dst[lane] = src[lane];
        u32 si = 4, run = 0;
        di = 4;
        ok = 1;
        while (si < count) {
            // ---- literals up to the next 0xFC
            const bool act = si + (u32)lane < count && si + (u32)lane >= si;
            const u32 v = act ? ldg<u8>(src + si + lane) : 0u;
            const u64 flagMask = __ballot(act && v == LZP_FLAG);
            const u32 nAct = count - si < 64u ? count - si : 64u;
            const u32 m = flagMask ? (u32)(__ffsll((long long)flagMask) - 1) : 64u;
            const u32 f = m < nAct ? m : nAct;
            if (f > dstEnd - di) { ok = 0; break; }                               // a literal does not fit
            const bool lit = (u32)lane < f;
            if (lit) dst[di + lane] = (u8)v;
            wave_fence();                                                     // contexts come from the bytes written (this batch, the match before it)
            // ---- their buckets, and the flag's context
            const u32 p = di + (u32)lane;
            const u32 r = run + (u32)lane;
            const bool vis = (u32)lane <= f && (u32)lane < nAct;                  // the literals and the flag
            const u32 h = vis ? lzp_hash(lzp_ctx(dst, p, r < 4 ? r : 4u)) : 0u;
            const bool dups = lzp_dups(seen, h, lit);
            lzp_put_wave(table, h, p, lit, dups, lane);
            si += f; di += f;
            run = run + f < 4 ? run + f : 4u;
            if (m >= nAct) continue;
            // ---- 0xFC at si: one lookup behind those stores
            wave_fence();
            const u32 hf = rl(h, m);
            const u32 ref = (u32)uni((int)table[hf]);
            wave_fence();
            if (lane == 0) table[hf] = di;
            u32 literal = ref == 0 ? 1u : 0u;
            if (!literal) {
                si++;
                if (si >= count) { ok = 0; break; }
                if ((u32)uni((int)ldg<u8>(src + si)) == 0xFFu) literal = 2;
            }
            if (literal) {                                                        // 0xFC itself: its bucket was empty, or 0xFF follows
                if (di >= dstEnd) { ok = 0; break; }
                if (lane == 0) dst[di] = (u8)LZP_FLAG;
                si++; di++;
                run = run + 1 < 4 ? run + 1 : 4u;
                continue;
            }
            u64 mLen = LZP_MIN_MATCH;
            for (;;) {                                                            // the run of 0xFE, 64 bytes per step
                const bool in = si + (u32)lane < count && si + (u32)lane >= si;
                const u64 other = __ballot(!(in && ldg<u8>(src + si + lane) == 0xFEu));
                const u32 k = other ? (u32)(__ffsll((long long)other) - 1) : 64u;
                si += k;
                mLen += 254ull * k;
                if (other) break;
            }
            if (si >= count) { ok = 0; break; }
            mLen += (u32)uni((int)ldg<u8>(src + si));
            si++;
            if (mLen > (u64)(dstEnd - di)) { ok = 0; break; }
            const u32 len = (u32)mLen, dist = di - ref;
            if (dist >= len) {
                const u32 bulk = len & ~7u;
                for (u32 i = 8u * (u32)lane; i < bulk; i += 512) st_u<u64>(dst + di + i, ldg_u<u64>(dst + ref + i));
                if ((u32)lane < len - bulk) dst[di + bulk + lane] = dst[ref + bulk + lane];
            } else {
                for (u32 i = (u32)lane; i < len; i += 64) dst[di + i] = dst[ref + i % dist];
            }
            di += len;
            run = 0;
        }
        if (ok && si != count) ok = 0;
    }
    if (lane == 0) { st.ok[b] = (u8)ok; st.newLen[b] = ok ? di : 0u; }
}

}  // namespace

size_t lzp_scratch_bytes(int nBlocks, u32 /*maxLen*/) { return (size_t)nBlocks * LZP_TABLE * sizeof(u32); }

void launch_lzp_forward(hipStream_t s, const XfStage& st, void* scratch)
{
    if (st.nBlocks <= 0) return;
    (void)hipMemsetAsync(scratch, 0, lzp_scratch_bytes(st.nBlocks, st.maxLen), s);
    KScope ks_("k_lzp_forward");
    hipLaunchKernelGGL(k_lzp_forward, dim3(st.nBlocks), dim3(64), 0, s, st, static_cast<u32*>(scratch));
}

void launch_lzp_inverse(hipStream_t s, const XfStage& st, void* scratch)
{
    if (st.nBlocks <= 0) return;
    (void)hipMemsetAsync(scratch, 0, lzp_scratch_bytes(st.nBlocks, st.maxLen), s);
    KScope ks_("k_lzp_inverse");
    hipLaunchKernelGGL(k_lzp_inverse, dim3(st.nBlocks), dim3(64), 0, s, st, static_cast<u32*>(scratch));
}

}  // namespace knz
