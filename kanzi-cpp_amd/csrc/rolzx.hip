// ROLZX (ROLZCodec2, kanzi transform id 12) on gfx950, forward and inverse: one wave per block.
//
// Reference being replaced: transform/ROLZCodec.cpp:52-96 (the guards of ROLZCodec), :862-912 (findMatch), :914-1010 (forward),
// :1012-1109 (inverse), ROLZCodec.hpp:168-173 (getMaxEncodedLength), :227-240 (keys and hash), :289-309 (emitCopy), :311-365 and
// ROLZCodec.cpp:681-820 (ROLZEncoder / ROLZDecoder: an adaptive binary range coder over 56 bits that moves 32 bits at a time).
//
// Per block, in the stage's scratch: `matches`, 32 positions for each of 65,536 keys (8 MiB, cleared at every chunk of 16 MiB), the
// literal probabilities (256 << 9) and the match-index probabilities (256 << 5), both set to 0x7FFF at every chunk. `counters`
// (65,536 bytes, cleared once per block) lives in LDS. The tables belong to one wave; where one lane stores and other lanes load,
// a wave-scope fence stands between the two.
//   forward  one kernel, the wave walks the greedy parse and codes each token as it finds it.
//            findMatch: lanes 0-31 read the key's 32 candidates in one 128-byte row, newest first, and measure theirs in 8-byte
//            words; the serial scan's result (first longest candidate; the scan ends at the first candidate that reaches maxMatch
//            exactly, a candidate that overshoots it does not end it) comes out of one ballot and one wave maximum.
//            coding: the bits of a token are known before it is coded, so the probability of bit i is loaded, updated and stored by
//            lane i (9 lanes for a literal or a length, 5 more for an index): one round trip to the tables per token instead of one
//            per bit. Depth i of a context's tree is always lane i's, so no lane reads what another lane stored. The chain on
//            low / high runs in registers, the same in every lane; lane 0 writes the bytes.
//   inverse  serial by nature (decode, table update, copy), run with the same control flow in every lane: the probabilities of a
//            token's context are loaded as one row, 16 bytes per lane, and the dependent steps pick theirs from registers
//            (rx_decode); lane 0 writes the literals and keeps the tables; the wave copies a match (a modulo gather when it overlaps
//            itself) and clears the tables at a chunk's start.
// The forward stops and refuses as soon as the bytes written reach `count` (the reference writes on into its slack and refuses at
// the end: the same verdict). The inverse refuses when it would read 4 bytes that do not lie inside `count` (the reference ends with
// srcIdx != count), and when a literal or a copy would end behind the decoded length: the reference's own check (:1086) lets a copy
// of the 7-byte minimum run up to 4 bytes past the block's end and is looser still in a second chunk; there the reference writes
// outside the block and the device refuses. Nothing is written at or behind `count` (forward) or the decoded length (inverse).
#include <stdlib.h>

#include "common.hpp"
#include "datatype.hpp"
#include "stages.hpp"

namespace knz {

namespace {

constexpr u32 RX_LOG_POS = 5;                             // ROLZCodec2::LOG_POS_CHECKS
constexpr u32 RX_POS_MASK = (1u << RX_LOG_POS) - 1;
constexpr u32 RX_KEYS = 65536;
constexpr u32 RX_CHUNK = 1u << 24;
constexpr u32 RX_HASH = 200002979u;
constexpr u32 RX_HASH_MASK = ~(RX_CHUNK - 1);
constexpr u32 RX_MIN_BLOCK = 64;
constexpr u32 RX_MAX_BLOCK = 1u << 30;
constexpr int RX_MAX_MATCH = 3 + 255;
constexpr u64 RX_TOP = 0x00FFFFFFFFFFFFFFull;
constexpr u32 RX_MATCH_WORDS = RX_KEYS << RX_LOG_POS;     // 32-bit words of `matches`
constexpr u32 RX_LIT_PROBS = 256u << 9;
constexpr u32 RX_IDX_PROBS = 256u << RX_LOG_POS;
constexpr size_t RX_BLOCK_BYTES = (size_t)RX_MATCH_WORDS * 4 + ((size_t)RX_LIT_PROBS + RX_IDX_PROBS) * 2;      // 8,667,136

__host__ __device__ inline u32 rx_max_encoded(u32 n) { return n + (n < 32768 ? 1024u : n >> 5); }            // = knz_max_encoded_len(KNZ_T_ROLZX, n)

struct RxTables { u32* matches; u16* lit; u16* idx; };

__device__ __forceinline__ RxTables rx_tables(u8* base, int slot)
{
    u8* p = base + (size_t)slot * RX_BLOCK_BYTES;
    RxTables t;
    t.matches = reinterpret_cast<u32*>(p);
    t.lit = reinterpret_cast<u16*>(p + (size_t)RX_MATCH_WORDS * 4);
    t.idx = t.lit + RX_LIT_PROBS;
    return t;
}

// what the reference does at the start of every chunk: memset of `matches`, reset() of the coder's probabilities
__device__ void rx_chunk_reset(const RxTables& t, int lane)
{
    uint4* m = reinterpret_cast<uint4*>(t.matches);
    for (u32 i = (u32)lane; i < RX_MATCH_WORDS / 4; i += 64) m[i] = make_uint4(0, 0, 0, 0);
    u32* p = reinterpret_cast<u32*>(t.lit);                                       // (the two probability sets are adjacent)
    for (u32 i = (u32)lane; i < (RX_LIT_PROBS + RX_IDX_PROBS) / 2; i += 64) p[i] = 0x7FFF7FFFu;
    wave_fence();
}

// ROLZCodec::getKey1 / getKey2 of the bytes at p - delta, from the 8 bytes in front of p (w, little endian)
__device__ __forceinline__ u32 rx_key(u64 w, u32 delta)
{
    if (delta == 8) return (u32)((w * (u64)RX_HASH) >> 40) & (RX_KEYS - 1);
    return (u32)(w >> (64 - 8 * delta)) & (RX_KEYS - 1);
}
__device__ __forceinline__ u32 rx_hash(u32 w) { return ((w << 8) * RX_HASH) & RX_HASH_MASK; }

// ---- ROLZEncoder ---------------------------------------------------------------------------------
struct RxEnc { u64 low, high; u32 idx, lim, full; u8* buf; };

// NB bits of val, most significant first, under the probabilities at `probs` (the context's tree): lane i owns bit i
template <int NB>
__device__ __forceinline__ void rx_encode(RxEnc& e, u16* probs, u32 val, int lane)
{
    u32 p = 0;
    if (lane < NB) {
        const u32 c1 = (1u << lane) | (val >> (NB - lane));
        const u32 bit = (val >> (NB - 1 - lane)) & 1;
        p = probs[c1];
        probs[c1] = (u16)(bit ? (int)p - (((int)p - 0xFFFF + 32) >> 5) : (int)p - (int)(p >> 5));
    }
#pragma unroll
    for (int i = 0; i < NB; i++) {
        const u32 pi = rl(p, i);
        const u64 split = (((e.high - e.low) >> 4) * (u64)(pi >> 4)) >> 8;
        if ((val >> (NB - 1 - i)) & 1) e.high = e.low + split;
        else e.low += split + 1;
        while (((e.low ^ e.high) >> 24) == 0) {
            if (e.full || e.idx + 4 >= e.lim) e.full = 1;                          // the bytes written reach `count`: refused
            else { if (lane == 0) st_u<u32>(e.buf + e.idx, bswap32((u32)(e.high >> 32))); e.idx += 4; }
            e.low <<= 32;
            e.high = (e.high << 32) | 0xFFFFFFFFull;
        }
    }
}

// ROLZCodec2::findMatch at `pos` of the chunk `s` (which ends at `end`): the reference's return value, -1 for no match. Registers `pos`.
__device__ int rx_find_match(const RxTables& t, u8* counters, const u8* s, u32 pos, u32 end, u32 key, int minMatch, int lane)
{
    const u32 hash32 = rx_hash(ldg_u<u32>(s + pos));
    const int maxMatch = (int)(end - pos < (u32)RX_MAX_MATCH ? end - pos : (u32)RX_MAX_MATCH) - 8;
    const u32 counter = counters[key];
    u32* row = t.matches + ((size_t)key << RX_LOG_POS);
    int n = 0;
    if (lane <= (int)RX_POS_MASK && maxMatch > 0) {                                // lane j: the j-th candidate of the scan, newest first
        const u32 e = row[(counter - (u32)lane) & RX_POS_MASK];
        if ((e & RX_HASH_MASK) == hash32) {                                        // (a zeroed entry is position 0 whenever hash32 is 0)
            const u8* a = s + (e & ~RX_HASH_MASK);
            const u8* c = s + pos;
            while (n < maxMatch) {
                const u64 x = ldg_u<u64>(a + n) ^ ldg_u<u64>(c + n);
                if (x) { n += (__ffsll((long long)x) - 1) >> 3; break; }
                n += 8;
            }
        }
    }
    // the scan ends behind the first candidate that reaches maxMatch, if it is maxMatch exactly (all before it are shorter: it wins)
    const u64 reach = __ballot(maxMatch > 0 && n >= maxMatch);
    if (reach) {
        const int f = __ffsll((long long)reach) - 1;
        const int nf = __builtin_amdgcn_readlane(n, f);
        if (nf == maxMatch && lane > f) n = 0;
    }
    // first longest candidate: the longest length, and among equals the lowest lane
    const u32 best = wave_max(lane <= (int)RX_POS_MASK ? ((u32)n << 8) | (RX_POS_MASK - (u32)lane) : 0u);
    const int bestLen = (int)(best >> 8), bestIdx = (int)(RX_POS_MASK - (best & 0xFF));
    const u32 next = (counter + 1) & RX_POS_MASK;
    if (lane == 0) { counters[key] = (u8)next; row[next] = hash32 | pos; }
    wave_fence();
    return bestLen < minMatch ? -1 : (bestIdx << 16) | (bestLen - minMatch);
}

__global__ __launch_bounds__(64) void k_rolzx_forward(XfStage st, u8* __restrict__ scratch, int first)
{
    const int b = first + (int)blockIdx.x;
    const int lane = lane_id();
    const u32 count = st.len[b];
    if (count == 0) return;
    const u8* __restrict__ src = st.src[b];
    u8* __restrict__ dst = st.dst[b];
    const RxTables t = rx_tables(scratch, (int)blockIdx.x);
    __shared__ u32 lds[RX_KEYS / 4];
    u8* counters = reinterpret_cast<u8*>(lds);
    u32 ok = 0, d = 0;
    if (count >= RX_MIN_BLOCK && count <= RX_MAX_BLOCK && st.cap[b] >= rx_max_encoded(count)) {
        // ---- the data type (:927-947): the context's, or detectSimpleType's verdict on the whole block, which is written back
        int dt = st.dtype ? (int)st.dtype[b] : DT_UNDEFINED;
        if (dt == DT_UNDEFINED) {
            for (int i = lane; i < 256; i += 64) lds[i] = 0;
            __syncthreads();
            const u32 bulk = count & ~7u;
            for (u32 i = 8u * (u32)lane; i < bulk; i += 512) {
                const u64 w = ldg_u<u64>(src + i);
#pragma unroll
                for (int k = 0; k < 8; k++) atomicAdd(&lds[(u32)(w >> (8 * k)) & 255], 1u);
            }
            if ((u32)lane < count - bulk) atomicAdd(&lds[ldg<u8>(src + bulk + lane)], 1u);
            __syncthreads();
            dt = pk_simple_type(count, lds);
            __syncthreads();
            if (dt != DT_UNDEFINED && st.dtype && lane == 0) st.dtype[b] = (u8)dt;
        }
        u32 delta = 2, flags = 0;
        int minMatch = 3;
        if (dt == DT_EXE) { delta = 3; flags = 8; }
        else if (dt == DT_DNA) { delta = 8; minMatch = 7; flags = 4; }
        for (int i = lane; i < (int)(RX_KEYS / 4); i += 64) lds[i] = 0;
        __syncthreads();
        if (lane == 0) { st_u<u32>(dst, bswap32(count)); dst[4] = (u8)flags; }
        RxEnc e;
        e.low = 0; e.high = RX_TOP; e.idx = 5; e.lim = count; e.full = 0; e.buf = dst;
        const u32 srcEnd = count - 4;
        u32 sizeChunk = count < RX_CHUNK ? count : RX_CHUNK, startChunk = 0, srcIdx = 0;
        const u8* s = src;
        while (startChunk < srcEnd && !e.full) {
            rx_chunk_reset(t, lane);
            const u32 endChunk = startChunk + sizeChunk < srcEnd ? startChunk + sizeChunk : srcEnd;
            sizeChunk = endChunk - startChunk;
            s = src + startChunk;
            srcIdx = 0;
            const u32 n = srcEnd - startChunk < 8u ? srcEnd - startChunk : 8u;
            for (u32 j = 0; j < n && !e.full; j++, srcIdx++) rx_encode<9>(e, t.lit, 0x100u | ldg<u8>(s + srcIdx), lane);
            while (srcIdx < sizeChunk && !e.full) {
                const u64 w = ldg_u<u64>(s + srcIdx - 8);                             // (srcIdx >= 8 here)
                const u32 prev = (u32)(w >> 56);
                const int match = rx_find_match(t, counters, s, srcIdx, sizeChunk, rx_key(w, delta), minMatch, lane);
                if (match < 0) {
                    rx_encode<9>(e, t.lit + (prev << 9), 0x100u | ldg<u8>(s + srcIdx), lane);
                    srcIdx++;
                    continue;
                }
                rx_encode<9>(e, t.lit + (prev << 9), (u32)match & 0xFFFF, lane);
                rx_encode<RX_LOG_POS>(e, t.idx + (prev << RX_LOG_POS), (u32)match >> 16, lane);
                srcIdx += ((u32)match & 0xFFFF) + (u32)minMatch;
            }
            startChunk = endChunk;
        }
        for (int i = 0; i < 4 && !e.full; i++, srcIdx++)                            // the last literals: no reset, the chunk's contexts
            rx_encode<9>(e, t.lit + ((u32)ldg<u8>(s + srcIdx - 1) << 9), 0x100u | ldg<u8>(s + srcIdx), lane);
        if (!e.full && e.idx + 8 < count) {                                         // dispose(); the result is dstIdx < count
            if (lane == 0) st_u<u64>(dst + e.idx, __builtin_bswap64(e.low));
            d = e.idx + 8;
            ok = 1;
        }
    }
    if (lane == 0) { st.ok[b] = (u8)ok; st.newLen[b] = ok ? d : 0u; }
}

// ---- ROLZDecoder ---------------------------------------------------------------------------------
// The decoder's state is the same in every lane. The 2^NB probabilities of a context's tree are one row (1 KiB for a literal or a
// length, 64 bytes for an index): lane L loads entries 8L .. 8L + 7 with one 16-byte load, the NB dependent steps then pick theirs with
// a register select and one readlane, the owning lane updates its copy, and the lanes that changed store theirs back: one round
// trip to the tables per token instead of one per bit. Entry k of a row is always lane k / 8's, so no lane reads what another stored.
struct RxDec { u64 low, high, cur; u32 idx, count, err; const u8* buf; };

template <int NB>
__device__ __forceinline__ u32 rx_decode(RxDec& r, u16* probs, int lane)
{
    uint4 mine = make_uint4(0, 0, 0, 0);
    const bool holds = lane < (1 << NB) / 8;
    if (holds) mine = *reinterpret_cast<const uint4*>(probs + 8 * lane);
    bool dirty = false;
    u32 c1 = 1;
#pragma unroll
    for (int i = 0; i < NB; i++) {
        const u32 sub = c1 & 7;
        const int owner = (int)(c1 >> 3);
        const u32 word = (sub & 4) ? ((sub & 2) ? mine.w : mine.z) : ((sub & 2) ? mine.y : mine.x);
        const u32 p = rl((word >> (16 * (sub & 1))) & 0xFFFF, owner);
        const u64 mid = r.low + ((((r.high - r.low) >> 4) * (u64)(p >> 4)) >> 8);
        u32 np;
        if (mid >= r.cur) { r.high = mid; np = (u32)((int)p - (((int)p - 0xFFFF + 32) >> 5)) & 0xFFFF; c1 += c1 + 1; }
        else { r.low = mid + 1; np = (u32)((int)p - (int)(p >> 5)) & 0xFFFF; c1 += c1; }
        if (lane == owner) {
            const u32 sh = 16 * (sub & 1);
            const u32 nw = (word & ~(0xFFFFu << sh)) | (np << sh);
            if (sub & 4) { if (sub & 2) mine.w = nw; else mine.z = nw; }
            else { if (sub & 2) mine.y = nw; else mine.x = nw; }
            dirty = true;
        }
        while (((r.low ^ r.high) >> 24) == 0) {
            if (r.idx + 4 > r.count) { r.err = 1; break; }                         // 4 bytes that do not lie inside `count`: refused
            r.low = (r.low << 32) & RX_TOP;
            r.high = ((r.high << 32) | 0xFFFFFFFFull) & RX_TOP;
            r.cur = ((r.cur << 32) | (u64)bswap32(ldg_u<u32>(r.buf + r.idx))) & RX_TOP;
            r.idx += 4;
        }
        if (r.err) break;
    }
    if (dirty) *reinterpret_cast<uint4*>(probs + 8 * lane) = mine;
    return c1 & ((1u << NB) - 1);
}

__global__ __launch_bounds__(64) void k_rolzx_inverse(XfStage st, u8* __restrict__ scratch, int first)
{
    const int b = first + (int)blockIdx.x;
    const int lane = lane_id();
    const u32 count = st.len[b];
    if (count == 0) return;
    const u8* __restrict__ src = st.src[b];
    u8* dst = st.dst[b];
    const RxTables t = rx_tables(scratch, (int)blockIdx.x);
    __shared__ u32 lds[RX_KEYS / 4];
    u8* counters = reinterpret_cast<u8*>(lds);
    for (int i = lane; i < (int)(RX_KEYS / 4); i += 64) lds[i] = 0;
    __syncthreads();
    u32 ok = 0, out = 0;
    const u32 dstEnd = count >= 5 ? bswap32(ldg_u<u32>(src)) : 0u;
    if (count >= 13 && count <= RX_MAX_BLOCK && dstEnd != 0 && dstEnd <= 0x7FFFFFFFu && dstEnd <= st.cap[b]) {
        const u32 flags = ldg<u8>(src + 4);
        u32 delta = 2, minMatch = 3;
        if ((flags & 0x0E) == 8) delta = 3;
        else if ((flags & 0x0E) == 4) { delta = 8; minMatch = 7; }
        RxDec r;
        r.low = 0; r.high = RX_TOP; r.cur = __builtin_bswap64(ldg_u<u64>(src + 5)); r.idx = 13; r.count = count; r.err = 0; r.buf = src;
        u32 sizeChunk = dstEnd < RX_CHUNK ? dstEnd : RX_CHUNK, startChunk = 0;
        ok = 1;
        while (startChunk < dstEnd && ok) {
            rx_chunk_reset(t, lane);
            const u32 endChunk = startChunk + sizeChunk < dstEnd ? startChunk + sizeChunk : dstEnd;
            sizeChunk = endChunk - startChunk;
            u8* o = dst + out;                                                     // (output._index: it leaves startChunk behind when a copy crosses a chunk's end)
            const u32 room = dstEnd - out;                                         // bytes of the block from o on
            u32 dstIdx = 0;
            // ---- first literals. Control flow is the same in every lane throughout; lane 0 writes the bytes and keeps the tables
            const u32 n = room < 8u ? room : 8u;
            for (u32 j = 0; j < n; j++) {
                const u32 val = rx_decode<9>(r, t.lit, lane);
                if (r.err || (val >> 8) == 0) { ok = 0; break; }
                if (lane == 0) o[dstIdx] = (u8)val;
                dstIdx++;
            }
            // w: the 8 bytes in front of dstIdx. Behind a literal they are shifted in registers (reading back the byte lane 0 has just
            // stored would put a store and a load into every step of the chain); behind a copy, and at the start, they are loaded.
            u64 w = 0;
            bool haveW = false;
            while (ok && dstIdx < sizeChunk) {
                if (dstIdx >= room) { ok = 0; break; }                             // (the reference would write behind the block)
                const u32 savedIdx = dstIdx;
                if (!haveW) {
                    wave_fence();                                               // the bytes lane 0 stored, the copy
                    w = ldg_u<u64>(o + dstIdx - 8);                                   // (dstIdx >= 8, or bytes of the chunk before)
                    haveW = true;
                }
                const u32 key = rx_key(w, delta);
                const u32 prev = (u32)(w >> 56);
                u32* row = t.matches + ((size_t)key << RX_LOG_POS);
                const u32 val = rx_decode<9>(r, t.lit + (prev << 9), lane);
                if (r.err) { ok = 0; break; }
                if (val >> 8) {
                    if (lane == 0) o[dstIdx] = (u8)val;
                    dstIdx++;
                    w = (w >> 8) | ((u64)(val & 0xFF) << 56);
                } else {
                    const u32 matchLen = val & 0xFF;
                    if (dstIdx + matchLen + 3 > dstEnd) { ok = 0; break; }                         // the reference's sanity check (:1086)
                    if (dstIdx + matchLen + minMatch > room) { ok = 0; break; }                    // (the reference would write behind the block)
                    const u32 matchIdx = rx_decode<RX_LOG_POS>(r, t.idx + (prev << RX_LOG_POS), lane);
                    if (r.err) { ok = 0; break; }
                    wave_fence();                                               // the ring and counter entries, and the literals, lane 0 stored
                    const u32 ref = row[((u32)counters[key] - matchIdx) & RX_POS_MASK];
                    const u32 len = matchLen + minMatch;
                    // emitCopy: a byte-exact overlapping copy (ref < dstIdx: a position the decoder stored, or 0)
                    const u32 dist = dstIdx - ref;
                    if (dist >= len) {
                        const u32 bulk = len & ~7u;
                        for (u32 i = 8u * (u32)lane; i < bulk; i += 512) st_u<u64>(o + dstIdx + i, ldg_u<u64>(o + ref + i));
                        if ((u32)lane < len - bulk) o[dstIdx + bulk + lane] = o[ref + bulk + lane];
                    } else {
                        for (u32 i = (u32)lane; i < len; i += 64) o[dstIdx + i] = o[ref + i % dist];
                    }
                    dstIdx += len;
                    haveW = false;
                    wave_fence();                                               // every lane has read the ring before lane 0 stores into it
                }
                if (lane == 0) {
                    const u32 c = (u32)counters[key] + 1;
                    counters[key] = (u8)c;
                    row[c & RX_POS_MASK] = savedIdx;
                }
            }
            startChunk = endChunk;
            out += dstIdx;
        }
        if (ok && r.idx != count) ok = 0;
    }
    if (lane == 0) { st.ok[b] = (u8)ok; st.newLen[b] = ok ? out : 0u; }
}

// KNZ_ROLZX_TABLES_MAX=bytes: what the tables of the blocks that run at once may take (default 4 GiB, 495 blocks: about two waves per
// CU, which is what the 64 KiB of LDS per wave allows). A larger batch runs in slices of as many blocks as fit, at least one.
size_t rx_budget()
{
    const char* e = getenv("KNZ_ROLZX_TABLES_MAX");
    const long long v = e ? atoll(e) : 0;
    return v > 0 ? (size_t)v : ((size_t)4 << 30);
}

int rx_slice_blocks(int nBlocks)
{
    const size_t fit = rx_budget() / RX_BLOCK_BYTES;
    return (int)(fit < 1 ? 1 : fit > (size_t)nBlocks ? (size_t)nBlocks : fit);
}

}  // namespace

size_t rolzx_scratch_bytes(int nBlocks, u32 /*maxLen*/) { return nBlocks <= 0 ? 0 : (size_t)rx_slice_blocks(nBlocks) * RX_BLOCK_BYTES; }

void launch_rolzx_forward(hipStream_t s, const XfStage& st, void* scratch)
{
    if (st.nBlocks <= 0) return;
    const int per = rx_slice_blocks(st.nBlocks);
    KScope ks_("k_rolzx_forward");
    for (int b0 = 0; b0 < st.nBlocks; b0 += per)
        hipLaunchKernelGGL(k_rolzx_forward, dim3(st.nBlocks - b0 < per ? st.nBlocks - b0 : per), dim3(64), 0, s, st, static_cast<u8*>(scratch), b0);
}

void launch_rolzx_inverse(hipStream_t s, const XfStage& st, void* scratch)
{
    if (st.nBlocks <= 0) return;
    const int per = rx_slice_blocks(st.nBlocks);
    KScope ks_("k_rolzx_inverse");
    for (int b0 = 0; b0 < st.nBlocks; b0 += per)
        hipLaunchKernelGGL(k_rolzx_inverse, dim3(st.nBlocks - b0 < per ? st.nBlocks - b0 : per), dim3(64), 0, s, st, static_cast<u8*>(scratch), b0);
}

}  // namespace knz
