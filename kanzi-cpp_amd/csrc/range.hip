// Range coder (kanzi "RANGE", entropy id 4) on gfx950.
//
// Reference being replaced (bit-identical streams): entropy/RangeEncoder.cpp:67-127 (updateFrequencies, encodeHeader), :130-192
// (encode, encodeByte), entropy/RangeDecoder.cpp:66-146 (decodeHeader), :150-224 (decode, decodeByte), entropy/EntropyUtils.cpp:57-123
// (alphabet), :131-245 (normalizeFrequencies). A block is coded in chunks of 32,768 bytes. Per chunk: the alphabet, 3 bits of lr - 8
// (lr = 12, lowered to 8 while 2^lr exceeds the chunk), the frequencies of all symbols but the first in groups of 6 or 8 behind a 4-bit
// width, then a carry-less range coder on 60-bit low / range in wrapping 64-bit arithmetic that leaves 28 bits whenever the top 28 bits
// of low and low + range agree -- or, when they differ and range has fallen to 16 bits, after cutting range back to the next 2^16
// border -- and 60 bits of low at the end. Chunks with one symbol are a header and nothing else.
// The reference's decoder takes no bitstream version: versions 3-5 read the same chunks.
//
// Mapping:
//   k_range_stats   one wave per chunk: the histogram / normalizeFrequencies / alphabet + group code of the order-0 rANS statistics
//                   kernel (ans_common.hpp) with the log range as a run-time value, and (cumulative, frequency) pairs for the encoder.
//   k_range_encode  The recurrence is serial inside a chunk and chunks are independent: one LANE per chunk, 16 chunks per wave. A
//                   step is an LDS read of the symbol's pair, two 64-bit multiplies and the renormalisation, whose trip count differs
//                   between lanes; with 16 lanes a wave waits for the slowest of 16, not of 64, 212 MB are 406 waves (one or less
//                   per SIMD of the device) instead of 102, and the tables of a wave are 16 KiB of LDS. The chunk's bytes are read 16
//                   at a time one interval ahead; emissions go through a 64-word LDS ring per chunk and leave as 64-byte stores by
//                   four lanes per chunk. The payload of a chunk is 28 k + 60 bits: one bit-granular piece of its ChunkDesc.
//   k_range_decode  The format has no chunk directory and no chunk length: where chunk k + 1 starts is known once chunk k is decoded.
//                   One wave per block, chunk after chunk: the whole wave parses the header and rebuilds the tables in LDS (slot ->
//                   symbol bytes, at most 32 KiB for lr 15; (cumulative, frequency) pairs), then every lane runs the same recurrence
//                   on wave-uniform values: the payload comes from a 128-word register window (one word per lane, loaded 64 words
//                   ahead), the quotient from a reciprocal estimate (range_div), the bytes of a 256-byte tile are collected one word
//                   per lane in a register and stored as words.
#include "common.hpp"
#include "stages.hpp"
#include "ans_common.hpp"

namespace knz {

constexpr u64 RANGE_TOP = 0x0FFFFFFFFFFFFFFFull;
constexpr u64 RANGE_BOTTOM = 0xFFFFull;
constexpr u64 RANGE_MASK = 0x0FFFFFFF00000000ull;
constexpr int RCH = 16;                  // chunks per encoder wave


// ------------------------------------------------------------------------------------------------
// statistics + header
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void k_range_stats(BlockView view, const u32* __restrict__ origLen, u32 copyThreshold, int maxChunks,
                                                    ChunkDesc* __restrict__ desc, u32* __restrict__ cumFreq, u8* __restrict__ tmp)
{
    const int slot = blockIdx.x;
    const int b = slot / maxChunks;
    const int ci = slot - b * maxChunks;
    const u32 len = view.len[b];
    const u32 start = (u32)ci * RANGE_CHUNK;
    if (start >= len) return;
    const int lane = lane_id();
    const u8* blk = view.ptr[b] + start;
    ChunkDesc* cd = desc + slot;
    if (origLen[b] <= copyThreshold) {
        // copy block: entropy type forced to NONE (io/CompressedOutputStream.cpp:691-695)
        if (lane == 0) desc_raw(cd, blk, 8 * len);
        return;
    }
    const u32 n = (len - start < RANGE_CHUNK) ? (len - start) : RANGE_CHUNK;
    u32 lr = 12;                                                  // RangeEncoder.cpp:143-147
    while (lr > 8 && (1u << lr) > n) lr--;

    __shared__ u32 hist[8][264];
    __shared__ u32 hdrw[HDR_WORDS];
    __shared__ u32 grpMax[64];
    __shared__ u32 grpOff[64];
    for (int i = lane; i < 8 * 264; i += 64) (&hist[0][0])[i] = 0;
    for (int i = lane; i < (int)HDR_WORDS; i += 64) hdrw[i] = 0;
    grpMax[lane] = 0;
    __syncthreads();

    u32 f[4];                                                     // lane owns symbols 4*lane .. 4*lane+3
    chunk_counts(lane, blk, n, hist, f);
    const Alphabet al = alphabet_of(f);
    const u32 present = al.present, asz = al.asz, rankBase = al.rankBase;

    if (n != (1u << lr)) ans_normalize_lr(lane, f, n, asz, lr);
    const u32 pos = ans_header_bits_lr(lane, f, present, asz, rankBase, 2, lr, hdrw, grpMax, grpOff, 0);
    __syncthreads();

    header_flush(lane, hdrw, pos, tmp + (size_t)slot * RANGE_STRIDE);

    // A frequency that does not fit 16 bits: the normalisation's last line wrapped below zero (EntropyUtils.cpp:243; a short chunk at a low
    // log range whose many rare symbols were raised to 1). Nobody can read such a chunk, the reference included, but it writes one, with
    // 64-bit products and unmasked fields: k_range_encode_wide and range_wide_spill (common.hpp) write the same bits.
    int wk = -1;
#pragma unroll
    for (int k = 0; k < 4; k++) if (f[k] > 0xFFFFu) wk = k;
    const bool wide = asz > 1 && __ballot(wk >= 0) != 0;
    if (wide && wk >= 0) {
        // position and value of the log size of this symbol's group, when it does not fit its 4 bits
        const u32 r = rankBase + (u32)__popc(present & ((1u << wk) - 1u));
        const u32 chk = (asz >= 64) ? 8u : 6u, nGroups = (asz - 1 + chk - 1) / chk;
        cd->mid[0] = 0xFFFFFFFFu; cd->mid[1] = 0;
        if (r >= 1 && grpMax[(r - 1) / chk] >= 16) {
            const u32 last = nGroups - 1, cntLast = asz - (1 + last * chk);
            const u32 groupsBits = grpOff[last] + 4 + cntLast * grpMax[last];
            cd->mid[0] = pos - groupsBits + grpOff[(r - 1) / chk];
            cd->mid[1] = grpMax[(r - 1) / chk];
        }
    }
    if (asz > 1) {
        // cumulative frequencies in symbol order (RangeEncoder.cpp:71-77), as the normalisation left them (wide: the frequencies alone)
        const u32 lsum = f[0] + f[1] + f[2] + f[3];
        const u32 lincl = wave_incl_scan(lsum);
        u32 cum = lincl - lsum;
        u32* out = cumFreq + (size_t)slot * 256;
#pragma unroll
        for (int k = 0; k < 4; k++) { out[4 * lane + k] = wide ? f[k] : (cum | (f[k] << 16)); cum += f[k]; }
    }
    if (lane == 0) {
        cd->hdrBits = pos; cd->midLen = 0; cd->trailerLen = 0; cd->nPieces = 0; cd->aux = asz | (lr << 16) | (wide ? 0x80000000u : 0u);
    }
}

// ------------------------------------------------------------------------------------------------
// encode: one lane per chunk, 16 chunks per wave
// ------------------------------------------------------------------------------------------------
// Renormalisation (RangeEncoder.cpp:178-191, RangeDecoder.cpp:208-221) never takes more than two turns, which is why the kernels run
// it as a loop of two: a unit leaves in the first form only while range < 2^32 (above that the top 28 bits of low and low + range
// differ) and multiplies range by 2^28; the second form leaves range = v * 2^28 with v in [1, 0xFFFF], which is above 0xFFFF. After a
// byte range is at least 2 (range >> lr >= 2 since range > 0xFFFF before it and lr <= 15; every frequency is at least 1), so after
// one unit of the first form it is at least 2^29 and cannot take the second form; after a unit of the second form one of the first
// may follow and leaves range >= 2^56; after two units of the first form range >= 2^57. In every case the third test ends the loop.
//
// Most units a chunk of n bytes can leave -- RANGE_MAX_UNITS(n) = n + n / 64 + 2, which sizes the chunk's staging region (stages.hpp):
// let P = log2(range). P starts at log2(2^60 - 1) and never exceeds 60. A byte lowers it by at most lr + log2(16 / 15) <= 12.094:
// range >= 2^16 when the byte starts, so floor(range / 2^lr) >= (range / 2^lr) * 15 / 16 with lr <= 12, and the frequency is at least
// 1. A unit of the first form raises P by exactly 28; one of the second form takes range from at most 0xFFFF (P < 16) to at least
// 2^28, more than 12. The sum of all rises is the sum of all falls plus P(end) - P(start) <= 12.094 n, so there are at most
// 12.094 n / 12 < n + n / 128 + 1 units.
__global__ __launch_bounds__(64) void k_range_encode(BlockView view, int maxChunks, int nSlots, ChunkDesc* __restrict__ desc,
                                                     const u32* __restrict__ cumFreq, u8* __restrict__ tmp)
{
    __shared__ u32 tab[RCH][257];                    // cumulative | frequency << 16; odd row stride: the chunks' rows start in different banks
    __shared__ u32 ringw[RCH][64];                   // 64 staged words per chunk
    const int lane = lane_id();
    const int slotBase = blockIdx.x * RCH;

    bool act = false;
    u32 n = 0, lr = 8;
    const u8* blk = nullptr;
    if (lane < RCH && slotBase + lane < nSlots) {
        const int slot = slotBase + lane;
        const int b = slot / maxChunks;
        const int ci = slot - b * maxChunks;
        const u32 len = view.len[b];
        const u32 start = (u32)ci * RANGE_CHUNK;
        if (start < len) {
            const u32 aux = desc[slot].aux;
            if ((aux & 0xFFFF) > 1 && !(aux >> 31)) {   // (0: raw copy block; 1: one symbol, the header is all; bit 31: k_range_encode_wide)
                act = true;
                lr = aux >> 16;
                n = (len - start < RANGE_CHUNK) ? (len - start) : RANGE_CHUNK;
                blk = view.ptr[b] + start;
            }
        }
    }
    const u64 actMask = __ballot(act);
    if (actMask == 0) return;
    for (int g = 0; g < RCH; g++) {
        if (!((actMask >> g) & 1)) continue;
        const u32* src = cumFreq + (size_t)(slotBase + g) * 256;
#pragma unroll
        for (int k = 0; k < 4; k++) tab[g][lane + 64 * k] = src[lane + 64 * k];
    }
    __syncthreads();

    const u32* mytab = tab[lane & (RCH - 1)];
    u32* ring = ringw[lane & (RCH - 1)];
    u64 low = 0, range = RANGE_TOP, acc = 0;
    u32 nacc = 0;                                    // bits waiting in acc (below 32)
    u32 wc = 0, fl = 0;                              // words produced / words already in global memory (a multiple of 16)
    auto emit = [&](u32 v, u32 nb) {
        acc = (acc << nb) | v;
        nacc += nb;
        if (nacc >= 32) { nacc -= 32; ring[wc & 63] = bswap32((u32)(acc >> nacc)); wc++; }
    };
    const bool aligned = ((reinterpret_cast<uintptr_t>(blk) & 15) == 0);
    auto load16 = [&](u32 k, u32 r[4]) {
        const u32 base = 16 * k;
        if (act && aligned && base + 16 <= n) {
            const uint4 v = *reinterpret_cast<const uint4*>(blk + base);
            r[0] = v.x; r[1] = v.y; r[2] = v.z; r[3] = v.w;
        } else {
#pragma unroll
            for (int c = 0; c < 4; c++) {
                u32 w = 0;
                for (u32 t = 0; t < 4; t++) { const u32 i = base + 4 * (u32)c + t; if (act && i < n) w |= (u32)blk[i] << (8 * t); }
                r[c] = w;
            }
        }
    };
    // the four lanes 4c .. 4c+3 move 16 finished words of chunk c from its ring to its payload area
    u8* payC = tmp + (size_t)(slotBase + (lane >> 2)) * RANGE_STRIDE + HDR_BYTES;
    auto flush16 = [&]() {
        const u32 wcC = (u32)__shfl((int)wc, lane >> 2, 64), flC = (u32)__shfl((int)fl, lane >> 2, 64);
        if (wcC - flC >= 16) {
            const u32 off = flC + 4 * ((u32)lane & 3);
            const u32* rp = &ringw[lane >> 2][off & 63];
            *reinterpret_cast<uint4*>(payC + 4 * (size_t)off) = make_uint4(rp[0], rp[1], rp[2], rp[3]);
        }
        if (wc - fl >= 16) fl += 16;
    };

    const u32 maxN = wave_max(n);
    u32 cur[4], nxt[4];
    load16(0, cur);
    for (u32 k = 0; 16 * k < maxN; k++) {
        load16(k + 1, nxt);
#pragma unroll
        for (int u = 0; u < 16; u++) {
            if (act && 16 * k + (u32)u < n) {
                const u32 e = mytab[(cur[u >> 2] >> (8 * (u & 3))) & 0xFF];
                range >>= lr;
                low += (u64)(e & 0xFFFF) * range;
                range *= (u64)(e >> 16);
                for (int it = 0; it < 2; it++) {
                    if (((low ^ (low + range)) & RANGE_MASK) != 0) {
                        if (range > RANGE_BOTTOM) break;
                        range = (0 - low) & RANGE_BOTTOM;              // ~(low - 1) & 0xFFFF
                    }
                    emit((u32)(low >> 32) & 0x0FFFFFFFu, 28);
                    range <<= 28;
                    low <<= 28;
                }
            }
        }
        // an interval leaves at most 32 units = 28 words; at most 15 were left behind: two rounds of 16 keep the ring below 64 words
        KNZ_WAVE_ORDER();
        flush16();
        flush16();
#pragma unroll
        for (int c = 0; c < 4; c++) cur[c] = nxt[c];
    }
    if (act) {
        emit((u32)(low >> 32) & 0x0FFFFFFFu, 28);                       // 60 bits of low
        emit((u32)low, 32);
        u32* pay = reinterpret_cast<u32*>(tmp + (size_t)(slotBase + lane) * RANGE_STRIDE + HDR_BYTES);
        for (u32 w = fl; w < wc; w++) pay[w] = ring[w & 63];
        if (nacc) pay[wc] = bswap32((u32)(acc << (32 - nacc)));
        ChunkDesc* cd = desc + slotBase + lane;
        cd->nPieces = 1; cd->pieceBits[0] = 32 * wc + nacc; cd->piecePtr[0] = reinterpret_cast<const u8*>(pay);
    }
}

// A chunk with a wide frequency (k_range_stats), one lane per chunk: RangeEncoder::encodeByte as it stands, in 64-bit cumulative
// frequencies and products that wrap. The payload staging holds the units as the bit stream will (the top four bits of every value
// masked off), those top bits per write at RANGE_WIDE_NIB for range_wide_spill, and the cumulative table. The renormalisation loop
// has no bound of two turns here (a product may wrap to a range of 0, on which the reference never ends): it stops at RANGE_WIDE_UNITS.
constexpr u32 RANGE_WIDE_UNITS = (RANGE_WIDE_NIB * 8 - 64) / 28;
constexpr u32 RANGE_WIDE_CUM = 2 * RANGE_WIDE_NIB;
static_assert(RANGE_WIDE_UNITS + 1 <= RANGE_WIDE_NIB && RANGE_WIDE_CUM + 257 * 8 <= RANGE_PAY_BYTES && (HDR_BYTES + RANGE_WIDE_CUM) % 8 == 0, "wide staging");
__global__ __launch_bounds__(64) void k_range_encode_wide(BlockView view, int maxChunks, int nSlots, ChunkDesc* __restrict__ desc,
                                                          const u32* __restrict__ cumFreq, u8* __restrict__ tmp)
{
    const int slot = (int)(blockIdx.x * 64 + threadIdx.x);
    if (slot >= nSlots) return;
    const int b = slot / maxChunks;
    const int ci = slot - b * maxChunks;
    const u32 len = view.len[b];
    const u32 start = (u32)ci * RANGE_CHUNK;
    if (start >= len) return;
    ChunkDesc* cd = desc + slot;
    const u32 aux = cd->aux;
    if (!(aux >> 31)) return;
    const u32 lr = (aux >> 16) & 0xFF;
    const u32 n = (len - start < RANGE_CHUNK) ? (len - start) : RANGE_CHUNK;
    const u8* blk = view.ptr[b] + start;
    u8* pay = tmp + (size_t)slot * RANGE_STRIDE + HDR_BYTES;
    u32* payw = reinterpret_cast<u32*>(pay);
    u8* nib = pay + RANGE_WIDE_NIB;
    u64* cum = reinterpret_cast<u64*>(pay + RANGE_WIDE_CUM);
    const u32* fr = cumFreq + (size_t)slot * 256;
    u64 c = 0;
    for (int i = 0; i < 256; i++) { cum[i] = c; c += fr[i]; }
    cum[256] = c;
    u64 low = 0, range = RANGE_TOP, acc = 0;
    u32 nacc = 0, wc = 0, units = 0;
    auto emit = [&](u32 v, u32 nb) {
        acc = (acc << nb) | v;
        nacc += nb;
        if (nacc >= 32) { nacc -= 32; payw[wc++] = bswap32((u32)(acc >> nacc)); }
    };
    for (u32 i = 0; i < n && units < RANGE_WIDE_UNITS; i++) {
        const u64 cf = cum[blk[i]], fq = cum[(u32)blk[i] + 1] - cf;
        range >>= lr;
        low += cf * range;
        range *= fq;
        while (units < RANGE_WIDE_UNITS) {
            if (((low ^ (low + range)) & RANGE_MASK) != 0) {
                if (range > RANGE_BOTTOM) break;
                range = (0 - low) & RANGE_BOTTOM;
            }
            emit((u32)(low >> 32) & 0x0FFFFFFFu, 28);
            nib[units++] = (u8)(low >> 60);
            range <<= 28;
            low <<= 28;
        }
    }
    emit((u32)(low >> 32) & 0x0FFFFFFFu, 28);                           // 60 bits of low
    emit((u32)low, 32);
    nib[units] = (u8)(low >> 60);
    if (nacc) payw[wc] = bswap32((u32)(acc << (32 - nacc)));
    cd->mid[2] = units;
    cd->nPieces = 1; cd->pieceBits[0] = 28 * units + 60; cd->piecePtr[0] = pay;
}

// ------------------------------------------------------------------------------------------------
// decode: one wave per block
// ------------------------------------------------------------------------------------------------
// floor(d / r) for r >= 1 and d < r * 2^15 (the decoder has checked d < r << lr) without a 64-bit division. With x = d / r < 2^15: the
// conversions of d and r round to nearest (relative error 2^-24 each), the reciprocal is within one unit in the last place (2^-23),
// the product rounds once more (2^-24), so the estimate is x (1 + e) with |e| < 2^-22 and differs from x by less than 2^-7: its
// integer part is q - 1, q or q + 1. Then d - est * r lies in [-r, 2 r) -- |est * r| <= d + r < 2^61, no overflow -- and one
// comparison on either side settles it.
__device__ __forceinline__ u32 range_div(u64 d, u64 r)
{
#ifdef KNZ_EMU
    const float inv = 1.0f / (float)r;
#else
    const float inv = __builtin_amdgcn_rcpf((float)r);
#endif
    u32 q = (u32)((float)d * inv);
    const int64_t rem = (int64_t)(d - (u64)q * r);
    if (rem < 0) q--;
    else if ((u64)rem >= r) q++;
    return q;
}

__global__ void k_range_div_probe(const u64* __restrict__ d, const u64* __restrict__ r, u32 n, u32* __restrict__ q)
{
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) q[i] = range_div(d[i], r[i]);
}

__global__ __launch_bounds__(64) void k_range_decode(BitSrc src, DecBlock* __restrict__ blocks, u8* const* __restrict__ outPtr, int framing)
{
    __shared__ u32 f2sw[8192];                       // slot -> symbol, one byte each (2^lr <= 32,768 slots)
    __shared__ u32 cf[256];                          // cumulative | frequency << 16
    __shared__ u32 cumS[260];
    __shared__ u32 grpPos[64], grpW[64];
    const int b = blockIdx.x;
    const int lane = lane_id();
    DecBlock& db = blocks[b];
    if (db.error) return;
    BitSrc s = src;
    {
        const u64 end = db.payloadBit + ((db.bits + 7) & ~7ull);
        s.limitBits = end < src.limitBits ? end : src.limitBits;      // never past the caller's in_bits
    }
    const u64 limit = s.limitBits;
    u64 pos = db.entropyBit;
    const u32 count = db.preLen;
    u8* block = outPtr[b];
    if (db.copyBlock) {
        const bool bad = pos + 8ull * count > limit;
        if (!bad) for (u32 i = (u32)lane; i < count; i += 64) block[i] = (u8)peek_bits(s, pos + 8ull * i, 8);
        if (lane == 0) { if (bad) db.error = KNZ_ERR_PROCESS_BLOCK; db.usedBits = bad ? (limit - db.entropyBit) : 8ull * count; }
        return;
    }
    const ClampedWords cw = clamped_words(src);
    const bool wordStores = ((reinterpret_cast<uintptr_t>(block) & 3) == 0);
    const u8* f2s = reinterpret_cast<const u8*>(f2sw);
    u32 start = 0;
    bool fail = false, ended = false;
    while (start < count && !fail) {
        const u32 n = (RANGE_CHUNK < count - start) ? RANGE_CHUNK : count - start;
        // ---- alphabet (EntropyUtils.cpp:91-123): lane owns symbols 4*lane .. 4*lane+3, the nibble (lane & 1) of mask byte lane >> 1
        if (pos + 2 > limit) { fail = true; break; }
        const u32 hb = peek_bits(s, pos, 7);
        if ((hb >> 6) != 0 && pos + 6 + 8ull * (((hb >> 1) & 31) + 1) > limit) { fail = true; break; }     // the mask bytes
        const auto fetch = [&](u64 at, u32 nb) { return peek_bits(s, at, nb); };
        const AlphabetIn<u64> ai = alphabet_get(fetch, lane, pos);
        pos = ai.next;
        const u32 asz = ai.a.asz;
        if (asz == 0) { ended = true; break; }                       // RangeDecoder.cpp:163-164: the count so far
        if (pos + 3 > limit) { fail = true; break; }
        const u32 lr = 8 + peek_bits(s, pos, 3);
        pos += 3;
        const u32 scale = 1u << lr;
        if (asz == 1) {
            const u32 sym = ai.firstSym;
            for (u32 i = (u32)lane; i < n; i += 64) block[start + i] = (u8)sym;
            start += n;
            continue;
        }
        // ---- every check of the header before the chunk's first byte (RangeDecoder.cpp:87-124)
        const u32 chk = (asz >= 64) ? 8u : 6u;
        const u32 nGroups = (asz - 1 + chk - 1) / chk;                // at most 43
        const u32 lastCnt = (asz - 1) - (nGroups - 1) * chk;
        u32 q = 0;                                                    // bit offset from pos
        for (u32 g = 0; g < nGroups; g++) {
            if (pos + q + 4 > limit) { fail = true; break; }
            const u32 w = peek_bits(s, pos + q, 4);                   // llr = 4 for every lr from 8 to 15
            if ((1u << w) > scale) { fail = true; break; }
            if ((u32)lane == g) { grpPos[g] = q + 4; grpW[g] = w; }
            q += 4 + ((g + 1 == nGroups) ? lastCnt : chk) * w;
        }
        if (fail || pos + q > limit) { fail = true; break; }
        __syncthreads();
        u32 f[4];
        if (freqs_get(ai.a, scale, [&](u32 g, u32& w) -> u64 { w = grpW[g]; return pos + grpPos[g]; }, fetch, f)) { fail = true; break; }
        {
            const u32 lsum = f[0] + f[1] + f[2] + f[3];
            const u32 lincl = wave_incl_scan(lsum);
            u32 cum = lincl - lsum;
#pragma unroll
            for (int k = 0; k < 4; k++) { cf[4 * lane + k] = cum | (f[k] << 16); cumS[4 * lane + k] = cum; cum += f[k]; }
            if (lane == 63) cumS[256] = scale;
        }
        __syncthreads();
        // slot p belongs to the last symbol whose cumulative frequency is <= p (symbols of frequency 0 share theirs with the next one)
        for (u32 p4 = (u32)lane; p4 < (scale >> 2); p4 += 64) {
            u32 word = 0;
#pragma unroll
            for (u32 t = 0; t < 4; t++) {
                const u32 p = 4 * p4 + t;
                u32 lo = 0;
#pragma unroll
                for (u32 step = 128; step; step >>= 1) if (cumS[lo + step] <= p) lo += step;
                word |= lo << (8 * t);
            }
            f2sw[p4] = word;
        }
        __syncthreads();
        pos += q;

        // ---- the recurrence (RangeDecoder.cpp:173-224), the same in every lane
        if (pos + 60 > limit) { fail = true; break; }
        u64 code = ((u64)peek_bits(s, pos, 28) << 32) | peek_bits(s, pos + 28, 32);
        pos += 60;
        u64 low = 0, range = RANGE_TOP;
        // payload words from word wbase on, one per lane: winCur = words [winBase, +64), winNext the 64 behind them
        const u64 wbase = pos >> 5;
        auto loadWin = [&](u32 w0) -> u32 {
            return bswap32(cw.raw(wbase + w0 + (u32)lane));
        };
        u32 winBase = 0;
        u32 winCur = loadWin(0), winNext = loadWin(64);
        for (u32 i0 = 0; i0 < n && !fail; i0 += 256) {
            const u32 nb = (n - i0 < 256) ? n - i0 : 256;
            u32 myWord = 0;
            for (u32 l = 0; l < nb; l++) {
                range >>= lr;
                if (range == 0) { fail = true; break; }
                const u64 d = code - low;
                if (d >= (range << lr)) { fail = true; break; }       // cum >= 2^lr
                const u32 cum = range_div(d, range);
                const u32 sym = f2s[cum];
                const u32 e = cf[sym];
                low += (u64)(e & 0xFFFF) * range;
                range *= (u64)(e >> 16);
                for (int it = 0; it < 2; it++) {                      // (two turns at most: see k_range_encode)
                    if (((low ^ (low + range)) & RANGE_MASK) != 0) {
                        if (range > RANGE_BOTTOM) break;
                        range = (0 - low) & RANGE_BOTTOM;
                    }
                    if (pos + 28 > limit) { fail = true; break; }
                    const u32 wi = (u32)((pos >> 5) - wbase);
                    if (wi - winBase >= 64) { winCur = winNext; winBase += 64; winNext = loadWin(winBase + 64); }
                    const u32 i = wi - winBase;
                    const u32 a = rl(winCur, i);
                    const u32 c = (i + 1 < 64) ? rl(winCur, (i + 1) & 63) : rl(winNext, 0);
                    const u32 unit = (u32)(((((u64)a << 32) | c) << (pos & 31)) >> 36);
                    pos += 28;
                    code = (code << 28) | unit;
                    range <<= 28;
                    low <<= 28;
                }
                if (fail) break;
                if ((u32)lane == (l >> 2)) myWord |= sym << (8 * (l & 3));
            }
            if (fail) break;
            // (the window loads are issued before the stores: a load behind a store would wait for it)
            u8* dst = block + start + i0;
            if (wordStores && 4 * (u32)lane + 4 <= nb) *reinterpret_cast<u32*>(dst + 4 * lane) = myWord;
            else for (u32 t = 0; t < 4; t++) if (4 * (u32)lane + t < nb) dst[4 * lane + t] = (u8)(myWord >> (8 * t));
        }
        start += n;
    }
    if (lane == 0) {
        if (fail || (ended && framing)) db.error = KNZ_ERR_PROCESS_BLOCK;
        else if (ended) db.preLen = start;                            // per-stage call: EntropyDecoder::decode's return value
        db.usedBits = pos - db.entropyBit;
    }
}

void launch_range_encode(hipStream_t s, BlockView view, const u32* origLen, u32 copyThreshold, int nBlocks, int maxChunks, ChunkDesc* desc,
                         u32* cumFreq, u8* tmp)
{
    const int nSlots = nBlocks * maxChunks;
    { KScope ks_("k_range_stats"); hipLaunchKernelGGL(k_range_stats, dim3(nSlots), dim3(64), 0, s, view, origLen, copyThreshold, maxChunks, desc, cumFreq, tmp); }
    { KScope ks_("k_range_encode"); hipLaunchKernelGGL(k_range_encode, dim3((nSlots + RCH - 1) / RCH), dim3(64), 0, s, view, maxChunks, nSlots, desc, cumFreq, tmp); }
    { KScope ks_("k_range_encode_wide"); hipLaunchKernelGGL(k_range_encode_wide, dim3((nSlots + 63) / 64), dim3(64), 0, s, view, maxChunks, nSlots, desc, cumFreq, tmp); }
}

void launch_range_decode(hipStream_t s, BitSrc src, DecBlock* blocks, int nBlocks, u8* const* outPtr, int framing)
{
    { KScope ks_("k_range_decode"); hipLaunchKernelGGL(k_range_decode, dim3(nBlocks), dim3(64), 0, s, src, blocks, outPtr, framing); }
}

void launch_range_div_probe(hipStream_t s, const u64* d, const u64* r, u32 n, u32* q)
{
    hipLaunchKernelGGL(k_range_div_probe, dim3((n + 255) / 256), dim3(256), 0, s, d, r, n, q);
}

}  // namespace knz
