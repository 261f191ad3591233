// What the coders behind BinaryEntropyEncoder / BinaryEntropyDecoder share (CM in cm.hip, TPAQ and TPAQX in tpaq.hip): the chunk rule,
// the 56-bit interval chain of one wave per block, the payload as 32-bit units (written through a ring in LDS, read as pre-shifted
// units one per lane), the chunk tail (binary_tail.hpp) and the two-tier staging. Only the predictor differs: a type P with
//   u32 get()            the split, a 12-bit probability of a 1, wave-uniform
//   void update(bool)    the coded bit, wave-uniform
// Reference: entropy/BinaryEntropyEncoder.cpp:75-139, BinaryEntropyEncoder.hpp:68-78 (encodeBit), entropy/BinaryEntropyDecoder.cpp:74-139,
// BinaryEntropyDecoder.hpp:68-89 (decodeBit).
//
// Format: a block of `count` bytes is coded in chunks of max(count, 64) bytes -- one chunk -- unless that is CM_BIG_BLOCK (64 MiB) or
// more: then a chunk is count >> 3 bytes, or count >> 4 when count / 8 is itself CM_BIG_BLOCK or more (8-9 or 16-17 chunks). A chunk
// is: var-int payload byte count, payload, 56 bits of low | 0xFFFFFF. Predictor and interval carry across chunks. The decoder reads
// the var-int, 56 bits into `current`, then the payload.
#pragma once
#include "common.hpp"
#include "binary_tail.hpp"
#include "ent_header.hpp"

namespace knz {

#ifdef KNZ_EMU_CM_BIG_BLOCK        // CPU emulation tests only: a low threshold, to cross chunk borders with small inputs
constexpr u32 CM_BIG_BLOCK = KNZ_EMU_CM_BIG_BLOCK;
#else
constexpr u32 CM_BIG_BLOCK = 1u << 26;
#endif
static_assert(CM_BIG_BLOCK >= 256, "a big block has at least 16 bytes per chunk");
constexpr u64 CM_TOP = 0x00FFFFFFFFFFFFFFull;
constexpr u64 CM_MASK32 = 0x00000000FFFFFFFFull;
constexpr u64 CM_MASK56 = 0x00FFFFFFFFFFFFFFull;
constexpr u32 CM_RING_WORDS = 512;            // a tile of 64 bytes is 512 bits, a bit leaves at most one word

__host__ __device__ __forceinline__ u32 cm_chunk_len(u32 count)
{
    u32 length = count < 64 ? 64u : count;
    if (length >= CM_BIG_BLOCK) length = (length / 8 < CM_BIG_BLOCK) ? count >> 3 : count >> 4;
    return length;
}

// The first staging of a block of n bytes. div != 0 (tests only, cm_tier1_div): n / div + 64 bytes, so that the second pass is taken.
__host__ __device__ __forceinline__ u64 cm_stage1(u64 n, u32 div)
{
    return div ? n / div + 64 : n + n / 8 + 64;
}

// A copy block: entropy type forced to NONE (io/CompressedOutputStream.cpp:691-695)
__device__ __forceinline__ void binary_copy_desc(ChunkDesc& cd, const u8* blk, u32 count)
{
    cd.hdrBits = 0; cd.midLen = 0; cd.trailerLen = 0; cd.aux = 0;
    cd.nPieces = 1; cd.pieceBits[0] = 8 * count; cd.piecePtr[0] = blk;
}

// The encoder of one block by one wave: `count` bytes at blk into buf (capacity cap), one ChunkDesc per chunk. Returns true when the
// staging was too small (nothing of the block is valid then). ring: CM_RING_WORDS words of LDS.
template <class P>
__device__ __forceinline__ bool binary_encode_block(P& pr, const u8* __restrict__ blk, u32 count, u8* __restrict__ buf, u64 cap, ChunkDesc* cds,
                                                    u32* ring, int lane)
{
    const u32 length = cm_chunk_len(count);
    u64 low = 0, high = CM_TOP;
    u64 index = 0;                                  // bytes of the block's staging in use; a chunk's payload starts where the last one ended
    u32 startChunk = 0;
    int ci = 0;
    bool full = false;
    while (startChunk < count && !full) {
        const u32 chunkSize = (length < count - startChunk) ? length : count - startChunk;
        const u32 endChunk = startChunk + chunkSize;
        const u64 index0 = index;
        u32 nByte = 0;
        { const u32 i = startChunk + (u32)lane; if (i < endChunk) nByte = blk[i]; }
        for (u32 i0 = startChunk; i0 < endChunk && !full; i0 += 64) {
            const u32 byte = nByte;
            { const u32 i = i0 + 64 + (u32)lane; nByte = 0; if (i < endChunk) nByte = blk[i]; }
            const u32 nb = (endChunk - i0 < 64) ? endChunk - i0 : 64;
            u32 cnt = 0;
            for (u32 l = 0; l < nb && !full; l++) {
                const u32 bv = rl(byte, l);
#pragma unroll
                for (int k = 0; k < 8; k++) {
                    const u64 pred = pr.get();
                    const bool one = (bv >> (7 - k)) & 1u;
                    const u64 mid = low + ((((high - low) >> 4) * pred) >> 8);
                    high = one ? mid : high;
                    low = one ? low : mid + 1;
                    pr.update(one);
                    const u64 x = low ^ high;
                    if ((((u32)(x >> 32)) | ((u32)x >> 24)) == 0) {  // top 32 of the 56 bits agree: they leave
                        if (index + 4ull * cnt + 4 > cap) { full = true; break; }
                        if (lane == 0) ring[cnt] = (u32)(high >> 24);
                        cnt++;
                        low <<= 32;
                        high = (high << 32) | CM_MASK32;
                    }
                }
            }
            __syncthreads();
            if (!full) for (u32 qd = (u32)lane; qd < cnt; qd += 64) reinterpret_cast<u32*>(buf + index)[qd] = bswap32(ring[qd]);
            __syncthreads();
            index += 4ull * cnt;
        }
        if (!full && lane == 0) binary_desc_finish(cds[ci], (u32)(index - index0), buf + index0, low);
        startChunk = endChunk;
        ci++;
    }
    return full;
}

// The decoder of one block by one wave: `count` bytes to `block` from bit `pos` of s (limit: s.limitBits). Returns true on failure.
template <class P>
__device__ __forceinline__ bool binary_decode_block(P& pr, const BitSrc& src, const BitSrc& s, u64& pos, u32 count, u8* __restrict__ block, int lane)
{
    const u64 limit = s.limitBits;
    const ClampedWords cw = clamped_words(src);
    const u32 length = cm_chunk_len(count);
    u64 low = 0, high = CM_TOP, current = 0;
    u32 startChunk = 0;
    bool fail = false;
    while (startChunk < count && !fail) {
        const u32 chunkSize = (length < count - startChunk) ? length : count - startChunk;
        const u32 endChunk = startChunk + chunkSize;
        int err = 0;
        const u32 szBytes = take_varint(s, pos, err);
        if (err) { fail = true; break; }
        {
            const u64 most = ((u64)chunkSize << 5) < 0x1FFFFFFFull ? ((u64)chunkSize << 5) : 0x1FFFFFFFull;      // BinaryEntropyDecoder.cpp:98-101
            if (szBytes > most) { fail = true; break; }
        }
        current = ((u64)take_bits(s, pos, 24, err) << 32) | take_bits(s, pos, 32, err);
        if (err || pos + 8ull * szBytes > limit) { fail = true; pos = limit; break; }
        const u64 payBit = pos;
        pos += 8ull * szBytes;
        // payload as 32-bit units in stream order, unit u = bits [payBit + 32 u, + 32): window = 64 units, one per lane
        const u64 wbase = payBit >> 5;
        const u32 sh = (u32)(payBit & 31);
        auto loadWin = [&](u32 unit0) -> u32 {
            const u64 w = wbase + unit0 + (u32)lane;
            const u32 a = bswap32(cw.raw(w)), c = bswap32(cw.raw(w + 1));
            return sh ? ((a << sh) | (c >> (32 - sh))) : a;
        };
        u32 winBase = 0;
        u32 winCur = loadWin(0), winNext = loadWin(64);
        u32 index = 0;
        for (u32 i0 = startChunk; i0 < endChunk && !fail; i0 += 64) {
            const u32 nb = (endChunk - i0 < 64) ? endChunk - i0 : 64;
            u32 myByte = 0;
            for (u32 l = 0; l < nb; l++) {
                u32 val8 = 0;
#pragma unroll
                for (int k = 0; k < 8; k++) {
                    const u64 pred = pr.get();
                    const u64 split = ((((high - low) >> 4) * pred) >> 8) + low;
                    const bool one = split >= current;
                    high = one ? split : high;
                    low = one ? low : split + 1;
                    pr.update(one);
                    val8 = 2 * val8 + (one ? 1u : 0u);
                    const u64 x = low ^ high;
                    if ((((u32)(x >> 32)) | ((u32)x >> 24)) == 0) {
                        low = (low << 32) & CM_MASK56;
                        high = ((high << 32) | CM_MASK32) & CM_MASK56;
                        if (index + 4 > szBytes) {
                            // the reference would read behind its payload here: no stream it writes does that
                            current = (current << 32) & CM_MASK56;
                            index = szBytes + 1;
                        } else {
                            const u32 u = index >> 2;
                            if (u - winBase >= 64) { winCur = winNext; winBase += 64; winNext = loadWin(winBase + 64); }
                            const u64 val = rl(winCur, (u - winBase) & 63);
                            current = ((current << 32) | val) & CM_MASK56;
                            index += 4;
                        }
                    }
                }
                if ((u32)lane == l) myByte = val8;
                if (index > szBytes) { fail = true; break; }
            }
            if ((u32)lane < nb && !fail) block[i0 + (u32)lane] = (u8)myByte;
        }
        startChunk = endChunk;
    }
    return fail;
}

// The head of a decoder kernel: the block's bit window, and copy blocks. Returns true when the block is done (copied or refused).
__device__ __forceinline__ bool binary_decode_head(const BitSrc& src, DecBlock& db, BitSrc& s, u8* __restrict__ block, int lane)
{
    if (db.error) return true;
    s = src;
    {
        const u64 end = db.payloadBit + ((db.bits + 7) & ~7ull);
        s.limitBits = end < src.limitBits ? end : src.limitBits;      // never past the caller's in_bits
    }
    if (!db.copyBlock) return false;
    const u64 limit = s.limitBits;
    const u64 pos = db.entropyBit;
    const u32 count = db.preLen;
    const bool bad = pos + 8ull * count > limit;
    if (!bad) for (u32 i = (u32)lane; i < count; i += 64) block[i] = (u8)peek_bits(s, pos + 8ull * i, 8);
    if (lane == 0) { if (bad) db.error = KNZ_ERR_PROCESS_BLOCK; db.usedBits = bad ? (limit - db.entropyBit) : 8ull * count; }
    return true;
}

}  // namespace knz
