// The wave-cooperative bit copy and the block header's length rule, shared by the assembly kernels (bitasm.hip) and the many-stream
// framing (streams.hip).
#pragma once
#include "common.hpp"

namespace knz {

// ---------------------------------------------------------------- wave-cooperative bit copy
// Copies nbits (MSB-first from src[0]) to bit position dstBit of the big-endian word stream dst.
__device__ inline void wave_copy_bits(u32* __restrict__ dst, u64 dstBit, const u8* __restrict__ src, u64 nbits)
{
    if (nbits == 0) return;
    const int lane = lane_id();
    const u64 w0 = dstBit >> 5;
    const u64 w1 = (dstBit + nbits - 1) >> 5;
    const u64 srcBytes = (nbits + 7) >> 3;
    for (u64 w = w0 + lane; w <= w1; w += 64) {
        const u64 wb = w << 5;
        const u64 lo = wb > dstBit ? wb : dstBit;
        const u64 hiEnd = dstBit + nbits;
        const u64 hi = (wb + 32) < hiEnd ? (wb + 32) : hiEnd;
        const u32 nb = (u32)(hi - lo);
        const u64 s = lo - dstBit;
        const u64 b0 = s >> 3;
        const u32 sh = (u32)(s & 7);
        // 40 source bits starting at byte b0 (big-endian): one (unaligned) dword + one byte when they are inside
        // the piece, single bytes only at its tail
        u64 win = 0;
        if (b0 + 5 <= srcBytes) {
            u32 x;
            __builtin_memcpy(&x, src + b0, 4);
            win = ((u64)bswap32(x) << 8) | (u64)src[b0 + 4];
        } else {
#pragma unroll
            for (int i = 0; i < 5; i++) {
                const u64 idx = b0 + i;
                const u64 v = idx < srcBytes ? (u64)src[idx] : 0ull;
                win |= v << (32 - 8 * i);
            }
        }
        const u32 val = (u32)((win >> (40 - sh - nb)) & (nb == 32 ? 0xFFFFFFFFull : ((1ull << nb) - 1)));
        const u32 word = val << (u32)((wb + 32) - hi);
        if (nb == 32) dst[w] = bswap32(word);
        else if (word) atomicOr(&dst[w], bswap32(word));
    }
}

// ---------------------------------------------------------------- framing helpers
// Block header bits: mode byte (+ skip byte when > 4 transforms) + length + checksum
// (io/CompressedOutputStream.cpp:757-807)
__device__ __forceinline__ u32 block_data_size(u32 postLen)
{
    return (postLen < 256) ? 1u : (u32)(ilog2_u32(postLen) >> 3) + 1u;
}

// One step of the block walk (io/CompressedInputStream.cpp:823-856, :875-919): the 5-bit / lw-bit length prefix at `pos` and, for a block,
// its mode byte, length and checksum. WALK_BLOCK: db is filled and pos stands behind the block; WALK_END: the end marker, pos behind it;
// WALK_ERROR: `error` holds the code. Nothing at or behind src.limitBits is read.
enum { WALK_BLOCK = 0, WALK_END = 1, WALK_ERROR = 2 };
__device__ inline int walk_step(const BitSrc& src, u64& pos, int checksumBits, u32 blockSize, DecBlock& db, int& error)
{
    int err = 0;
    const u32 lr = 3 + take_bits(src, pos, 5, err);
    if (err) { error = KNZ_ERR_READ_FILE; return WALK_ERROR; }
    u64 len = 0;
    if (lr > 32) { len = (u64)take_bits(src, pos, lr - 32, err) << 32; len |= take_bits(src, pos, 32, err); }
    else len = take_bits(src, pos, lr, err);
    if (err) { error = KNZ_ERR_READ_FILE; return WALK_ERROR; }
    if (len == 0) return WALK_END;
    if (len > (1ull << 34)) { error = KNZ_ERR_BLOCK_SIZE; return WALK_ERROR; }
    if (pos + len > src.limitBits) { error = KNZ_ERR_READ_FILE; return WALK_ERROR; }
    db.payloadBit = pos; db.bits = len; db.error = 0; db.usedBits = 0; db.checksum = 0;
    u64 p = pos;
    BitSrc bs = src;
    bs.limitBits = pos + len;
    int e2 = 0;
    const u32 mode = take_bits(bs, p, 8, e2);
    db.copyBlock = (mode & 0x80) ? 1u : 0u;
    if (db.copyBlock) db.skipFlags = 0xFF;
    else if (mode & 0x10) db.skipFlags = take_bits(bs, p, 8, e2);
    else db.skipFlags = ((mode << 4) | 0x0F) & 0xFF;
    const u32 ds = 1 + ((mode >> 5) & 3);
    db.preLen = take_bits(bs, p, 8 * ds, e2);
    const u32 blkLen = (blockSize + 512 > blockSize + (blockSize >> 4)) ? blockSize + 512 : blockSize + (blockSize >> 4);
    u32 mts = blkLen + blkLen / 2;
    if (mts < 2048) mts = 2048;
    if (mts > (1u << 30)) mts = 1u << 30;
    if (e2 || db.preLen == 0 || db.preLen > mts) db.error = KNZ_ERR_READ_FILE;
    if (checksumBits == 32) db.checksum = take_bits(bs, p, 32, e2);
    else if (checksumBits == 64) { db.checksum = (u64)take_bits(bs, p, 32, e2) << 32; db.checksum |= take_bits(bs, p, 32, e2); }
    if (e2 && !db.error) db.error = KNZ_ERR_PROCESS_BLOCK;
    db.entropyBit = p;
    pos += len;
    return WALK_BLOCK;
}

}  // namespace knz
