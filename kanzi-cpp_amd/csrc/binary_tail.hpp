// What a chunk of the two binary arithmetic coders (FPAQ, CM) adds to its block's bit stream: var-int payload byte count, the payload
// (one piece of the staging buffer), 56 bits of low | 0xFFFFFF.
#pragma once
#include "common.hpp"

namespace knz {

__device__ __forceinline__ void binary_desc_finish(ChunkDesc& cd, u32 index, const u8* buf, u64 low)
{
    cd.hdrBits = 0; cd.aux = 0;
    u8 mid[8];
    u32 ml = 0;
    u32 v = index;
    while (v >= 128) { mid[ml++] = (u8)(0x80 | (v & 0x7F)); v >>= 7; }
    mid[ml++] = (u8)v;
    u32 mw[6] = { 0, 0, 0, 0, 0, 0 };
    for (u32 i = 0; i < ml; i++) mw[i >> 2] |= (u32)mid[i] << (8 * (i & 3));
    for (int i = 0; i < 6; i++) cd.mid[i] = mw[i];
    cd.midLen = ml;
    cd.nPieces = index ? 1 : 0;
    cd.pieceBits[0] = 8 * index;
    cd.piecePtr[0] = buf;
    // 56 bits of low | 0xFFFFFF after every chunk; the last one is written by dispose() (FPAQEncoder.cpp:92-110, BinaryEntropyEncoder.cpp:114-128)
    const u64 tail = (low | 0x0000000000FFFFFFull) & 0x00FFFFFFFFFFFFFFull;
    u32 tw[2] = { 0, 0 };
    for (int k = 0; k < 7; k++) { const u32 byte = (u32)((tail >> (48 - 8 * k)) & 0xFF); tw[k >> 2] |= byte << (8 * (k & 3)); }
    cd.trailer[0] = tw[0]; cd.trailer[1] = tw[1];
    cd.trailerLen = 7;
}

}  // namespace knz
