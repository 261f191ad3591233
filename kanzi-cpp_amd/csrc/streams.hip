// Framing of a batch that holds many independent streams (knz_hip_encode_streams / knz_hip_decode_streams).
//
// The stage kernels take ragged batches as they are; what assumes ONE stream is the framing around them: k_block_scan and
// k_walk_blocks of bitasm.hip each run on one thread, because one stream has tens of blocks. A batch of thousands of small streams has
// thousands of blocks, and every stream starts a bit count of its own:
//   k_stream_frame   per block hdrBits / written / lw in parallel, a 64-bit scan over the blocks that restarts at every stream's
//                    prologue, a scan over the streams' byte lengths (each rounded up to 16) for the stream bases
//   k_stream_prologues   one wave per stream copies its prologue to the stream's base
//   k_walk_count / k_walk_scan / k_walk_fill   one lane per stream walks its length prefixes, the counts are scanned, a second walk
//                    writes the DecBlock entries at the stream's first slot
// The bit offsets of a 2 GiB batch do not fit 32 bits, so the scans here are 64-bit (wave_incl_scan64), not those of prims.hpp.
#include "common.hpp"
#include "stages.hpp"
#include "bitcopy.hpp"

namespace knz {

constexpr int SF_THREADS = 1024;            // one workgroup scans the batch: 64 tiles for the most blocks a call takes

// Exclusive 64-bit sum over the workgroup's threads in thread order, on top of `carry` (LDS, the running total of the tiles before;
// updated). Every thread of the workgroup calls it.
__device__ __forceinline__ u64 wg_excl_scan64(u64 v, u64* waveTot, u64* carry)
{
    const u64 incl = wave_incl_scan64(v);
    const int wv = (int)(threadIdx.x >> 6);
    if (lane_id() == 63) waveTot[wv] = incl;
    __syncthreads();
    u64 off = *carry;
    for (int k = 0; k < wv; k++) off += waveTot[k];
    __syncthreads();
    if (threadIdx.x == blockDim.x - 1) *carry = off + incl;
    __syncthreads();
    return off + incl - v;
}

// info[b].payloadBits is set (k_block_sum). Leaves hdrBits, written, lw and the absolute bitOff of every block, the streams' places in
// res and the bytes of output in use in *totalBytes. excl: nBlocks + 1 words of scratch. One workgroup of SF_THREADS threads.
__global__ __launch_bounds__(SF_THREADS) void k_stream_frame(BlockInfo* __restrict__ info, const u32* __restrict__ blockLen, const u32* __restrict__ origLen,
                                                             const u32* __restrict__ itemOf, int nBlocks, const StreamEnc* __restrict__ st, int nItems,
                                                             FrameParams fp, u64* __restrict__ excl, StreamOut* __restrict__ res, u64* __restrict__ totalBytes)
{
    __shared__ u64 waveTot[SF_THREADS / 64];
    __shared__ u64 carry;
    if (threadIdx.x == 0) carry = 0;
    __syncthreads();
    // 1. the blocks' framing fields, and every block's bit position as if the batch were one stream without prologue
    for (int base = 0; base < nBlocks; base += SF_THREADS) {
        const int b = base + (int)threadIdx.x;
        u64 v = 0;
        if (b < nBlocks) {
            const u32 ds = block_data_size(blockLen[b]);
            // (more than four transforms: the skip flags get a byte of their own, except in copy blocks; io/CompressedOutputStream.cpp:791-799)
            const u32 skipByte = (fp.nTransforms > 4 && origLen[b] > 15) ? 8u : 0u;
            const u32 hdrBits = 8u + skipByte + 8u * ds + (u32)fp.checksumBits;
            const u64 written = (u64)hdrBits + info[b].payloadBits;
            const u32 lw = (written < 8) ? 3u : (u32)ilog2_u32((u32)(written >> 3)) + 4u;
            info[b].hdrBits = hdrBits;
            info[b].written = written;
            info[b].lw = lw;
            v = 5u + lw + written;
        }
        const u64 e = wg_excl_scan64(v, waveTot, &carry);
        if (b < nBlocks) excl[b] = e;
    }
    if (threadIdx.x == 0) { excl[nBlocks] = carry; carry = 0; }
    __threadfence_block();
    __syncthreads();
    // 2. the streams: prologue + blocks + end marker, in bytes rounded up to 16, one behind the other
    for (int base = 0; base < nItems; base += SF_THREADS) {
        const int i = base + (int)threadIdx.x;
        u64 bits = 0, bytes = 0;
        if (i < nItems) {
            bits = (u64)st[i].prologueBits + (excl[st[i + 1].first] - excl[st[i].first]) + (fp.finish ? 8u : 0u);
            bytes = (((bits + 7) >> 3) + 15) & ~15ull;
        }
        const u64 at = wg_excl_scan64(bytes, waveTot, &carry);
        if (i < nItems) { res[i].base = at; res[i].bits = bits; }
    }
    if (threadIdx.x == 0) *totalBytes = carry;
    __threadfence_block();
    __syncthreads();
    // 3. the blocks' places: the scan of step 1 restarted at the stream's first block, behind the stream's prologue
    for (int b = (int)threadIdx.x; b < nBlocks; b += SF_THREADS) {
        const u32 i = itemOf[b];
        info[b].bitOff = 8ull * res[i].base + st[i].prologueBits + (excl[b] - excl[st[i].first]);
    }
}

__global__ __launch_bounds__(64) void k_stream_prologues(u32* __restrict__ out, const StreamEnc* __restrict__ st, const StreamOut* __restrict__ res,
                                                         const u8* __restrict__ prologues)
{
    const int i = blockIdx.x;
    wave_copy_bits(out, 8ull * res[i].base, prologues + st[i].prologueOff, st[i].prologueBits);
}

// ---------------------------------------------------------------- decode side
__device__ __forceinline__ BitSrc stream_src(const u8* in, const StreamDec& sd)
{
    BitSrc src;
    src.words = reinterpret_cast<const u32*>(in + sd.inOff);      // (inOff is a multiple of 16)
    src.nBytes = (sd.inBits + 7) >> 3;
    src.nWords = src.nBytes >> 2;
    src.limitBits = sd.inBits;
    return src;
}

// One lane per stream: the length prefixes from the stream's start bit up to the end marker, the stream's own bit limit or the most
// blocks its room can take (room / blockSize + 2, as a single-stream call bounds its walk). Nothing behind the stream's bits is read.
// The verdicts are those of a single-stream call: damaged framing is the walk's error, blocks beyond the room KNZ_ERR_WRITE_FILE;
// a stream with a verdict contributes no block.
__global__ __launch_bounds__(64) void k_walk_count(const u8* __restrict__ in, const StreamDec* __restrict__ sd, int nItems, int checksumBits, u32 blockSize,
                                                   StreamWalk* __restrict__ res)
{
    const int i = blockIdx.x * 64 + (int)threadIdx.x;
    if (i >= nItems) return;
    const StreamDec d = sd[i];
    const BitSrc src = stream_src(in, d);
    const u64 most = d.outCap / blockSize + 2;
    u64 pos = d.startBit, nb = 0;
    int error = 0, ended = 0;
    while (nb < most) {
        DecBlock db;
        const int r = walk_step(src, pos, checksumBits, blockSize, db, error);
        if (r == WALK_END) { ended = 1; break; }
        if (r == WALK_ERROR) break;
        nb++;
    }
    if (!error && nb * blockSize > d.outCap + blockSize) error = KNZ_ERR_WRITE_FILE;
    StreamWalk w;
    w.first = 0; w.count = error ? 0u : (u32)nb; w.error = error; w.ended = ended;
    res[i] = w;
}

// res[i].first = blocks of the streams before i; res[nItems].first = all blocks. One workgroup of SF_THREADS threads.
__global__ __launch_bounds__(SF_THREADS) void k_walk_scan(StreamWalk* __restrict__ res, int nItems)
{
    __shared__ u64 waveTot[SF_THREADS / 64];
    __shared__ u64 carry;
    if (threadIdx.x == 0) carry = 0;
    __syncthreads();
    for (int base = 0; base < nItems; base += SF_THREADS) {
        const int i = base + (int)threadIdx.x;
        const u64 e = wg_excl_scan64(i < nItems ? (u64)res[i].count : 0ull, waveTot, &carry);
        if (i < nItems) res[i].first = e;
    }
    if (threadIdx.x == 0) { res[nItems].first = carry; res[nItems].count = 0; res[nItems].error = 0; res[nItems].ended = 0; }
}

// The second walk: stream i's blocks at blocks[first ..], their bit positions counted from the start of the whole input, and every
// block's place and room in the output (block k of a stream lies k block sizes behind the stream's place).
__global__ __launch_bounds__(64) void k_walk_fill(const u8* __restrict__ in, const StreamDec* __restrict__ sd, int nItems, int checksumBits, u32 blockSize,
                                                  const StreamWalk* __restrict__ res, DecBlock* __restrict__ blocks, u64* __restrict__ outOff, u64* __restrict__ room)
{
    const int i = blockIdx.x * 64 + (int)threadIdx.x;
    if (i >= nItems) return;
    const StreamDec d = sd[i];
    const BitSrc src = stream_src(in, d);
    const u64 first = res[i].first;
    const u32 count = res[i].count;
    u64 pos = d.startBit;
    int error = 0;
    for (u32 k = 0; k < count; k++) {
        DecBlock db;
        if (walk_step(src, pos, checksumBits, blockSize, db, error) != WALK_BLOCK) return;      // (cannot happen: the first walk counted them)
        db.payloadBit += 8ull * d.inOff;
        db.entropyBit += 8ull * d.inOff;
        blocks[first + k] = db;
        const u64 at = (u64)k * blockSize;
        outOff[first + k] = d.outOff + at;
        room[first + k] = d.outCap > at ? d.outCap - at : 0;
    }
}

void launch_stream_frame(hipStream_t s, BlockInfo* info, const u32* blockLen, const u32* origLen, const u32* itemOf, int nBlocks, const StreamEnc* st, int nItems,
                         FrameParams fp, u64* excl, StreamOut* res, u64* totalBytes)
{
    { KScope ks_("k_stream_frame"); hipLaunchKernelGGL(k_stream_frame, dim3(1), dim3(SF_THREADS), 0, s, info, blockLen, origLen, itemOf, nBlocks, st, nItems, fp, excl, res, totalBytes); }
}

void launch_stream_prologues(hipStream_t s, u32* out, const StreamEnc* st, const StreamOut* res, int nItems, const u8* prologues)
{
    if (nItems == 0) return;
    { KScope ks_("k_stream_prologues"); hipLaunchKernelGGL(k_stream_prologues, dim3(nItems), dim3(64), 0, s, out, st, res, prologues); }
}

void launch_walk_streams_count(hipStream_t s, const u8* in, const StreamDec* sd, int nItems, int checksumBits, u32 blockSize, StreamWalk* res)
{
    if (nItems) { KScope ks_("k_walk_count"); hipLaunchKernelGGL(k_walk_count, dim3((nItems + 63) / 64), dim3(64), 0, s, in, sd, nItems, checksumBits, blockSize, res); }
    { KScope ks_("k_walk_scan"); hipLaunchKernelGGL(k_walk_scan, dim3(1), dim3(SF_THREADS), 0, s, res, nItems); }
}

void launch_walk_streams_fill(hipStream_t s, const u8* in, const StreamDec* sd, int nItems, int checksumBits, u32 blockSize, const StreamWalk* res,
                              DecBlock* blocks, u64* outOff, u64* room)
{
    if (nItems == 0) return;
    { KScope ks_("k_walk_fill"); hipLaunchKernelGGL(k_walk_fill, dim3((nItems + 63) / 64), dim3(64), 0, s, in, sd, nItems, checksumBits, blockSize, res, blocks, outOff, room); }
}

}  // namespace knz
