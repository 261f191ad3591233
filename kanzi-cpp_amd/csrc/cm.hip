// CM on gfx950 (kanzi "CM", entropy id 6): the binary arithmetic coder of FPAQ behind a context-mixing predictor.
//
// Reference being replaced (bit-identical streams): entropy/CMPredictor.hpp:55-87 (update / get), CMPredictor.cpp:27-53 (tables),
// entropy/BinaryEntropyEncoder.cpp:75-139, BinaryEntropyEncoder.hpp:68-78 (encodeBit), entropy/BinaryEntropyDecoder.cpp:74-139,
// BinaryEntropyDecoder.hpp:68-89 (decodeBit). Every stream path of the reference builds the predictor with a Context of bitstream
// version 6, so counter2[*][16] starts at 65536; the 65535 of version 7 and up is not built here (api.hip refuses that version).
//
// The coder itself -- chunk rule, interval chain, payload units, chunk tail -- is binary_coder.hpp, shared with tpaq.hip; this file is the
// predictor, the two kernels that instantiate the coder with it, and the staging protocol's host side.
//
// Format: a block of `count` bytes is coded in chunks of max(count, 64) bytes -- one chunk -- unless that is CM_BIG_BLOCK (64 MiB) or
// more: then a chunk is count >> 3 bytes, or count >> 4 when count / 8 is itself CM_BIG_BLOCK or more (8-9 or 16-17 chunks). A chunk
// is: var-int payload byte count, payload, 56 bits of low | 0xFFFFFF. Predictor and interval carry across chunks. The decoder reads
// the var-int, 56 bits into `current`, then the payload.
//
// Predictor state, in LDS (CmTables, 150,016 bytes: ONE workgroup per compute unit, the batch queues behind that):
//   counter1[256][257] as 16-bit cells. A cell starts at 32768 and never exceeds 65,520: a 0 bit takes p to p - (p >> r), which is not
//   above p and not below 0; a 1 bit takes p to p - ((p - 65536 + 16) >> r) = p + ceil((65520 - p) / 2^r) for p < 65520 (arithmetic
//   shift of a negative number), and ceil(d / 2^r) <= d for d >= 1, so the result is at most 65520; at p = 65520 the step is 0.
//   counter2[512][17]: cells 0-15 start at j << 12 <= 61440 and obey the same rule: 16 bits. Cell 16 starts at 65536 and needs 17 bits
//   until its first 0 bit (after that it obeys the rule as well): it is kept apart as 32-bit words (c2top).
//   get() reads counter1[ctx][256], [ctx][c1], [ctx][c2]; their mix p <= 65520 picks counter2[ctx | runMask][p >> 12] and its right
//   neighbour (p >> 12 <= 15, so the neighbour is at most cell 16).
//
// Encoder shape that was built: the PLAIN one, one wave per block (k_cm_encode): predictor and interval in one wave-uniform chain.
// The split into eight predictor waves (one per tree level: the levels touch disjoint rows of both tables) in front of an interval
// wave, the shape of k_fpaq_encode, is not built yet.
// Decoder: one wave per block (k_cm_decode); the next context is the decoded bit, the format allows nothing else. Payload as
// pre-shifted 32-bit units one per lane, readable from any start bit, as in k_fpaq_decode.
//
// Staging: nobody has derived a tighter bound on what CM can emit than the format's own (a bit leaves at most one 32-bit unit: 32 bytes
// per input byte), so none is assumed: a block is staged at cm_stage1(n, 0) = n + n / 8 + 64 bytes (the reference's first buffer size),
// the capacity is checked before every 32-bit flush, a block that would overflow is marked, and the marked blocks are coded again
// from scratch into a staging of 32 n + 16 bytes each that launch_cm_encode_again asks its caller for (readbacks and stream
// synchronisations: the rare path). The count of marked blocks is the first word of the control area; the caller reads it back with
// what it reads back anyway, so the common path has no synchronisation of its own.
#include "common.hpp"
#include "stages.hpp"
#include "binary_coder.hpp"

#include <stdlib.h>
#include <vector>

namespace knz {

struct CmTables {
    u16 c1[256 * 257];
    u16 c2[512 * 16];
    u32 c2top[512];
};
static_assert(sizeof(CmTables) == 150016, "16-bit cells, cell 16 of counter2 apart");
static_assert(sizeof(CmTables) + 4 * CM_RING_WORDS + 64 <= KNZ_LDS_BYTES, "the predictor of a block lives in the LDS of one workgroup");

// KNZ_CM_TIER1_DIV=d (a debugging aid like KNZ_POISON_WS, read on every call so that a test can set it): the first tier -- the
// encoder's first staging and what knz_hip_encode_bound returns for CM -- becomes n / d, so that blocks that do not compress take the
// second pass and the callers' retries with the second tier. The emulator build has no environment to set: it fixes the value.
u32 cm_tier1_div()
{
#ifdef KNZ_EMU_CM_STAGE1_DIV
    return KNZ_EMU_CM_STAGE1_DIV;
#else
    const char* e = getenv("KNZ_CM_TIER1_DIV");
    const int v = e ? atoi(e) : 0;
    return v > 0 ? (u32)v : 0u;
#endif
}

__device__ __forceinline__ void cm_init(CmTables& t, int lane)
{
    u32* w1 = reinterpret_cast<u32*>(t.c1);
    for (u32 i = (u32)lane; i < 256 * 257 / 2; i += 64) w1[i] = 0x80008000u;
    for (u32 i = (u32)lane; i < 512 * 16; i += 64) t.c2[i] = (u16)((i & 15) << 12);
    for (u32 i = (u32)lane; i < 512; i += 64) t.c2top[i] = 65536;
}

// CMPredictor::update for one cell at rate r
__device__ __forceinline__ u32 cm_move(u32 p, bool one, int r)
{
    return one ? p - (u32)(((int)p - 65536 + 16) >> r) : p - (p >> r);
}

struct CmCtx { u32 c1, c2, ctx, runMask; };

// The five cells of one bit, read by every lane (same address: a broadcast) and made wave-uniform; get()'s 12-bit split.
struct CmCells { u32 a, b, d, e, idx, row; };
__device__ __forceinline__ u32 cm_get(const CmTables& t, const CmCtx& s, CmCells& k)
{
    const u16* r1 = t.c1 + s.ctx * 257;
    k.a = uni(r1[256]);
    k.b = uni(r1[s.c1]);
    const u32 c = uni(r1[s.c2]);
    const u32 p = (13 * (k.a + k.b) + 6 * c) >> 5;
    k.idx = p >> 12;
    k.row = s.ctx | s.runMask;
    k.d = uni(t.c2[k.row * 16 + k.idx]);
    k.e = uni(k.idx == 15 ? t.c2top[k.row] : (u32)t.c2[k.row * 16 + ((k.idx + 1) & 15)]);
    return (p + p + 3 * (k.d + k.e) + 64) >> 7;
}

// update(): every lane stores the same values (no exec-mask detour on the chain); rates 2 / 4 / 6 / 6
__device__ __forceinline__ void cm_update(CmTables& t, CmCtx& s, const CmCells& k, bool one)
{
    u16* r1 = t.c1 + s.ctx * 257;
    r1[256] = (u16)cm_move(k.a, one, 2);
    r1[s.c1] = (u16)cm_move(k.b, one, 4);
    t.c2[k.row * 16 + k.idx] = (u16)cm_move(k.d, one, 6);
    const u32 e = cm_move(k.e, one, 6);
    if (k.idx == 15) t.c2top[k.row] = e; else t.c2[k.row * 16 + k.idx + 1] = (u16)e;
    s.ctx = 2 * s.ctx + (one ? 1u : 0u);
    if (s.ctx > 255) {
        s.c2 = s.c1;
        s.c1 = s.ctx & 0xFF;
        s.ctx = 1;
        s.runMask = (s.c1 == s.c2) ? 0x100u : 0u;
    }
}

// The predictor as binary_coder.hpp takes it
struct CmPred {
    CmTables& t;
    CmCtx s;
    CmCells cells;
    __device__ __forceinline__ explicit CmPred(CmTables& tables) : t(tables) { s.c1 = 0; s.c2 = 0; s.ctx = 1; s.runMask = 0; }
    __device__ __forceinline__ u32 get() { return cm_get(t, s, cells); }
    __device__ __forceinline__ void update(bool one) { cm_update(t, s, cells, one); }
};

// ------------------------------------------------------------------------------------------------
// encoder: one wave per block
// ------------------------------------------------------------------------------------------------
// ctrl[0] = number of marked blocks, ctrl[1 + b] = 1: block b did not fit its first staging. pass 0 codes every block into
// tmp + b * tmpStride (capacity cm_stage1(len)); pass 1 codes the marked blocks again into big + bigOff[b] (capacity 32 len + 16).
__global__ __launch_bounds__(64) void k_cm_encode(BlockView view, const u32* __restrict__ origLen, u32 copyThreshold, int maxChunks,
                                                  ChunkDesc* __restrict__ desc, u8* __restrict__ tmp, u64 tmpStride, u32* __restrict__ ctrl,
                                                  u8* __restrict__ big, const u64* __restrict__ bigOff, int pass, u32 tier1Div)
{
    __shared__ CmTables t;
    __shared__ u32 ring[CM_RING_WORDS];
    const int b = blockIdx.x;
    const int lane = lane_id();
    const u32 count = view.len[b];
    const u8* blk = view.ptr[b];
    ChunkDesc* cds = desc + (size_t)b * maxChunks;
    if (pass == 1 && ctrl[1 + b] != 1) return;
    if (origLen[b] <= copyThreshold) {
        if (lane == 0) binary_copy_desc(cds[0], blk, count);
        return;
    }
    cm_init(t, lane);
    __syncthreads();
    u8* buf = pass ? big + bigOff[b] : tmp + (size_t)b * tmpStride;
    const u64 cap = pass ? 32ull * count + 16 : cm_stage1(count, tier1Div);
    CmPred pr(t);
    const bool full = binary_encode_block(pr, blk, count, buf, cap, cds, ring, lane);
    // (pass 1 cannot fill its staging: a bit leaves at most one unit, 32 bytes per input byte; the check only guards the memory)
    if (full && pass == 0 && lane == 0) { ctrl[1 + b] = 1; atomicAdd(&ctrl[0], 1u); }
}

// ------------------------------------------------------------------------------------------------
// decoder: one wave per block, wave-uniform chain
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void k_cm_decode(BitSrc src, DecBlock* __restrict__ blocks, u8* const* __restrict__ outPtr)
{
    __shared__ CmTables t;
    const int b = blockIdx.x;
    const int lane = lane_id();
    DecBlock& db = blocks[b];
    BitSrc s;
    u8* block = outPtr[b];
    if (binary_decode_head(src, db, s, block, lane)) return;
    u64 pos = db.entropyBit;
    cm_init(t, lane);
    __syncthreads();
    CmPred pr(t);
    const bool fail = binary_decode_block(pr, src, s, pos, db.preLen, block, lane);
    if (lane == 0) {
        if (fail) db.error = KNZ_ERR_PROCESS_BLOCK;
        db.usedBits = pos - db.entropyBit;
    }
}

int cm_max_chunks(u64 S) { return S >= CM_BIG_BLOCK ? (int)CM_MAX_CHUNKS : 1; }
u64 cm_stage_stride(u64 S) { return (cm_stage1(S, cm_tier1_div()) + 255) & ~255ull; }
size_t cm_ctrl_bytes(int nBlocks) { return (4 * ((size_t)nBlocks + 1) + 7) / 8 * 8 + 8 * (size_t)nBlocks; }

void launch_cm_encode(hipStream_t s, BlockView view, const u32* origLen, u32 copyThreshold, int nBlocks, int maxChunks, ChunkDesc* desc,
                      u8* tmp, u64 tmpStride, void* ctrlMem)
{
    u32* ctrl = reinterpret_cast<u32*>(ctrlMem);
    hipMemsetAsync(desc, 0, sizeof(ChunkDesc) * (size_t)nBlocks * maxChunks, s);
    hipMemsetAsync(ctrl, 0, 4 * ((size_t)nBlocks + 1), s);
    { KScope ks_("k_cm_encode"); hipLaunchKernelGGL(k_cm_encode, dim3(nBlocks), dim3(64), 0, s, view, origLen, copyThreshold, maxChunks, desc, tmp, tmpStride, ctrl,
                                                    (u8*)nullptr, (const u64*)nullptr, 0, cm_tier1_div()); }
}

// What both binary coders do before their second pass: read the marks and the lengths back (the stream is synchronised), lay the marked
// blocks out in a second staging of 32 n + 16 bytes each that bigAlloc gives, and put the offsets behind the marks. Returns the
// number of marked blocks, -1 for a HIP error, -2 when bigAlloc failed.
int binary_again_prepare(hipStream_t s, BlockView view, int nBlocks, void* ctrlMem, CmBigAlloc bigAlloc, void* user, u64** bigOffOut, u8** bigOut)
{
    u32* ctrl = reinterpret_cast<u32*>(ctrlMem);
    u64* bigOff = *bigOffOut = reinterpret_cast<u64*>(reinterpret_cast<u8*>(ctrlMem) + (4 * ((size_t)nBlocks + 1) + 7) / 8 * 8);
    std::vector<u32> flags((size_t)nBlocks), lens((size_t)nBlocks);
    if (hipMemcpyAsync(flags.data(), ctrl + 1, 4 * (size_t)nBlocks, hipMemcpyDeviceToHost, s) != hipSuccess) return -1;
    if (hipMemcpyAsync(lens.data(), view.len, 4 * (size_t)nBlocks, hipMemcpyDeviceToHost, s) != hipSuccess) return -1;
    if (hipStreamSynchronize(s) != hipSuccess) return -1;
    std::vector<u64> off((size_t)nBlocks, 0);
    u64 total = 0;
    int marked = 0;
    for (int b = 0; b < nBlocks; b++) {
        if (flags[b] != 1) continue;
        marked++;
        off[b] = total;
        total += (32ull * lens[b] + 16 + 255) & ~255ull;
    }
    u8* big = *bigOut = bigAlloc ? reinterpret_cast<u8*>(bigAlloc(user, (size_t)total)) : nullptr;
    if (big == nullptr) return -2;
    if (hipMemcpyAsync(bigOff, off.data(), 8 * (size_t)nBlocks, hipMemcpyHostToDevice, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess) return -1;
    return marked;
}

// The rare path: the caller has read the first word of ctrlMem back (with whatever else it reads back behind the encoder) and found it
// non-zero. Reads the marks and the lengths back, asks for the second staging and codes the marked blocks again.
int launch_cm_encode_again(hipStream_t s, BlockView view, const u32* origLen, u32 copyThreshold, int nBlocks, int maxChunks, ChunkDesc* desc,
                           u8* tmp, u64 tmpStride, void* ctrlMem, CmBigAlloc bigAlloc, void* user)
{
    u32* ctrl = reinterpret_cast<u32*>(ctrlMem);
    u64* bigOff = nullptr;
    u8* big = nullptr;
    const int marked = binary_again_prepare(s, view, nBlocks, ctrlMem, bigAlloc, user, &bigOff, &big);
    if (marked < 0) return marked;
    { KScope ks_("k_cm_encode"); hipLaunchKernelGGL(k_cm_encode, dim3(nBlocks), dim3(64), 0, s, view, origLen, copyThreshold, maxChunks, desc, tmp, tmpStride, ctrl,
                                                    big, (const u64*)bigOff, 1, 0u); }
    return marked;
}

void launch_cm_decode(hipStream_t s, BitSrc src, DecBlock* blocks, int nBlocks, u8* const* outPtr)
{
    { KScope ks_("k_cm_decode"); hipLaunchKernelGGL(k_cm_decode, dim3(nBlocks), dim3(64), 0, s, src, blocks, outPtr); }
}

}  // namespace knz
