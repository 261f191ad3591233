// Launchers of the device stages (defined in the .hip files next to this header).
#pragma once
#include "common.hpp"

namespace knz {

struct FrameParams {
    int framing;          // 0: raw entropy output of block 0 only (per-stage API), 1: block framing
    int nTransforms;      // number of transform slots in the sequence
    int checksumBits;
    int finish;
    u32 prologueBits;
};

// bitasm.hip
// Per-block tables (the trailing arguments of the bookkeeping launchers here, in sequence.hip and in xxhash.hip): a batch of many
// streams (streams.hip) places block b at a byte offset of its own, with a length and, on the way back, a room of its own. nullptr =
// one stream cut into equal blocks, b * stride.
void launch_init_blocks(hipStream_t s, u64 n, u32 blockSize, int nBlocks, u32* origLen, u32* blockLen, const u32* lenTab = nullptr);
// A block owns ceil(len / chunkSize) * slotMul consecutive ChunkDesc slots (slotMul > 1: ANS1, one slot per context table).
void launch_block_sum(hipStream_t s, ChunkDesc* desc, BlockInfo* info, const u32* blockLen, int nBlocks, int maxChunks, u32 chunkSize, u32 slotMul);
void launch_block_scan(hipStream_t s, BlockInfo* info, const u32* blockLen, const u32* origLen, int nBlocks, FrameParams fp, u64* totalBits);
void launch_assemble(hipStream_t s, const ChunkDesc* desc, const BlockInfo* info, const u32* blockLen, const u32* origLen,
                     const u8* skipFlags, const u64* checksums, const u8* hdrBase, int nBlocks, int maxChunks, u32 chunkSize,
                     u32 slotMul, u32 hdrStride, FrameParams fp, u32* out);
void launch_put_prologue(hipStream_t s, u32* out, const u8* d_prologue, u32 bits);
void launch_shift_bits(hipStream_t s, const u8* in, u64 nbits, u32 r, u8* out);
void launch_walk_blocks(hipStream_t s, BitSrc src, u64 startBit, int64_t maxBlocks, int framing, u32 rawLen, int checksumBits,
                        u32 blockSize, DecBlock* blocks, void* res);
void launch_check_prelen(hipStream_t s, DecBlock* blocks, int nBlocks, u32 maxPre, u64 outCap, u64 outStride, const u64* roomTab = nullptr);

// streams.hip: the framing of a batch of many independent streams. Stream i owns the blocks [st[i].first, st[i + 1].first) of the batch
// (st has one entry more than there are streams); itemOf[b] is the stream of block b.
struct StreamEnc { u32 first; u32 prologueBits; u32 prologueOff; u32 pad; };      // prologueOff: into the call's prologue bytes
struct StreamOut { u64 base; u64 bits; };                                         // where the stream lies in the output (bytes), its length
struct StreamDec { u64 inOff; u64 inBits; u64 startBit; u64 outOff; u64 outCap; };
struct StreamWalk { u64 first; u32 count; int32_t error; int32_t ended; u32 pad; };   // first block's slot, blocks, the walk's verdict
// hdrBits / written / lw / bitOff of every block (payloadBits set by launch_block_sum), res[i] and *totalBytes: what launch_block_scan
// leaves for one stream, for all of them; the streams lie back to back from byte 0, each at a multiple of 16. excl: nBlocks + 1 words.
void launch_stream_frame(hipStream_t s, BlockInfo* info, const u32* blockLen, const u32* origLen, const u32* itemOf, int nBlocks, const StreamEnc* st, int nItems,
                         FrameParams fp, u64* excl, StreamOut* res, u64* totalBytes);
void launch_stream_prologues(hipStream_t s, u32* out, const StreamEnc* st, const StreamOut* res, int nItems, const u8* prologues);
// res: nItems + 1 entries; res[nItems].first = blocks of all streams. Then, with room for that many: the DecBlock entries (bit positions
// counted from `in`) and every block's place and room in the output.
void launch_walk_streams_count(hipStream_t s, const u8* in, const StreamDec* sd, int nItems, int checksumBits, u32 blockSize, StreamWalk* res);
void launch_walk_streams_fill(hipStream_t s, const u8* in, const StreamDec* sd, int nItems, int checksumBits, u32 blockSize, const StreamWalk* res,
                              DecBlock* blocks, u64* outOff, u64* room);

// none.hip
void launch_none_encode(hipStream_t s, BlockView view, int nBlocks, int maxChunks, ChunkDesc* desc);
void launch_none_decode(hipStream_t s, BitSrc src, DecBlock* blocks, int nBlocks, u8* const* outPtr);

// ans.hip
void launch_ans0_encode(hipStream_t s, BlockView view, int nBlocks, int maxChunks, ChunkDesc* desc, uint2* encTab, u8* tmp);
void launch_ans0_decode(hipStream_t s, BitSrc src, DecBlock* blocks, int nBlocks, int maxChunks, void* chunkMeta, u8* const* outPtr);
size_t ans0_dec_chunk_bytes();

// ans1.hip (order-1 rANS: 4 MiB chunks, 256 context tables per chunk)
constexpr u32 ANS1_CHUNK = 4u << 20;
constexpr u32 ANS1_SLOTS = 257;              // ChunkDesc slots per chunk: 256 context headers + (var-int, states, payload)
struct Ans1EncWs { u32* hist; uint2* encTab; u8* hdr; u8* pay; u64 payStride; };
void launch_ans1_encode(hipStream_t s, BlockView view, int nBlocks, int chunksPerBlock, ChunkDesc* desc, const Ans1EncWs& ws);
size_t ans1_hist_bytes(size_t nChunks);
size_t ans1_enctab_bytes(size_t nChunks);
struct Ans1DecWs { void* meta; u32* slotTab; };
void launch_ans1_decode(hipStream_t s, BitSrc src, DecBlock* blocks, int nBlocks, int chunksPerBlock, const Ans1DecWs& ws, u8* const* outPtr);
size_t ans1_meta_bytes(size_t nChunks);
size_t ans1_slottab_bytes(size_t nChunks);

// range.hip (RANGE, entropy id 4: chunks of 32,768 bytes). A chunk of n bytes leaves at most RANGE_MAX_UNITS(n) = n + n / 64 + 2 units of
// 28 bits (derived at k_range_encode) and 60 bits of low: the staging region of a chunk slot holds that behind the header buffer.
constexpr u32 RANGE_CHUNK = 1u << 15;
constexpr u32 RANGE_MAX_UNITS = RANGE_CHUNK + RANGE_CHUNK / 64 + 2;
constexpr u32 RANGE_PAY_BYTES = ((28u * RANGE_MAX_UNITS + 60u + 31u) / 32u * 4u + 255u) & ~255u;      // 116,736
constexpr u32 RANGE_STRIDE = HDR_BYTES + RANGE_PAY_BYTES;                                            // a multiple of 64
void launch_range_encode(hipStream_t s, BlockView view, const u32* origLen, u32 copyThreshold, int nBlocks, int maxChunks, ChunkDesc* desc,
                         u32* cumFreq, u8* tmp);
void launch_range_decode(hipStream_t s, BitSrc src, DecBlock* blocks, int nBlocks, u8* const* outPtr, int framing);
void launch_range_div_probe(hipStream_t s, const u64* d, const u64* r, u32 n, u32* q);      // range_div on n pairs (tests)

// prims_probe.hip (tests: the scans and the radix sort of prims.hpp by themselves; 0, or a code for the C ABI with its message in err)
void prims_probe_info(u32 out[4]);
int prims_probe_scan(hipStream_t s, int op, const u32* in, u32* out, size_t nMax, const u32* nDev, u32* totalOut, char* err, size_t errCap);
int prims_probe_sort(hipStream_t s, int keyBytes, int hasVal, int keep, int oneRead, const void* keys, const u32* vals, const u32* segBase, int nSeg,
                     size_t maxSegLen, int loBit, int hiBit, void* keysOut, u32* valsOut, char* err, size_t errCap);

// One transform stage over a batch (all arrays are device arrays indexed by block).
struct XfStage {
    const u8* const* src;
    u8* const* dst;
    const u32* len;          // active length (0 = block does not take part in this stage)
    const u32* cap;          // destination capacity seen by the transform
    u8* ok;                  // out: 1 when the reference's forward()/inverse() would return true
    u32* newLen;             // out: bytes produced
    int nBlocks;
    u32 maxLen;              // upper bound of len[] (grid sizing)
    u32* scratchU32;         // stage scratch (8-byte aligned)
    int entropyType;         // stream entropy id (RLT escape choice)
    int bsVersion = 6;       // bitstream version the blocks come from (inverse only: BWT block header of versions below 6)
    u32 maxCap = 0;          // upper bound of cap[] when the host knows one (inverse stages that size scratch by their output)
    u32 capModel = 0;        // inverse: the capacity of the reference's buffer where cap[] is smaller (the last inverse stage of a stream writes
                             // into the caller's buffer, one block size per block, while the reference decodes into a buffer with slack):
                             // UTF and EXE, whose verdicts depend on the capacity, judge by max(cap, capModel) and write within cap. 0: cap[] is all
    u8* dtype = nullptr;     // per-block Global::DataType (0 = UNDEFINED) read and written by PACK, MM, UTF, ROLZX, EXE and TEXT; nullptr: a fresh context per block
    u32 onlyDNA = 0;         // PACK forward as the DNA transform (AliasCodec with packOnlyDNA): blocks that are not DNA are refused
    u32 blockSize = 0;       // the stream's block size (the "blockSize" of the reference's Context): TEXT sizes its hash map by it. 0: none given
};

// zrlt_mtft.hip
void launch_zrlt_forward(hipStream_t s, const XfStage& st);
void launch_zrlt_inverse(hipStream_t s, const XfStage& st);
void launch_mtft_forward(hipStream_t s, const XfStage& st);
void launch_mtft_inverse(hipStream_t s, const XfStage& st);
size_t zrlt_scratch_u32(int nBlocks, u32 maxLen);
size_t mtft_scratch_u32(int nBlocks, u32 maxLen);
int mtft_tune_chain(int on);                                 // 1 = forward ranks by the byte-serial chain kernel (knz_hip_tune "mtf_chain")
int mtft_tune(int tileBytes);                                // 0 = tile size by batch size, 1024 / 4096 force it (knz_hip_tune "mtf_tile")

// bwt.hip (these synchronise the stream: active-set sizes are read back through h_pinned)
int launch_bwt_forward(hipStream_t s, const XfStage& st, void* scratch, size_t scratchBytes, u32* h_pinned);
int launch_bwt_inverse(hipStream_t s, const XfStage& st, void* scratch, size_t scratchBytes, u32* h_pinned);
size_t bwt_forward_scratch_bytes(int nBlocks, u32 VS, size_t total);
size_t bwt_inverse_scratch_bytes(int nBlocks, u32 VS, size_t total);
int bwt_forward_tune(const char* key, int value);          // developer knobs of the suffix sort (knz_hip_tune)
int bwt_inverse_tune(int knob, int value);                 // knz_hip_tune: 0 "bwt_inv_jump_all", 1 "bwt_inv_ruler_log", 2 "bwt_inv_wide"

// bwts.hip (these synchronise the stream like the BWT stages; cap >= len is all a block needs, blocks below 2 bytes are copied)
int launch_bwts_forward(hipStream_t s, const XfStage& st, void* scratch, size_t scratchBytes, u32* h_pinned);
int launch_bwts_inverse(hipStream_t s, const XfStage& st, void* scratch, size_t scratchBytes, u32* h_pinned);
size_t bwts_forward_scratch_bytes(int nBlocks, u32 VS, size_t total);
size_t bwts_inverse_scratch_bytes(int nBlocks, u32 VS, size_t total);

// pack.hip (AliasCodec; scratch: pack_scratch_bytes(nBlocks, maxLen) bytes)
void launch_pack_forward(hipStream_t s, const XfStage& st, void* scratch);
void launch_pack_inverse(hipStream_t s, const XfStage& st, void* scratch);
size_t pack_scratch_bytes(int nBlocks, u32 maxLen);

// mm.hip (FSDCodec; scratch: mm_scratch_bytes(nBlocks, maxLen) bytes; reads and writes XfStage::dtype like PACK)
void launch_mm_forward(hipStream_t s, const XfStage& st, void* scratch);
void launch_mm_inverse(hipStream_t s, const XfStage& st, void* scratch);
size_t mm_scratch_bytes(int nBlocks, u32 maxLen);

// lzp.hip (LZPCodec; scratch: lzp_scratch_bytes(nBlocks, maxLen) bytes, one table of 65,536 positions per block, cleared by the launcher)
void launch_lzp_forward(hipStream_t s, const XfStage& st, void* scratch);
void launch_lzp_inverse(hipStream_t s, const XfStage& st, void* scratch);
size_t lzp_scratch_bytes(int nBlocks, u32 maxLen);

// rolzx.hip (ROLZCodec2; scratch: rolzx_scratch_bytes(nBlocks, maxLen) bytes, about 8.3 MiB of tables for each block that runs at once,
// bounded by KNZ_ROLZX_TABLES_MAX: the launchers run a larger batch in slices and the kernels clear the tables; reads XfStage::dtype
// and writes detectSimpleType's verdict like PACK; no host synchronisation)
void launch_rolzx_forward(hipStream_t s, const XfStage& st, void* scratch);
void launch_rolzx_inverse(hipStream_t s, const XfStage& st, void* scratch);
size_t rolzx_scratch_bytes(int nBlocks, u32 maxLen);

// utf.hip (UTFCodec; scratch: utf_scratch_bytes(nBlocks, maxLen) bytes, about 1.8 MiB per block plus len / 4; reads and writes
// XfStage::dtype like PACK; no host synchronisation)
void launch_utf_forward(hipStream_t s, const XfStage& st, void* scratch);
void launch_utf_inverse(hipStream_t s, const XfStage& st, void* scratch);
size_t utf_scratch_bytes(int nBlocks, u32 maxLen);

// exe.hip (EXECodec; scratch: exe_scratch_bytes(nBlocks, maxLen) bytes, about 1 KiB per block plus len / 4; reads and writes
// XfStage::dtype; the inverse judges by max(cap, capModel) like UTF's; no host synchronisation)
void launch_exe_forward(hipStream_t s, const XfStage& st, void* scratch);
void launch_exe_inverse(hipStream_t s, const XfStage& st, void* scratch);
size_t exe_scratch_bytes(int nBlocks, u32 maxLen);

// text.hip (TextCodec, both word-index encodings, chosen by XfStage::entropyType; scratch: text_scratch_bytes(nBlocks, maxLen, blockSize)
// bytes -- a hash map sized by the stream's block size, up to 2^19 entries and two words per possible word for each block that runs at
// once, bounded by KNZ_TEXT_TABLES_MAX: the launchers run a larger batch in slices and clear the tables on the stream; reads and
// writes XfStage::dtype; the inverse judges by max(cap, capModel) like UTF's; no host synchronisation)
void launch_text_forward(hipStream_t s, const XfStage& st, void* scratch);
void launch_text_inverse(hipStream_t s, const XfStage& st, void* scratch);
size_t text_scratch_bytes(int nBlocks, u32 maxLen, u32 blockSize);

// fpaq.hip (probs: fpaq_probs_bytes(nBlocks, S) bytes of scratch, S = upper bound of the block lengths)
void launch_fpaq_encode(hipStream_t s, BlockView view, const u32* origLen, u32 copyThreshold, int nBlocks, int maxChunks, ChunkDesc* desc, u8* tmp, u64 tmpStride,
                        u16* probs, u64 S);
size_t fpaq_probs_bytes(int nBlocks, u64 S);
void launch_fpaq_decode(hipStream_t s, BitSrc src, DecBlock* blocks, int nBlocks, u8* const* outPtr);

// cm.hip (CM, entropy id 6). A block owns cm_max_chunks(S) ChunkDesc slots (1, or CM_MAX_CHUNKS when blocks can reach the size the
// format splits at); its payload is staged at tmp + b * tmpStride, tmpStride = cm_stage_stride(S) (n + n / 8 + slack: no bound is proved
// for CM). launch_cm_encode leaves the number of blocks that did not fit in the first 32-bit word of ctrlMem (cm_ctrl_bytes(nBlocks)
// bytes of device memory); a caller that reads a non-zero count back calls launch_cm_encode_again before it uses the descriptors:
// the marked blocks are coded again into 32 n + 16 bytes each, which it asks bigAlloc for (device memory that lives until the stream
// is assembled; nullptr = failure). That call synchronises the stream; it returns the number of blocks coded again, -1 for a HIP
// error, -2 when bigAlloc failed.
constexpr u32 CM_MAX_CHUNKS = 17;            // ceil(count / (count >> 4)) for count >= 256
typedef void* (*CmBigAlloc)(void* user, size_t bytes);
int cm_max_chunks(u64 S);
u32 cm_tier1_div();                          // 0, or the divisor KNZ_CM_TIER1_DIV sets for tests (cm.hip)
u64 cm_stage_stride(u64 S);
size_t cm_ctrl_bytes(int nBlocks);
void launch_cm_encode(hipStream_t s, BlockView view, const u32* origLen, u32 copyThreshold, int nBlocks, int maxChunks, ChunkDesc* desc,
                      u8* tmp, u64 tmpStride, void* ctrlMem);
int launch_cm_encode_again(hipStream_t s, BlockView view, const u32* origLen, u32 copyThreshold, int nBlocks, int maxChunks, ChunkDesc* desc,
                           u8* tmp, u64 tmpStride, void* ctrlMem, CmBigAlloc bigAlloc, void* user);
void launch_cm_decode(hipStream_t s, BitSrc src, DecBlock* blocks, int nBlocks, u8* const* outPtr);

int binary_again_prepare(hipStream_t s, BlockView view, int nBlocks, void* ctrlMem, CmBigAlloc bigAlloc, void* user, u64** bigOffOut, u8** bigOut);

// tpaq.hip (TPAQ, entropy id 7, extra = 0; TPAQX, id 9, extra = 1). Slots, staging, ctrlMem and the second pass as CM's (cm_max_chunks,
// cm_stage_stride, cm_ctrl_bytes). The predictor's tables live in `tables`: tpaq_table_bytes(rbsz, abszMax, extra) bytes for each of
// tpaq_slice_blocks(that, nBlocks) blocks; rbsz is the stream's block size, abszMax the longest block (after the transforms) that the
// batch can hold. The launchers zero the tables on the stream and run the batch in slices of that many blocks.
struct TpaqSizes { u32 states, mixers, hash, buffer, sse0, sse1; };
TpaqSizes tpaq_params(u32 rbsz, u32 absz, int extra);       // the format's sizes (tests: knz_hip_tpaq_params)
u32 tpaq_states_log();                                      // 0, or the k of KNZ_TPAQ_STATES_LOG (tests)
size_t tpaq_table_bytes(u32 rbsz, u32 abszMax, int extra);
int tpaq_slice_blocks(size_t tableBytes, int nBlocks);      // KNZ_TPAQ_TABLES_MAX: bytes of tables in use at once (default 16 GiB)
void launch_tpaq_encode(hipStream_t s, int extra, BlockView view, const u32* origLen, u32 copyThreshold, int nBlocks, int maxChunks, ChunkDesc* desc,
                        u8* tmp, u64 tmpStride, void* ctrlMem, void* tables, u32 rbsz, u32 abszMax);
int launch_tpaq_encode_again(hipStream_t s, int extra, BlockView view, const u32* origLen, u32 copyThreshold, int nBlocks, int maxChunks, ChunkDesc* desc,
                             u8* tmp, u64 tmpStride, void* ctrlMem, CmBigAlloc bigAlloc, void* user, void* tables, u32 rbsz, u32 abszMax);
void launch_tpaq_decode(hipStream_t s, int extra, BitSrc src, DecBlock* blocks, int nBlocks, u8* const* outPtr, void* tables, u32 rbsz, u32 abszMax);

void launch_srt_forward(hipStream_t s, const XfStage& st);          // scratch: srt_scratch_u32(nBlocks, maxLen) words
size_t srt_scratch_u32(int nBlocks, u32 maxLen);
void launch_srt_inverse(hipStream_t s, const XfStage& st);          // scratch: srt_inverse_scratch_u32(nBlocks, maxLen) words
size_t srt_inverse_scratch_u32(int nBlocks, u32 maxLen);
void launch_rlt_forward(hipStream_t s, const XfStage& st);
void launch_rlt_inverse(hipStream_t s, const XfStage& st);

// sbrt.hip (mode 2 = RANK, 3 = TIMESTAMP; 1 = MTF for cross-checks)
void launch_sbrt_forward(hipStream_t s, const XfStage& st, int mode);
void launch_sbrt_inverse(hipStream_t s, const XfStage& st, int mode);

// lz.hip (ttype = KNZ_T_LZ or KNZ_T_LZX)
int launch_lz_forward(hipStream_t s, const XfStage& st, int ttype, void* scratch, size_t scratchBytes);
void launch_lz_inverse(hipStream_t s, const XfStage& st, void* scratch, size_t scratchBytes, u32 maxCap);   // no scratch: serial decoder only
size_t lz_inverse_scratch_bytes(int nBlocks, u32 maxCap);
int lz_serial_decode(int set);                               // knob "lz_serial_decode": >= 0 sets it, returns the value (1 = one wave per block only)
size_t lz_forward_scratch_bytes(int ttype, int nBlocks, u32 maxLen);

// xxhash.hip
void launch_xxhash(hipStream_t s, const u8* const* ptr, const u32* lens, int nBlocks, int bits, u64* out);
void launch_block_ptrs(hipStream_t s, const u8* base, u64 stride, int nBlocks, const u8** ptr, const u64* offTab = nullptr);
void launch_verify_checksums(hipStream_t s, DecBlock* blocks, int nBlocks, int bits, const u8* out, u64 outStride, const u8** ptrScratch,
                             u32* lenScratch, u64* sumScratch, const u64* offTab = nullptr);

// sequence.hip : TransformSequence bookkeeping on the device
struct SeqArrays {
    u8* where;               // 0 = caller buffer, 1 = workspace A, 2 = workspace B
    u8* swaps;
    u8* active;
    u32* len;                // current data length per block
    u32* alen;               // active length for the current stage
    u8* skip;                // skip flags (bit 7-i set = stage i not applied)
    const u8** src;
    u8** dst;
    u32* cap;
    u8* ok;
    u32* newLen;
    const u32* origLen;
    const u32* dataCap;      // reference buffer capacities (forward only)
    const u32* bufCap;
    u8* dtype;               // per-block data type (forward: preset from the block's magic, io/CompressedOutputStream.cpp:722-731)
};
void launch_seq_fwd_direct(hipStream_t s, const SeqArrays& a, u32* origLen, u64 n, u32 blockSize, int nBlocks, int nStages, const u8* in, const u8** viewPtr,
                           const u64* inOff = nullptr, const u32* lenTab = nullptr);
void launch_seq_fwd_prepare(hipStream_t s, const SeqArrays& a, int nBlocks, int stage, const u8* in, u64 inStride, u8* A, u8* B, u64 S, const u64* inOff = nullptr);
void launch_seq_fwd_null(hipStream_t s, const SeqArrays& a, int nBlocks, int stage);
void launch_seq_fwd_hosted(hipStream_t s, const SeqArrays& a, int nBlocks, int stage, int applied);
void launch_seq_fwd_commit(hipStream_t s, const SeqArrays& a, int nBlocks, int stage);
void launch_seq_fwd_dtype(hipStream_t s, const SeqArrays& a, int nBlocks, const u8* in, u64 inStride, const u64* inOff = nullptr);
void launch_seq_fwd_finish(hipStream_t s, const SeqArrays& a, int nBlocks, const u8* in, u64 inStride, u8* A, u8* B, u64 S, const u8** viewPtr, const u64* inOff = nullptr);
void launch_seq_inv_entropy_dst(hipStream_t s, const SeqArrays& a, DecBlock* blocks, int nBlocks, u8* out, u64 outStride, u8* A, u64 S, u8** entDst, u32 realMask, u32 unit, u64 outCap,
                                const u64* outOff = nullptr, const u64* roomTab = nullptr);
void launch_seq_inv_prepare(hipStream_t s, const SeqArrays& a, DecBlock* blocks, int nBlocks, int stage, u8* out, u64 outStride, u8* A, u8* B, u64 S, u32 capMid, u32 capFinal, u32 realMask, u64 outCap,
                            const u64* outOff = nullptr, const u64* roomTab = nullptr);
void launch_seq_inv_commit(hipStream_t s, const SeqArrays& a, DecBlock* blocks, int nBlocks, int stage, int ttype);

// copy_many.hip : n device-to-device copies in one launch; tileFirst = the exclusive prefix of copy_many_tiles over the copies (n + 1 words)
u64 copy_many_tiles(u64 dst, u64 len);
u32 copy_many_tile_bytes();
void launch_copy_many(hipStream_t s, const knz_copy* copies, const u32* tileFirst, u32 n, u32 nTiles);

// planes.hip : n buffers split into byte planes, or joined from them, in one launch; tileFirst = the exclusive prefix of planes_tiles
// over the entries (n + 1 words)
u64 planes_tiles(u64 len);
u32 planes_tile_bytes();
void launch_split_many(hipStream_t s, const knz_plane_copy* entries, const u32* tileFirst, u32 n, u32 nTiles);
void launch_join_many(hipStream_t s, const knz_plane_copy* entries, const u32* tileFirst, u32 n, u32 nTiles);

// huffman.hip
void launch_huffman_encode(hipStream_t s, BlockView view, int nBlocks, int maxChunks, ChunkDesc* desc, u8* tmp);
void launch_huffman_decode(hipStream_t s, BitSrc src, DecBlock* blocks, int nBlocks, int maxChunks, void* chunkMeta, u8* const* outPtr, int bsVersion = 6);
size_t huffman_dec_chunk_bytes();

}  // namespace knz
