/*
 * knz_hip.h -- C ABI of the MI355X (gfx950) kanzi block pipeline.
 *
 * This is the thin device layer SURVEY.md section 8(b) calls "New thin C-ABI to HIP": one call
 * processes a batch of independent blocks that are already resident in HBM and returns the block
 * payloads exactly as the reference's EncodingTask would have put them in its private bitstream
 * (io/CompressedOutputStream.cpp:651-898), assembled MSB-first at bit granularity
 * (bitstream/DefaultOutputBitStream.hpp:97-131). Plain pointers and sizes only; all pointers
 * named d_* are device pointers, everything else is host memory. Every function returns 0 on
 * success, a negative value for a device/runtime failure (see knz_hip_last_error) or a positive
 * kanzi Error code (src/Error.hpp:26-48) for data errors.
 *
 * The C++ host mirror of the reference interfaces (Transform<byte>, EntropyEncoder/Decoder,
 * CompressedOutputStream/InputStream, include/kanzi_amd/) and the reference C API replacement
 * (include/kanzi_api.h) are built on top of these entry points.
 */
#ifndef KNZ_HIP_H
#define KNZ_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define KNZ_API __attribute__((visibility("default")))

/* kanzi ids: entropy (entropy/EntropyEncoderFactory.hpp:37-52) and transforms (transform/TransformFactory.hpp:49-73) */
enum { KNZ_E_NONE = 0, KNZ_E_HUFFMAN = 1, KNZ_E_FPAQ = 2, KNZ_E_RANGE = 4, KNZ_E_ANS0 = 5, KNZ_E_CM = 6, KNZ_E_TPAQ = 7, KNZ_E_ANS1 = 8, KNZ_E_TPAQX = 9 };
enum { KNZ_T_NONE = 0, KNZ_T_BWT = 1, KNZ_T_BWTS = 2, KNZ_T_LZ = 3, KNZ_T_RLT = 5, KNZ_T_ZRLT = 6, KNZ_T_MTFT = 7, KNZ_T_RANK = 8, KNZ_T_EXE = 9, KNZ_T_ROLZX = 12, KNZ_T_SRT = 13, KNZ_T_LZP = 14, KNZ_T_MM = 15, KNZ_T_LZX = 16, KNZ_T_PACK = 18, KNZ_T_DNA = 19 /* PACK that takes DNA blocks only */,
       KNZ_T_TIMESTAMP = 64 /* SBRT's third mode: no kanzi id, never part of a chain; per-stage entry points only */,
       KNZ_T_UTF = 17 /* a device stage in any position; also accepted among the host's leading stages (below) */,
       KNZ_T_TEXT = 10 /* a device stage in any position; also accepted among the host's leading stages (below) */ };

/* kanzi error codes surfaced for data errors (src/Error.hpp:26-48) */
enum { KNZ_ERR_BLOCK_SIZE = 2, KNZ_ERR_INVALID_CODEC = 3, KNZ_ERR_READ_FILE = 11, KNZ_ERR_WRITE_FILE = 12,
       KNZ_ERR_PROCESS_BLOCK = 13, KNZ_ERR_INVALID_FILE = 15, KNZ_ERR_STREAM_VERSION = 16,
       KNZ_ERR_INVALID_PARAM = 18, KNZ_ERR_CRC_CHECK = 19 };

typedef struct knz_ctx knz_ctx;

/* Number of visible HIP devices. */
KNZ_API int knz_hip_device_count(int* count);

/* Create a context on `device`. `stream` is a hipStream_t (as void*) to enqueue on, or NULL to
 * let the context create its own. Workspaces are grown on demand and reused across calls. */
KNZ_API int knz_hip_create(int device, void* stream, knz_ctx** out);
KNZ_API void knz_hip_destroy(knz_ctx* ctx);
KNZ_API const char* knz_hip_last_error(knz_ctx* ctx);

/* Parameters of one batch of blocks: what CompressedOutputStream puts in the per-task Context
 * (io/CompressedOutputStream.cpp:491-496): transform ids (48 bits, 6 per stage, first stage in
 * bits 47..42), entropy id, block size, checksum width (0/32/64). */
typedef struct {
    uint64_t transform_type;
    int32_t entropy_type;
    int32_t block_size;
    int32_t checksum_bits;
    int32_t jobs;            /* reference job count being reproduced (0/1 = single). It only selects the
                                buffer slot, hence the capacities, a block sees. */
    int32_t bs_version;      /* decode only: bitstream version of the stream the blocks come from, as
                                CompressedInputStream puts it in the Context (io/CompressedInputStream.cpp:528-537).
                                0 (unset, the ABI default) or 6 = current. 1..5 select the old layouts the reference still reads (it treats every
                                version below 6 alike; a caller that parsed or was given version 0 passes 1): Huffman chunks
                                (entropy/HuffmanDecoder.cpp:349-459), the BWT block header
                                (transform/BWTBlockCodec.cpp:140-164) and LZ / LZX blocks (transform/LZCodec.cpp:614-760).
                                The encoder writes version 6 only, like the reference. */
} knz_params;

/* Upper bound, in bytes, of the bit-packed output of knz_hip_encode_blocks for n input bytes.
 * KNZ_E_CM: nothing tighter than the format's own ceiling of 32 bytes per input byte is known for CM, so the value is a FIRST tier --
 * n + n / 8 plus framing, what the reference's own buffer starts at and what every input met so far stays below. An encode whose
 * stream does not fit out_cap fails with KNZ_ERR_WRITE_FILE (the message names the size needed) and leaves the context usable;
 * the second tier, knz_hip_encode_bound(p, n) + 32 * n, holds whatever the format can write.
 * KNZ_E_TPAQ, KNZ_E_TPAQX: the same coder behind another predictor; the same two tiers. */
KNZ_API size_t knz_hip_encode_bound(const knz_params* p, size_t n);

/*
 * Encode n bytes at d_in, cut into blocks of p->block_size (the last one may be short), each block
 * through TransformSequence::forward + block header + EntropyEncoder::encode, and append the
 * results in block order as CompressedOutputStream does (5-bit lw-3, lw-bit length, payload bits;
 * io/CompressedOutputStream.cpp:852-864).
 *
 *   prologue/prologue_bits : host bytes placed first (the stream header, or NULL/0)
 *   first_block_id         : 0-based id of the first block in this batch (only for buffer-capacity
 *                            modelling of the reference)
 *   finish                 : append the end-of-stream marker (5+3 zero bits, :415-417)
 *   d_out/out_cap          : device output, zero-filled by the call, out_cap >= knz_hip_encode_bound
 *   out_bits               : total bits written (host). Output bytes = (out_bits+7)/8.
 *
 * The call is synchronous with respect to the host when out_bits != NULL (it has to read the
 * length back); all device work is enqueued on the context's stream.
 */
KNZ_API int knz_hip_encode_blocks(knz_ctx* ctx, const knz_params* p, const uint8_t* d_in, size_t n,
                                  const uint8_t* prologue, uint32_t prologue_bits, int64_t first_block_id,
                                  int finish, uint8_t* d_out, size_t out_cap, uint64_t* out_bits);

/*
 * Decode a run of blocks: d_in holds the bit stream, the first block's 5-bit length prefix is at
 * bit `start_bit`. Blocks are decoded until the end marker, `max_blocks` blocks or `in_bits` is
 * exhausted. Decoded blocks are written back to back at d_out.
 *   out_bytes  : decoded byte count (host)
 *   end_bit    : bit position after the last consumed block / end marker (host, may be NULL)
 * Mirrors DecodingTask::run (io/CompressedInputStream.cpp:790-1041) incl. its accept/reject rules.
 */
KNZ_API int knz_hip_decode_blocks(knz_ctx* ctx, const knz_params* p, const uint8_t* d_in, uint64_t in_bits,
                                  uint64_t start_bit, int64_t max_blocks, uint8_t* d_out, size_t out_cap,
                                  uint64_t* out_bytes, uint64_t* end_bit, int64_t* blocks_done);

/*
 * Chains whose first stages run on the host (the reference's level presets 5 and 6: TEXT + UTF in front of BWT + RANK / SRT + ZRLT,
 * app/BlockCompressor.cpp:583-591). The host applies those stages to ONE block (they change its length by a different amount per block)
 * and hands over what TransformSequence::forward would have left for the next stage (transform/TransformSequence.hpp:88-162):
 *   stages        how many leading stages of p->transform_type the host owns (each KNZ_T_TEXT or KNZ_T_UTF). TEXT is a device stage
 *                 as well (knz_hip_transform_supported(KNZ_T_TEXT) = 1 since it is), so this entry point is for callers that want TEXT
 *                 on the host; they own the chain up to its last leading TEXT, and a UTF in front of that TEXT has to run on the host
 *                 too ("UTF+TEXT+...": stages = 2), a UTF behind it is a device stage like any other ("TEXT+UTF+...": stages = 1 is
 *                 what the stream classes pass; stages = 2 with UTF applied by the caller still works)
 *   applied_mask  bit i set = stage i succeeded (its skip flag is clear, and it counts as a buffer swap for the capacities the
 *                 device stages see); clear = the stage refused the block and the block went on unchanged
 *   orig_len      length of the block before any stage (decides copy blocks and the buffer sizes of the reference)
 *   reserved      the data type the host stages left in the block's Context (Global::DataType: 0 UNDEFINED, 1 TEXT, 2 MULTIMEDIA,
 *                 3 EXE, 4 NUMERIC, 5 BASE64, 6 DNA, 7 BIN, 8 UTF8, 9 SMALL_ALPHABET); the device stages that read it (UTF, PACK, MM) start
 *                 from it. 0 when the caller does not track it; values above 9 count as 0
 *   checksum      XXHash32 / 64 of the ORIGINAL block when p->checksum_bits != 0 (the device only ever sees the transformed bytes)
 * d_in holds the n bytes the host stages left. Everything else as knz_hip_encode_blocks with exactly one block; the block header
 * carries the skip flags of all stages (a separate byte when the chain has more than four, io/CompressedOutputStream.cpp:791-799).
 */
typedef struct { int32_t stages; uint32_t applied_mask; uint32_t orig_len; uint32_t reserved; uint64_t checksum; } knz_host_stages;
KNZ_API int knz_hip_encode_block_hosted(knz_ctx* ctx, const knz_params* p, const knz_host_stages* hs, const uint8_t* d_in, size_t n,
                                        const uint8_t* prologue, uint32_t prologue_bits, int64_t first_block_id, int finish,
                                        uint8_t* d_out, size_t out_cap, uint64_t* out_bits);
/* The way back: ONE block is entropy-decoded and taken through the inverse of the device stages; the host stages are left to the
 * caller, who gets the block's skip flags (bit 7 = stage 0; 0xFF for a copy block) and its stored checksum (not verified here: it is
 * the checksum of the original block). *done = 0 when the end marker was found instead of a block. */
KNZ_API int knz_hip_decode_block_hosted(knz_ctx* ctx, const knz_params* p, int32_t host_stages, const uint8_t* d_in, uint64_t in_bits,
                                        uint64_t start_bit, uint8_t* d_out, size_t out_cap, uint64_t* out_bytes, uint64_t* end_bit,
                                        uint32_t* skip_flags, uint64_t* checksum, int32_t* done);

/*
 * Many independent streams in one call. One call is one batch: the blocks of all items go through the stages together, and the number
 * of kernel launches, host synchronisations and bus copies does not grow with the number of items (TPAQ's table slices excepted).
 * An item is one stream: one input cut into blocks of p->block_size, framed by itself, block ids counted from 0.
 *
 * Limits of a call: at most KNZ_STREAMS_MAX_ITEMS items and KNZ_STREAMS_MAX_BLOCKS blocks; at most 2 GiB of input (encode), or of bytes
 * the streams can decode to (decode: the sum over the items of min(out_cap, blocks found x block size)); blocks x the longest block of
 * the call at most 2 GiB as well (the workspaces are that large: encode, the longest block of any item; decode, the largest
 * min(out_cap, block size) -- so a thousand items of 1 KiB cost the same under a block size of 4 MiB as under one of 1 KiB, and one item
 * of 4 MiB among them makes the call a thousand times 4 MiB); every in_off / out_off a multiple of 16, d_in and d_out 16-byte aligned.
 * A caller with more splits its work into several calls; a call over a limit fails as a whole and says which.
 */
#define KNZ_STREAMS_MAX_ITEMS 65536
#define KNZ_STREAMS_MAX_BLOCKS 65536
typedef struct {
    uint64_t in_off;        /* byte offset of the item in d_in, multiple of 16 */
    uint64_t in_len;        /* encode: bytes of input; decode: bits of the stream, counted from in_off * 8 */
    uint64_t start_bit;     /* decode: bit of the first block's length prefix, relative to in_off * 8 (behind the header) */
    uint32_t prologue_off;  /* encode: where this item's prologue begins in the call's `prologues` host array */
    uint32_t prologue_bits; /* encode: bits put first in the stream (the stream header, or 0); at most 200 bytes */
    uint64_t out_off;       /* encode: OUT, byte offset of the stream in d_out (multiple of 16);
                               decode: IN, byte offset where the item's bytes go (multiple of 16) */
    uint64_t out_cap;       /* decode: IN, room at out_off */
    uint64_t out_len;       /* OUT: encode = bits written, decode = bytes decoded */
    int32_t  blocks;        /* OUT */
    int32_t  error;         /* OUT: 0, or the kanzi Error code of this item */
} knz_item;

/* Bytes of d_out that knz_hip_encode_streams needs for these items (in_len and prologue_bits are read): the sum over the items of
 * knz_hip_encode_bound(p, in_len) plus the prologue, each rounded up to 16. The binary coders' bound is their first tier here too. */
KNZ_API size_t knz_hip_encode_streams_bound(const knz_params* p, const knz_item* items, size_t n_items);

/*
 * Item i becomes exactly the bytes that knz_hip_encode_blocks(d_in + in_off, in_len, prologues + prologue_off, prologue_bits,
 * first_block_id = 0, finish, ...) writes: blocks of p->block_size, copy blocks, the per-block data type, checksums of the original
 * bytes, the skip byte of chains of more than four stages, the capacities of p->jobs, the end marker. An empty item is its prologue
 * plus the end marker. The streams lie in d_out back to back, each at a 16-byte boundary (out_off) with zero bytes up to the next, so
 * that every one can be handed to knz_hip_decode_blocks where it lies; out_len is its length in bits, blocks its block count.
 * *out_bytes = bytes of d_out in use. The call fails as a whole (nothing in `items` is then meaningful): a chain the device refuses,
 * out_cap below knz_hip_encode_streams_bound, more than 2 GiB of input, too many items or blocks, a misaligned offset. Hosted leading
 * stages (knz_host_stages) are not part of this call. `prologues` may be NULL when every prologue_bits is 0.
 */
KNZ_API int knz_hip_encode_streams(knz_ctx* ctx, const knz_params* p, const uint8_t* d_in, knz_item* items, size_t n_items,
                                   const uint8_t* prologues, int finish, uint8_t* d_out, size_t out_cap, uint64_t* out_bytes);

/*
 * All items share p (the caller groups streams by header). For every item the blocks from start_bit to the end marker are decoded
 * to d_out + out_off. Items are judged one by one: error is 0, a block's error code, KNZ_ERR_WRITE_FILE when out_cap is too small
 * for the blocks the stream holds, KNZ_ERR_PROCESS_BLOCK for a short block that is not the last, KNZ_ERR_READ_FILE for damaged
 * framing; out_len and blocks are the decoded bytes and the blocks found (0 bytes for an item with an error). A failing item leaves
 * every other item as a call without it would, and writes nothing outside [out_off, out_off + out_cap). The ranges overlap for no two
 * items and lie inside out_cap bytes of d_out. The return value is non-zero only for failures of the call itself.
 */
KNZ_API int knz_hip_decode_streams(knz_ctx* ctx, const knz_params* p, const uint8_t* d_in, knz_item* items, size_t n_items,
                                   uint8_t* d_out, size_t out_cap);

/*
 * n independent device-to-device copies in ONE kernel launch: what moves scattered device buffers into the packed, 16-aligned d_in of
 * knz_hip_encode_streams, its 16-aligned output streams into one tight blob, and streams at arbitrary byte offsets back to 16-aligned
 * ones for knz_hip_decode_streams. src and dst are absolute device addresses of any alignment, in any relation to each other; len
 * may be 0. Nothing outside [src, src + len) is read and nothing outside [dst, dst + len) is written. No destination range of a call
 * may overlap another range of the same call, source or destination (sources may coincide); this is not checked.
 *
 * The launch is enqueued on the context's stream and the call does not wait for it; the table is staged, so `copies` may be reused
 * as soon as the call returns. n == 0 is a successful no-op. Limits of a call: at most KNZ_COPY_MAX_COPIES copies, every len below
 * 2^32, fewer than 2^31 tiles of 16 KiB in all (a copy of len bytes has at most len / 16384 + 2); a call over a limit fails as a whole
 * with KNZ_ERR_INVALID_PARAM, says which, and launches nothing.
 */
#define KNZ_COPY_MAX_COPIES 1048576
typedef struct { uint64_t src; uint64_t dst; uint64_t len; } knz_copy;   /* device addresses, bytes */
KNZ_API int knz_hip_copy_many(knz_ctx* ctx, const knz_copy* copies /* host */, size_t n);

/*
 * n device buffers split into byte planes, or joined from them, in ONE kernel launch. An entry of len bytes holds m = len / elem
 * elements of elem bytes; split writes dst[k * m + i] = src[i * elem + k] (byte k of every element to plane k), join writes
 * dst[i * elem + k] = src[k * m + i]; with elem == 1 both are a plain copy, so one call can carry ordinary copies beside its planes.
 * What gathers tensors of 2-, 4- and 8-byte elements for knz_hip_encode_streams with their compressible bytes side by side, at the
 * price of the copy that knz_hip_copy_many would make anyway. The element width is not stored anywhere: the caller keeps it.
 *
 * src and dst are absolute device addresses of any alignment; len may be 0. Nothing outside [src, src + len) is read and nothing
 * outside [dst, dst + len) is written. The result is undefined where an entry's dst range overlaps its own src range or any other
 * range of the same call (sources may coincide); this is not checked.
 *
 * Staging, ordering and limits are knz_hip_copy_many's: enqueued on the context's stream without waiting, `entries` reusable as soon
 * as the call returns, n == 0 a successful no-op; at most KNZ_COPY_MAX_COPIES entries, every len below 2^32, fewer than 2^31 tiles
 * of 16 KiB in all (an entry has len / 16384 rounded up). elem has to be 1, 2, 4 or 8 and to divide len, reserved has to be 0. A call
 * that breaks one of these fails as a whole with KNZ_ERR_INVALID_PARAM, names the entry, and launches nothing.
 */
typedef struct { uint64_t src; uint64_t dst; uint64_t len; uint32_t elem; uint32_t reserved; } knz_plane_copy;
KNZ_API int knz_hip_split_many(knz_ctx* ctx, const knz_plane_copy* entries /* host */, size_t n);
KNZ_API int knz_hip_join_many(knz_ctx* ctx, const knz_plane_copy* entries /* host */, size_t n);

/* ---- per-stage entry points (host buffers in/out; used by the host mirror classes and tests) ---- */

/* EntropyEncoder::encode for one buffer (entropy/EntropyEncoder.hpp:30-37). out receives the bits
 * MSB-first from bit 0; *out_bits the exact bit count (dispose() bits included for FPAQ). */
KNZ_API int knz_hip_entropy_encode(knz_ctx* ctx, int entropy_type, const uint8_t* in, uint32_t n,
                                   uint8_t* out, size_t out_cap, uint64_t* out_bits);
/* EntropyDecoder::decode: reads from bit `start_bit` of `in`; *used_bits = bits consumed.
 * Returns 0 and *decoded == n on success; *decoded mirrors the reference's return value otherwise. */
KNZ_API int knz_hip_entropy_decode(knz_ctx* ctx, int entropy_type, const uint8_t* in, uint64_t in_bits,
                                   uint64_t start_bit, uint8_t* out, uint32_t n, int32_t* decoded,
                                   uint64_t* used_bits);
/* The same with the bitstream version the bits come from (knz_params.bs_version: 0 / 6 current, 1..5 the old Huffman chunk
 * layout): what HuffmanDecoder takes from its Context (entropy/HuffmanDecoder.hpp:32, HuffmanDecoder.cpp:349-352). */
KNZ_API int knz_hip_entropy_decode_v(knz_ctx* ctx, int entropy_type, int bs_version, const uint8_t* in, uint64_t in_bits,
                                     uint64_t start_bit, uint8_t* out, uint32_t n, int32_t* decoded,
                                     uint64_t* used_bits);

/* The same two calls with the block size of the stream the buffer belongs to -- the "blockSize" entry of the Context that
 * EntropyEncoderFactory / EntropyDecoderFactory hand to the predictor. KNZ_E_TPAQ and KNZ_E_TPAQX size their tables by it
 * (entropy/TPAQPredictor.hpp:312-339) and by the buffer's own length n (the "size" entry), so the same bytes code differently in
 * streams of different block sizes; the other coders ignore it. 0 = the buffer's own length rounded up to 16, which is what
 * knz_hip_entropy_encode / _decode_v pass. */
KNZ_API int knz_hip_entropy_encode_bs(knz_ctx* ctx, int entropy_type, uint32_t stream_block_size, const uint8_t* in, uint32_t n,
                                      uint8_t* out, size_t out_cap, uint64_t* out_bits);
KNZ_API int knz_hip_entropy_decode_bs(knz_ctx* ctx, int entropy_type, int bs_version, uint32_t stream_block_size, const uint8_t* in,
                                      uint64_t in_bits, uint64_t start_bit, uint8_t* out, uint32_t n, int32_t* decoded, uint64_t* used_bits);

/* Transform<byte>::forward / inverse for one buffer (src/Transform.hpp:38-45). dst_cap mirrors
 * SliceArray::_length - _index of the destination (it changes results for ZRLT/RLT; LZ/LZX refuse a
 * destination below getMaxEncodedLength). *ok = 1 when the reference would return true. entropy_type: the
 * stream's entropy id (RLT escape choice), -1 if unset. Classes replaced, by transform_type:
 *   KNZ_T_BWT   BWTBlockCodec        transform/BWTBlockCodec.cpp:32-87,89-168 (+ BWT.cpp, DivSufSort.cpp)
 *   KNZ_T_MTFT / KNZ_T_RANK / KNZ_T_TIMESTAMP   SBRT modes 1 / 2 / 3   transform/SBRT.cpp:46-97,99-145
 *   KNZ_T_SRT   SRT                  transform/SRT.cpp:22-109,111-204
 *   KNZ_T_ZRLT  ZRLT                 transform/ZRLT.cpp:27-117,119-215
 *   KNZ_T_RLT   RLT                  transform/RLT.cpp:39-221,247-369
 *   KNZ_T_LZ / KNZ_T_LZX   LZCodec -> LZXCodec<false> / LZXCodec<true>   transform/LZCodec.cpp:119-456,470-640
 *   KNZ_T_LZP   LZPCodec             transform/LZCodec.cpp:771-879,881-992
 *   KNZ_T_ROLZX ROLZCodec -> ROLZCodec2   transform/ROLZCodec.cpp:52-96,862-1109 (+ ROLZEncoder / ROLZDecoder :681-820, ROLZCodec.hpp:311-365)
 *   KNZ_T_EXE   EXECodec             transform/EXECodec.cpp:63-312,314-518 (+ detectType :520-625, parseHeader :627-849)
 *   KNZ_T_PACK  AliasCodec           transform/AliasCodec.cpp:38-209,211-371
 *   KNZ_T_DNA   AliasCodec with packOnlyDNA = 1 (TransformFactory.hpp:293-294): the forward refuses a preset type other than UNDEFINED
 *               or DNA (AliasCodec.cpp:66) and a block whose detection does not say DNA (:93); the inverse is PACK's
 *   KNZ_T_MM    FSDCodec             transform/FSDCodec.cpp:103-291,293-386
 *   KNZ_T_UTF   UTFCodec             transform/UTFCodec.cpp:48-204,206-298 (+ validate :303-422, pack / unpack UTFCodec.hpp:71-154)
 *   KNZ_T_TEXT  TextCodec -> TextCodec1 / TextCodec2   transform/TextCodec.cpp:520-1015,1017-1581 (+ statistics :213-425); entropy_type
 *               picks the encoding as TransformFactory.hpp:225-242 does (NONE, HUFFMAN, RANGE, ANS0: TextCodec2; TPAQX: TextCodec1 with
 *               a doubled hash map; anything else and -1: TextCodec1); the stream's block size is 0 here (knz_hip_transform_forward_bs)
 * (the inverse of LZ/LZX expects what the reference expects: two readable bytes behind `in + n`,
 * LZCodec.cpp:486-490; the library stages the input itself, so callers need not pad). */
KNZ_API int knz_hip_transform_forward(knz_ctx* ctx, int transform_type, const uint8_t* in, int32_t n,
                                      uint8_t* out, int32_t dst_cap, int entropy_type, int32_t* out_len, int32_t* ok);
KNZ_API int knz_hip_transform_inverse(knz_ctx* ctx, int transform_type, const uint8_t* in, int32_t n,
                                      uint8_t* out, int32_t dst_cap, int32_t* out_len, int32_t* ok);
/* The forward stage with the "dataType" entry of the block's Context (Global::DataType, 0 UNDEFINED .. 9 SMALL_ALPHABET, as in
 * knz_host_stages.reserved): *data_type goes in, and comes back as the stage left it. PACK refuses MULTIMEDIA, UTF8, EXE and
 * BIN and sets detectSimpleType's result on an UNDEFINED block; MM takes UNDEFINED, MULTIMEDIA and BIN blocks only and leaves
 * MULTIMEDIA once it has found a distance, or detectSimpleType's result of its samples when it has not; RLT refuses DNA, BASE64 and UTF8;
 * UTF takes UNDEFINED (it validates the block first) and UTF8 (it does not) and leaves UTF8 once validation has passed or been skipped,
 * also on a block it then refuses (too many symbols, a broken third byte, no gain); any other type makes it refuse and stays; ROLZX
 * takes every type (EXE: keys 3 bytes back; DNA: hashed 8-byte keys, matches of 7 and more) and sets detectSimpleType's result of the
 * whole block on an UNDEFINED one; EXE takes UNDEFINED, EXE and BIN blocks of 4,096 bytes and more, leaves EXE on a block it rewrites,
 * overwrites the type with what its detection found (UNDEFINED included) on a block that detection rejects, and leaves it alone on a
 * block it refuses for another reason (the gates; fewer than 16 rewritten addresses; more than 2 % of growth). EXE is the only stage
 * that produces the type EXE, which ROLZX reads and PACK refuses; TEXT takes UNDEFINED, TEXT and BIN blocks of 1,024 bytes and more,
 * leaves TEXT on a block its statistics call text (also when the encoding then outgrows the block) and the type they found -- DNA,
 * NUMERIC, BASE64, BIN, SMALL_ALPHABET, UTF8 or UNDEFINED -- on one they do not. The other stages ignore the type.
 * knz_hip_transform_forward is this call with a fresh Context (UNDEFINED). */
KNZ_API int knz_hip_transform_forward_dt(knz_ctx* ctx, int transform_type, const uint8_t* in, int32_t n, uint8_t* out,
                                         int32_t dst_cap, int entropy_type, int32_t* data_type, int32_t* out_len, int32_t* ok);
/* The same for a block of an older stream (bs_version as in knz_params: the BWT block header of versions below 6,
 * transform/BWTBlockCodec.cpp:140-164, and the LZ / LZX token layout, transform/LZCodec.cpp:614-760): what the transform
 * classes take from the "bsVersion" entry of their Context. */
KNZ_API int knz_hip_transform_inverse_v(knz_ctx* ctx, int transform_type, int bs_version, const uint8_t* in, int32_t n,
                                        uint8_t* out, int32_t dst_cap, int32_t* out_len, int32_t* ok);

/* The two calls with the block size of the stream the block belongs to (the "blockSize" entry of the Context) and, on the way back,
 * the stream's entropy id: TEXT sizes its hash map by the block size (TextCodec.cpp:533-541, 1030-1035; 0 = 8,192 slots) and picks its
 * encoding by the entropy id in both directions. The other stages ignore both. */
KNZ_API int knz_hip_transform_forward_bs(knz_ctx* ctx, int transform_type, uint32_t stream_block_size, const uint8_t* in, int32_t n,
                                         uint8_t* out, int32_t dst_cap, int entropy_type, int32_t* data_type, int32_t* out_len, int32_t* ok);
KNZ_API int knz_hip_transform_inverse_bs(knz_ctx* ctx, int transform_type, int bs_version, uint32_t stream_block_size, int entropy_type,
                                         const uint8_t* in, int32_t n, uint8_t* out, int32_t dst_cap, int32_t* out_len, int32_t* ok);

/* Device-memory helpers so that non-HIP hosts (ctypes, cgo, JNI) can stage data. */
KNZ_API int knz_hip_malloc(knz_ctx* ctx, size_t bytes, void** d_ptr);
KNZ_API int knz_hip_free(knz_ctx* ctx, void* d_ptr);
KNZ_API int knz_hip_memcpy_h2d(knz_ctx* ctx, void* d_dst, const void* src, size_t bytes);
KNZ_API int knz_hip_memcpy_d2h(knz_ctx* ctx, void* dst, const void* d_src, size_t bytes);
KNZ_API int knz_hip_sync(knz_ctx* ctx);
/* The same copies, queued on the context's copy streams (one per direction) and returning at once: they run beside the kernels
 * of a knz_hip_encode_blocks / knz_hip_decode_blocks call that another host thread has in flight (no context lock is taken), which
 * is how the stream classes overlap PCIe with compute. Host memory must be page-locked (knz_hip_host_alloc); the device buffer
 * must not be in use by a call in flight. knz_hip_copy_wait blocks until the copy behind `ticket` is complete (a ticket can be
 * waited for once; 0 and unknown tickets return at once). */
KNZ_API int knz_hip_memcpy_h2d_async(knz_ctx* ctx, void* d_dst, const void* src, size_t bytes, uint64_t* ticket);
KNZ_API int knz_hip_memcpy_d2h_async(knz_ctx* ctx, void* dst, const void* d_src, size_t bytes, uint64_t* ticket);
KNZ_API int knz_hip_copy_wait(knz_ctx* ctx, uint64_t ticket);
/* Page-locked host memory for staging buffers (what knz_hip_memcpy_h2d / _d2h move at full PCIe rate). */
KNZ_API int knz_hip_host_alloc(size_t bytes, void** ptr);
KNZ_API int knz_hip_host_free(void* ptr);

/* d_out = r zero bits (1..7) followed by the nbits bits of d_in (MSB-first byte streams, (r + nbits + 7) / 8 bytes written): what a
 * host that appends bit runs of independent batches in order needs (io/CompressedOutputStream.cpp:835-868 appends at bit granularity).
 * Queued on the context's stream. */
KNZ_API int knz_hip_shift_bits(knz_ctx* ctx, const uint8_t* d_in, uint64_t nbits, uint32_t r, uint8_t* d_out);

/* Timing of the kernels of the last encode/decode call, measured with HIP events on the context's
 * stream: name/ms pairs. Returns the number of entries written (<= cap). */
typedef struct { char name[48]; float ms; uint64_t launches; } knz_kernel_time;
KNZ_API int knz_hip_set_profiling(knz_ctx* ctx, int enabled);
KNZ_API int knz_hip_get_kernel_times(knz_ctx* ctx, knz_kernel_time* out, int cap);

/* Developer / test knobs, process-wide (the same names in upper case with a KNZ_ prefix are read from the environment once, when
 * the library first needs them): "bwt_nsym" (symbols of the suffix sort's first round, 0 = four or five by the data's entropy),
 * "bwt_no_run_round", "bwt_run_fallback" (1: force the general path for runs), "bwt_plain_labels" (32-bit labels, as blocks above
 * 256 MiB), "bwt_no_pack", "bwt_no_unsplit_skip" (medium groups whose keys are all equal stored and sorted like any other),
 * "bwt_no_group_sleep" (such groups gathered in every round, also where the round before already tells that no key will differ),
 * "bwt_no_medium_fuse" (medium groups' keys gathered by a kernel of their own, as with the 32-bit labels), "bwt_run_sort" (1: the run round's members generated and sorted instead of placed directly; also KNZ_BWT_RUN_SORT), "bwt_run_in_sort" (1: the run members go through round 0's sort instead of staying out of it; also KNZ_BWT_RUN_IN_SORT), "bwt_link" (0: the suffix sort's link step for groups inside long repeats off), "bwt_stats", "bwt_split" (parts of a batch the BWT stages run in, 1..4), "bwt_part_min" (fewest blocks per such part, default 2), "dec_parts" (block ranges a decode call runs side by side, 1..3), "rs_onesweep" (0: radix passes with a
 * counting kernel of their own), "lz_serial_decode" (1: LZ / LZX blocks decoded by one wave each), "mtf_tile" (0: MTFT tile size by
 * batch size, 1024 / 4096 force it), "mtf_chain" (1: MTFT forward ranks by the byte-serial kernel of rounds 2-4),
 * "bwt_inv_jump_all" (1: the inverse BWT ranks its rows by pointer jumping over all of them instead of the ruler walk: decodes the
 * blocks the ruler walk refuses), "bwt_inv_ruler_log" (one row in 2^k is a ruler, 2..8, anything else means 3), "bwt_inv_wide" (1: the
 * inverse BWT's 8-byte link records, as for blocks above 8 MiB, whatever the longest block of the batch is).
 * Returns 0, or -1 for an unknown name. No knob changes a result. */
KNZ_API int knz_hip_tune(const char* name, int value);

/* 1 when this library runs transform id `transform_type` as a device stage (in a chain and through the per-stage entry points), else 0.
 * libkanzi_amd.so asks it for KNZ_T_UTF to decide where UTF runs: against a device library without the stage, or from before this entry
 * point existed (it binds the symbol weakly), UTF stays among the host's leading stages as it used to. */
KNZ_API int knz_hip_transform_supported(int transform_type);

/* Test hook: q[i] = floor(d[i] / r[i]) by the RANGE decoder's reciprocal-based divide (host arrays; every pair must satisfy what the
 * decoder has checked before it divides: r >= 1 and d < r * 2^15). */
KNZ_API int knz_hip_range_divide(knz_ctx* ctx, const uint64_t* d, const uint64_t* r, uint32_t n, uint32_t* q);

/* Test hooks: the device-wide primitives of csrc/prims.hpp by themselves (prefix scans over 32-bit words, segmented stable LSD radix sort).
 * out[0..3] = keys per radix tile (RS_TILE), tiles per group of the column scan (RS_GROUP), words per scan tile (SC_TILE), passes the
 * one-read sort counts ahead (RS_MAXPASS): the sizes at which the kernels change path. Needs no context and no device. */
KNZ_API int knz_hip_prims_info(uint32_t out[4]);
/* op 0: d_out[i] = d_in[0] + .. + d_in[i-1] (wraps at 32 bits), 1: max of d_in[0..i], 2: min of d_in[0..i], for i < n, where
 * n = min(n_max, *d_n) when d_n (a device word) is given and n_max when it is NULL. d_in and d_out are device arrays of n_max words,
 * 16-byte aligned, and may be the same array; words of d_out from n on are left alone. d_total (device word, or NULL; op 0 only) receives
 * the sum of the n words -- 0 when *d_n is 0. n_max = 0 launches nothing and writes nothing. The scan's scratch is allocated by the call, which
 * runs on the context's stream and returns when the result is there. */
KNZ_API int knz_hip_prims_scan(knz_ctx* ctx, int op, const uint32_t* d_in, uint32_t* d_out, size_t n_max, const uint32_t* d_n, uint32_t* d_total);
/* Sorts every segment [d_seg_base[g], d_seg_base[g + 1]) (g < n_seg; d_seg_base[0] = 0, ascending, no segment longer than max_seg_len)
 * of the keys (key_bytes 4 or 8) stably on key bits [lo_bit, hi_bit), and moves d_vals (32-bit; NULL when has_val = 0) along.
 * one_read 1: one kernel per pass that learns the counts of the tiles in front of it by look-back (fails when the knob "rs_onesweep" is 0),
 * 0: a counting kernel, a column scan and a scatter per pass. keep 0: prims::rs_sort on a copy of the input; 1: prims::rs_sort_keep, which
 * reads the caller's arrays directly and must leave them as they are. The result always lands in d_keys_out / d_vals_out (no overlap with the
 * input). The call allocates the sort's workspace (exactly rs_ws_bytes of the key count and n_seg) and its ping-pong arrays with 4 KiB of
 * a fixed byte pattern in front of and behind each, and returns an error when a byte of a pattern has changed. It runs on the context's
 * stream and returns when the result is there. */
KNZ_API int knz_hip_prims_sort(knz_ctx* ctx, int key_bytes, int has_val, int keep, int one_read, const void* d_keys, const uint32_t* d_vals,
                               const uint32_t* d_seg_base, int n_seg, size_t max_seg_len, int lo_bit, int hi_bit, void* d_keys_out, uint32_t* d_vals_out);

/* Test hook: the sizes the TPAQ (extra = 0) / TPAQX (extra = 1) predictor takes for a block of block_len bytes (behind the
 * transforms) in a stream of block size stream_block_size, bitstream version 6: sizes[0..5] = bytes of the big states table, mixers,
 * words of the position hash, bytes of the ring buffer, contexts of the first and of the second SSE map. Needs no context and no device. */
KNZ_API int knz_hip_tpaq_params(uint32_t stream_block_size, uint32_t block_len, int extra, uint32_t sizes[6]);

#ifdef __cplusplus
}
#endif
#endif
