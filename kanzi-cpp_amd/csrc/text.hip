// TEXT (TextCodec, kanzi transform id 10) on gfx950, forward and inverse: the dictionary word coder in both of its encodings.
//
// Specification: host/text_codec.cpp (wordsForward / wordsInverse, pinned bit for bit to the reference by tests/test_host_text_utf.py),
// behind it transform/TextCodec.cpp. Codec 1 (indexes behind an escape byte) serves the entropy coders FPAQ, CM, TPAQ and "unset",
// with a doubled hash map for TPAQX; codec 2 (indexes with the top bit set) serves NONE, HUFFMAN, RANGE and ANS0.
//
// Forward. Only the dictionary is serial, and it is a function of the words, not of the bytes:
//   k_tx_f_head     refusals by size, capacity and preset type; clears the statistics
//   k_tx_stats      per chunk of 4,096 bytes: the byte histogram, the handful of pair counts blockFlags reads (CR / LF neighbours, "&a"
//                   "&g" "&l" "&q", pairs that UTF-8 forbids), and the number of lookup points of the chunk
//   k_tx_verdict    the flag byte or the non-text verdict with its data type (known before a byte is written), offsets of the chunks' words
//   k_tx_words      the lookup points in order: a delimiter behind a run of 2 to 31 letters (one u32 each, the delimiter's position)
//   k_tx_walk       one wave per block over the words in windows of 64: every lane hashes its word and looks it up speculatively; the
//                   window's puts are then applied in word order, and a later lane whose first or second slot was put or cleared in
//                   the window looks again. Leaves one u32 per word: the index it is replaced by, or 0
//   k_tx_emit<0/1>  every position knows its bytes (a literal with its escapes, nothing for a dropped CR, an implied space or the
//                   inside of a replaced word, the index bytes at a replaced word's first letter): counted per chunk, scanned, written.
//                   Every refusal of the host code is "an event at output offset o with o >= a bound that depends on the event",
//                   and o only grows, so the verdict is the OR over all positions of that test against the scanned offsets
//                   (Enc2::literals' `checked` shortcut only skips tests that cannot fail)
//   k_tx_f_final    ok, length, flag byte
// Dictionary::grow() makes every entry claim its slot again. Before the index wraps a put only happens into an empty slot, so that is
// a no-op for every slot but one: a put on a fresh entry clears slot[0 & mask] (the unused entry's hash is 0), so slot 0 alone is
// rebuilt at a grow, from the highest entry whose hash lands there (TxDict::zeroMax). After the wrap nothing grows any more.
//
// Inverse: one wave per block walks the tokens (the dictionary is rebuilt as it goes, its words point into the encoded block);
// letter runs, tail comparisons and word copies are wave-wide. The verdict depends on the capacity (the `room` tests, the initial
// dictionary size), so the last inverse stage of a stream judges by max(cap, capModel) and writes within cap, as UTF and EXE do.
//
// Scratch: text_scratch_bytes. Per block that runs at once: a hash map of 4 << logSlots bytes (logSlots from the stream's block
// size, 13 to 27), 2^18 or 2^19 entries of 16 bytes, two u32 per possible word (len / 3) and a few words per chunk; bounded by
// KNZ_TEXT_TABLES_MAX (bytes, default 4 GiB): a larger batch runs in slices. The maps are cleared on the stream by one memset per slice,
// the inverse zeroes its entries as its index grows; nothing synchronises.
#include "common.hpp"
#include "stages.hpp"
#include "datatype.hpp"
#include "magic.hpp"
#include "knz_hip.h"

#include <stdlib.h>

namespace knz {

namespace {

constexpr int TX_T = 256;                       // threads per workgroup
constexpr int TX_ROWS = 16;                     // positions per thread: position row * TX_T + thread of the chunk
constexpr u32 TX_CHUNK = TX_T * TX_ROWS;
constexpr u32 TX_HALO = 32;                     // bytes staged in front of a chunk (a word is at most 31 letters) or marked behind it
constexpr u32 TX_MIN = 1024, TX_MAX = 1u << 30;
constexpr u32 TX_H1 = 0x7FEB352Du, TX_H2 = 0x846CA68Bu;
constexpr u32 TX_MAX_WORD = 31, TX_MAX_ENTRIES = 1u << 19;
constexpr u32 TX_T1 = 128, TX_T2 = TX_T1 * TX_T1, TX_T3 = 64, TX_T4 = TX_T3 * 128;
constexpr u32 TX_ESC1 = 0x0F, TX_ESC2 = 0x0E, TX_CR = 0x0D, TX_LF = 0x0A, TX_SP = 0x20;
constexpr u32 TXF_NOT_TEXT = 0x80, TXF_CRLF = 0x40, TXF_XML = 0x20, TXF_CODEC2 = 0x10, TXF_TYPE = 0x0F;
constexpr u32 TX_NSTATIC = 1024;
constexpr u32 TX_POS_STATIC = 0x80000000u;      // entry text: an offset into tx_words
constexpr u32 TX_POS_ESC2 = 0xFFFFFFFEu, TX_POS_ESC1 = 0xFFFFFFFFu;      // codec 1's two one-byte entries

// per-block scratch (u32 words)
constexpr u32 TX_INFO = 0;                      // [32] TxInfo
constexpr u32 TX_STAT = 32;                     // [256] f0, then the counters below
constexpr u32 TXS_AMP = 256, TXS_CR_BAD = 257, TXS_LF_BAD = 258, TXS_UTF_BAD = 259, TXS_WORDS = 260 /* LDS only: lookup points of the chunk */, TXS_N = 264;
constexpr u32 TX_CH = TX_STAT + TXS_N;          // four arrays of chunks + 1: words per chunk, their offsets, output bytes per chunk, their offsets

struct TxInfo {
    u32 active;         // the block is text and is being encoded
    u32 codec1;
    u32 flags;
    u32 nWords;
    u32 fail;
    u32 logSlots;
};
static_assert(sizeof(TxInfo) <= 32 * 4, "TxInfo too large");

// the static dictionary: the project's own list, once for the table built at compile time and once as device data
constexpr char tx_words_c[] =
#include "../host/text_words_en.inc"
    ;
__device__ const char tx_words[] =
#include "../host/text_words_en.inc"
    ;

struct TxStaticTab { u32 hash[TX_NSTATIC]; u16 off[TX_NSTATIC]; u8 len[TX_NSTATIC]; u32 n; };
constexpr TxStaticTab tx_make_static()
{
    TxStaticTab t{};
    const u32 size = (u32)sizeof(tx_words_c) - 1;
    u32 at = 0, n = 0;
    while (at < size) {
        u32 e = at;
        while (e < size && tx_words_c[e] != ' ') e++;
        if (e > at) {
            u32 h = TX_H1;
            for (u32 i = at; i < e; i++) h = (h * TX_H1) ^ ((u32)(u8)tx_words_c[i] * TX_H2);
            if (n < TX_NSTATIC) { t.hash[n] = h; t.off[n] = (u16)at; t.len[n] = (u8)(e - at); }
            n++;
        }
        at = e + 1;
    }
    t.n = n;
    return t;
}
static_assert(tx_make_static().n == TX_NSTATIC, "the static dictionary has 1,024 words");
__device__ const TxStaticTab tx_static = tx_make_static();

__host__ __device__ inline u32 tx_chunks(u32 maxLen) { return maxLen / TX_CHUNK + 1; }
__host__ __device__ inline u32 tx_max_words(u32 maxLen) { return maxLen / 3 + 2; }
__host__ __device__ inline size_t tx_stride_u32(u32 maxLen)
{
    return (TX_CH + 4 * (size_t)(tx_chunks(maxLen) + 1) + 2 * (size_t)tx_max_words(maxLen) + 63) & ~(size_t)63;
}
__device__ __forceinline__ u32* tx_cnt(u32* ws) { return ws + TX_CH; }
__device__ __forceinline__ u32* tx_off(u32* ws, u32 maxLen) { return ws + TX_CH + (tx_chunks(maxLen) + 1); }
__device__ __forceinline__ u32* tx_ocnt(u32* ws, u32 maxLen) { return ws + TX_CH + 2 * (tx_chunks(maxLen) + 1); }
__device__ __forceinline__ u32* tx_ooff(u32* ws, u32 maxLen) { return ws + TX_CH + 3 * (tx_chunks(maxLen) + 1); }
__device__ __forceinline__ u32* tx_rec(u32* ws, u32 maxLen) { return ws + TX_CH + 4 * (size_t)(tx_chunks(maxLen) + 1); }
__device__ __forceinline__ u32* tx_res(u32* ws, u32 maxLen) { return tx_rec(ws, maxLen) + tx_max_words(maxLen); }

// entries of the dictionary of a block that can run: the index only grows past 2^18 entries when there are that many words
__host__ __device__ inline u32 tx_ent_cap(u32 maxLen) { return 2 * (1027 + (size_t)maxLen / 3) > (1u << 18) ? TX_MAX_ENTRIES : (1u << 18); }

__host__ __device__ inline bool tx_codec1_of(int entropyType)
{
    return !(entropyType == KNZ_E_NONE || entropyType == KNZ_E_HUFFMAN || entropyType == KNZ_E_RANGE || entropyType == KNZ_E_ANS0);
}
__host__ __device__ inline u32 tx_ilog2(u32 x) { u32 l = 0; while (x >>= 1) l++; return l; }
// Enc1::logSlots / Enc2::logSlots, and the doubled map the reference builds for TPAQX
__host__ __device__ inline u32 tx_log_slots(int entropyType, u32 blockSize)
{
    if (tx_codec1_of(entropyType)) {
        u32 l = 13;
        if (blockSize >= 8) { l = tx_ilog2(blockSize / 8); l = l > 26 ? 26 : (l < 13 ? 13 : l); }
        return l + (entropyType == KNZ_E_TPAQX ? 1 : 0);
    }
    u32 l = 13;
    if (blockSize >= 32) { l = tx_ilog2(blockSize / 32); l = l > 24 ? 24 : (l < 13 ? 13 : l); }
    return l;
}

__device__ __forceinline__ bool tx_letter(u32 c) { return ((c | 0x20u) - 'a') < 26u; }
// 0 letter, 1 delimiter, -1 anything else
__device__ __forceinline__ int tx_class(u32 c)
{
    if (tx_letter(c)) return 0;
    if ((c >= ' ' && c <= '/') || (c >= ':' && c <= '?')) return 1;
    if (c == '\n' || c == '\r' || c == '\t' || c == '_' || c == '|' || c == '{' || c == '}' || c == '[' || c == ']') return 1;
    return -1;
}
__device__ __forceinline__ u32 tx_hash_step(u32 h, u32 c) { return (h * TX_H1) ^ (c * TX_H2); }

// byte j of an entry's text
__device__ __forceinline__ u32 tx_text(const u8* src, u32 pos, u32 j)
{
    if (pos >= TX_POS_ESC2) return pos == TX_POS_ESC1 ? TX_ESC1 : TX_ESC2;
    if (pos & TX_POS_STATIC) return (u32)(u8)tx_words[(pos & 0x7FFFFFFFu) + j];
    return ldg<u8>(src + pos + j);
}

// ---------------------------------------------------------------------------------------------------------------------
// the dictionary of one block, held by one wave: every field is the same in all lanes, lane 0 stores
// ---------------------------------------------------------------------------------------------------------------------
struct TxDict {
    u32* slot;          // hash & mask -> entry + 1, 0 = empty
    uint4* ent;         // hash, text, length, -
    u32 mask, fixed, size, at, wrapped, cap;
    u32 clear;          // the inverse: entries are zeroed as the index takes them in (a damaged block may name one no word has taken)
    int zeroMax;        // highest entry whose hash lands in slot 0 (what a grow leaves there), -1 = none
    u32 broken;         // the index would outgrow its memory (cannot happen by text_scratch_bytes' bound; refused rather than written)
};

__device__ void tx_dict_init(TxDict& d, u32* slot, uint4* ent, u32 cap, u32 logSlots, u32 count, bool escapes, bool clear, int lane)
{
    d.slot = slot; d.ent = ent; d.cap = cap; d.clear = clear ? 1u : 0u;
    d.mask = (1u << logSlots) - 1u;
    d.fixed = TX_NSTATIC + (escapes ? 2u : 0u);
    u32 lg = 13;
    if (count >= 1024) { lg = tx_ilog2(count / 128); lg = lg > 18 ? 18 : (lg < 13 ? 13 : lg); }
    d.size = 1u << lg;
    d.at = d.fixed; d.wrapped = 0; d.broken = d.size > cap ? 1u : 0u;
    // (the later of two static words that share a slot keeps it: the highest index wins)
    for (u32 i = (u32)lane; i < TX_NSTATIC; i += 64) {
        ent[i] = make_uint4(tx_static.hash[i], TX_POS_STATIC | tx_static.off[i], tx_static.len[i], 0);
        atomicMax(&slot[tx_static.hash[i] & d.mask], i + 1);
    }
    if (clear && !d.broken) for (u32 i = d.fixed + (u32)lane; i < d.size; i += 64) ent[i] = make_uint4(0, 0, 0, 0);
    if (escapes && lane == 0) {
        ent[TX_NSTATIC] = make_uint4(0, TX_POS_ESC2, 1, 0);
        ent[TX_NSTATIC + 1] = make_uint4(0, TX_POS_ESC1, 1, 0);
        atomicMax(&slot[0], TX_NSTATIC + 2);
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    KNZ_WAVE_ORDER();
    d.zeroMax = (int)slot[0] - 1;
}

// Dictionary::put. Returns the slot that was cleared; grew: the index doubled and slot 0 was rebuilt.
__device__ u32 tx_put(TxDict& d, u32 pos, u32 len, u32 h, int lane, bool& grew)
{
    const u32 sc = d.wrapped ? (d.ent[d.at].x & d.mask) : 0u;       // (a fresh entry's hash is 0)
    KNZ_WAVE_ORDER();                                               // (every lane has read the old entry and the slots before lane 0 stores)
    if (lane == 0) {
        d.slot[sc] = 0;
        d.ent[d.at] = make_uint4(h, pos, len, 0);
        d.slot[h & d.mask] = d.at + 1;
    }
    if (!d.wrapped && (h & d.mask) == 0) d.zeroMax = (int)d.at;
    d.at++;
    grew = false;
    if (d.at >= d.size) {
        if (d.size < TX_MAX_ENTRIES) {
            if (2 * d.size > d.cap) { d.broken = 1; d.at = d.fixed; }
            else {
                if (d.clear) for (u32 i = d.size + (u32)lane; i < 2 * d.size; i += 64) d.ent[i] = make_uint4(0, 0, 0, 0);
                d.size *= 2;
                if (lane == 0) d.slot[0] = (u32)(d.zeroMax + 1);
                grew = true;
            }
        } else { d.at = d.fixed; d.wrapped = 1; }
    }
    return sc;
}

// ---------------------------------------------------------------------------------------------------------------------
// forward
// ---------------------------------------------------------------------------------------------------------------------

// bytes [c0 - before, c0 + TX_CHUNK) of the block at sb[0 ..]; zero outside the block
__device__ void tx_stage(u8* sb, const u8* __restrict__ src, u32 c0, u32 before, u32 n)
{
    for (u32 i = threadIdx.x; i < before + TX_CHUNK; i += TX_T) {
        const long long p = (long long)c0 - before + i;
        sb[i] = (p >= 0 && p < (long long)n) ? ldg<u8>(src + p) : (u8)0;
    }
    __syncthreads();
}

// whether the delimiter at sb[i] is a lookup point: a run of 2 to 31 letters right in front of it (wordsForward: i > delim + 2 && t > 0,
// len <= MAX_WORD; the byte in front of the block is no letter)
__device__ __forceinline__ bool tx_lookup_point(const u8* sb, u32 i)
{
    if (tx_class(sb[i]) != 1) return false;
    u32 L = 0;
    while (L <= TX_MAX_WORD && tx_letter(sb[i - 1 - L])) L++;
    return L >= 2 && L <= TX_MAX_WORD;
}

__global__ __launch_bounds__(TX_T) void k_tx_f_head(XfStage st, u32* scratch, size_t stride, int b0)
{
    const int b = b0 + (int)blockIdx.x;
    u32* ws = scratch + (size_t)blockIdx.x * stride;
    for (u32 i = threadIdx.x; i < TXS_N; i += TX_T) ws[TX_STAT + i] = 0u;
    if (threadIdx.x != 0) return;
    TxInfo* info = reinterpret_cast<TxInfo*>(ws + TX_INFO);
    const u32 count = st.len[b];
    TxInfo o = {};
    st.ok[b] = count == 0 ? 1 : 0;
    st.newLen[b] = 0;
    const u32 dt = st.dtype ? st.dtype[b] : (u32)DT_UNDEFINED;
    if (count >= TX_MIN && count <= TX_MAX && st.cap[b] >= count && (dt == DT_UNDEFINED || dt == DT_TEXT || dt == DT_BIN)) {
        o.active = 1;
        o.codec1 = tx_codec1_of(st.entropyType) ? 1u : 0u;
        o.logSlots = tx_log_slots(st.entropyType, st.blockSize);
    }
    *info = o;
}

__global__ __launch_bounds__(TX_T) void k_tx_stats(XfStage st, u32* scratch, size_t stride, int b0)
{
    const int b = b0 + (int)blockIdx.y;
    u32* ws = scratch + (size_t)blockIdx.y * stride;
    const TxInfo* info = reinterpret_cast<const TxInfo*>(ws + TX_INFO);
    if (!info->active) return;
    const u32 n = st.len[b], c0 = blockIdx.x * TX_CHUNK;
    if (c0 >= n) { if (threadIdx.x == 0) tx_cnt(ws)[blockIdx.x] = 0; return; }
    __shared__ u8 sb[TX_HALO + TX_CHUNK];
    __shared__ u32 hist[TXS_N];
    for (u32 i = threadIdx.x; i < TXS_N; i += TX_T) hist[i] = 0u;
    tx_stage(sb, st.src[b], c0, TX_HALO, n);
    u32 amp = 0, crBad = 0, lfBad = 0, utfBad = 0, words = 0;
    for (int r = 0; r < TX_ROWS; r++) {
        const u32 i = TX_HALO + r * TX_T + threadIdx.x, p = c0 + r * TX_T + threadIdx.x;
        if (p >= n) break;
        const u32 c = sb[i], q = sb[i - 1];                        // (the byte in front of the block counts as 0)
        atomicAdd(&hist[c], 1u);
        if (q == '&' && (c == 'a' || c == 'g' || c == 'l' || c == 'q')) amp++;
        if (q == TX_CR && c != TX_LF) crBad++;
        if (c == TX_LF && q != TX_CR) lfBad++;
        // pairs that UTF-8 forbids (looksLikeUtf8): a lead byte followed by something outside its range
        if (q >= 0xC2 && q <= 0xF4) {
            const u32 lo = q == 0xE0 ? 0xA0u : (q == 0xF0 ? 0x90u : 0x80u), hi = q == 0xED ? 0x9Fu : (q == 0xF4 ? 0x8Fu : 0xBFu);
            if (c < lo || c > hi) utfBad++;
        }
        if (tx_lookup_point(sb, i)) words++;
    }
    if (amp) atomicAdd(&hist[TXS_AMP], amp);
    if (crBad) atomicAdd(&hist[TXS_CR_BAD], crBad);
    if (lfBad) atomicAdd(&hist[TXS_LF_BAD], lfBad);
    if (utfBad) atomicAdd(&hist[TXS_UTF_BAD], utfBad);
    if (words) atomicAdd(&hist[TXS_WORDS], words);
    __syncthreads();
    u32* stat = ws + TX_STAT;
    for (u32 i = threadIdx.x; i < TXS_WORDS; i += TX_T) if (hist[i]) atomicAdd(&stat[i], hist[i]);
    if (threadIdx.x == 0) tx_cnt(ws)[blockIdx.x] = hist[TXS_WORDS];
}

// exclusive prefix sums of in[0 .. m) into out[0 .. m], by one workgroup; returns the total
__device__ u32 tx_scan_array(const u32* in, u32* out, u32 m, u32* sh /* [4] */)
{
    const int lane = lane_id(), wave = (int)(threadIdx.x >> 6);
    u32 run = 0;
    for (u32 base = 0; base < m; base += TX_T) {
        const u32 i = base + threadIdx.x;
        const u32 v = i < m ? in[i] : 0u;
        const u32 incl = wave_incl_scan(v);
        if (lane == 63) sh[wave] = incl;
        __syncthreads();
        u32 carry = 0, tot = 0;
        for (int w = 0; w < TX_T / 64; w++) { if (w < wave) carry += sh[w]; tot += sh[w]; }
        if (i < m) out[i] = run + carry + incl - v;
        run += tot;
        __syncthreads();
    }
    if (threadIdx.x == 0) out[m] = run;
    return run;
}

// TextCodec's block statistics (blockFlags of host/text_codec.cpp): F_NOT_TEXT | type, or F_CRLF / F_XML for text
__device__ u32 tx_block_flags(const u8* src, u32 n, const u32* f0, bool strict)
{
    if (!strict && knz_magic::magic_of(src) != 0) return TXF_NOT_TEXT;
    const int N = (int)n;
    int letters = (int)(f0[TX_CR] + f0[TX_LF]), ascii = 0;
    for (u32 c = 0; c < 128; c++) { if (tx_letter(c)) letters += (int)f0[c]; ascii += (int)f0[c]; }
    const int high = N - ascii;
    bool notText = high > (N >> 2);
    if (!notText) {
        notText = letters < (N >> 2);
        if (strict) notText |= (f0[0] >= (u32)(N / 100)) || ((ascii / 95) < (N / 100));
        else notText |= f0[TX_SP] < (u32)(N / 50);
    }
    if (notText) {
        const int t = pk_simple_type(n, f0);
        if (t != DT_UNDEFINED) return TXF_NOT_TEXT | (u32)t;
        u32 bad = f0[0xC0] + f0[0xC1] + f0[TXS_UTF_BAD], cont = 0;
        for (u32 c = 0xF5; c <= 0xFF; c++) bad += f0[c];
        for (u32 c = 0x80; c <= 0xBF; c++) cont += f0[c];
        return (bad == 0 && cont >= (u32)(N / 8)) ? (TXF_NOT_TEXT | (u32)DT_UTF8) : TXF_NOT_TEXT;
    }
    u32 res = 0;
    if (high <= N - N / 10) {
        const int lt = (int)f0['<'], gt = (int)f0['>'], amp = (int)f0[TXS_AMP];
        const int least = max((N - high) >> 9, 2);
        if (lt >= least && gt >= least && amp > 0) {
            if (lt < gt) { if (lt >= gt - gt / 100) res |= TXF_XML; }
            else if (gt < lt) { if (gt >= lt - lt / 100) res |= TXF_XML; }
            else res |= TXF_XML;
        }
    }
    if (f0[TX_CR] != 0 && f0[TX_CR] == f0[TX_LF] && f0[TXS_CR_BAD] == 0 && f0[TXS_LF_BAD] == 0) res |= TXF_CRLF;
    return res;
}

__global__ __launch_bounds__(TX_T) void k_tx_verdict(XfStage st, u32* scratch, size_t stride, int b0)
{
    const int b = b0 + (int)blockIdx.x;
    u32* ws = scratch + (size_t)blockIdx.x * stride;
    TxInfo* info = reinterpret_cast<TxInfo*>(ws + TX_INFO);
    if (!info->active) return;
    __shared__ u32 sh[4];
    const u32 n = st.len[b];
    const u32 total = tx_scan_array(tx_cnt(ws), tx_off(ws, st.maxLen), n / TX_CHUNK + 1, sh);
    if (threadIdx.x != 0) return;
    const u32* stat = ws + TX_STAT;
    const u32 flags = tx_block_flags(st.src[b], n, stat, info->codec1 != 0);
    if (flags & TXF_NOT_TEXT) {
        if (st.dtype) st.dtype[b] = (u8)(flags & TXF_TYPE);
        info->active = 0;
        return;
    }
    if (st.dtype) st.dtype[b] = DT_TEXT;
    info->flags = flags;
    info->nWords = total;
}

// position-ordered exclusive offsets inside a chunk: v[r] belongs to position r * TX_T + thread. tot: [TX_ROWS * 4 + 1] in LDS,
// tot[TX_ROWS * 4] is left holding the chunk's total
__device__ void tx_chunk_scan(const u32 (&v)[TX_ROWS], u32 (&off)[TX_ROWS], u32* tot)
{
    const int lane = lane_id(), wave = (int)(threadIdx.x >> 6);
    for (int r = 0; r < TX_ROWS; r++) {
        const u32 incl = wave_incl_scan(v[r]);
        off[r] = incl - v[r];
        if (lane == 63) tot[r * 4 + wave] = incl;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        u32 run = 0;
        for (int k = 0; k < TX_ROWS * 4; k++) { const u32 x = tot[k]; tot[k] = run; run += x; }
        tot[TX_ROWS * 4] = run;
    }
    __syncthreads();
    for (int r = 0; r < TX_ROWS; r++) off[r] += tot[r * 4 + wave];
}

__global__ __launch_bounds__(TX_T) void k_tx_words(XfStage st, u32* scratch, size_t stride, int b0)
{
    const int b = b0 + (int)blockIdx.y;
    u32* ws = scratch + (size_t)blockIdx.y * stride;
    const TxInfo* info = reinterpret_cast<const TxInfo*>(ws + TX_INFO);
    if (!info->active) return;
    const u32 n = st.len[b], c0 = blockIdx.x * TX_CHUNK;
    if (c0 >= n) return;
    __shared__ u8 sb[TX_HALO + TX_CHUNK];
    __shared__ u32 tot[TX_ROWS * 4 + 1];
    tx_stage(sb, st.src[b], c0, TX_HALO, n);
    u32 v[TX_ROWS], off[TX_ROWS];
    for (int r = 0; r < TX_ROWS; r++) {
        const u32 p = c0 + r * TX_T + threadIdx.x;
        v[r] = (p < n && tx_lookup_point(sb, TX_HALO + r * TX_T + threadIdx.x)) ? 1u : 0u;
    }
    tx_chunk_scan(v, off, tot);
    u32* rec = tx_rec(ws, st.maxLen) + tx_off(ws, st.maxLen)[blockIdx.x];
    for (int r = 0; r < TX_ROWS; r++) if (v[r]) rec[off[r]] = c0 + r * TX_T + threadIdx.x;
}

// One wave per block: the words against the dictionary, in windows of 64.
__global__ __launch_bounds__(64) void k_tx_walk(XfStage st, u32* scratch, size_t stride, u8* slots, u8* ents, size_t slotBytes, u32 entCap, int b0)
{
    const int b = b0 + (int)blockIdx.x, lane = lane_id();
    u32* ws = scratch + (size_t)blockIdx.x * stride;
    TxInfo* info = reinterpret_cast<TxInfo*>(ws + TX_INFO);
    if (!info->active) return;
    const u8* __restrict__ src = st.src[b];
    const u32 n = st.len[b], nWords = info->nWords;
    TxDict d;
    tx_dict_init(d, reinterpret_cast<u32*>(slots + (size_t)blockIdx.x * slotBytes), reinterpret_cast<uint4*>(ents) + (size_t)blockIdx.x * entCap, entCap,
                 info->logSlots, n, info->codec1 != 0, false, lane);
    const u32* rec = tx_rec(ws, st.maxLen);
    u32* res = tx_res(ws, st.maxLen);
    for (u32 w0 = 0; w0 < nWords; w0 += 64) {
        const u32 k = w0 + (u32)lane;
        const bool valid = k < nWords;
        u32 L = 0, start = 0, h = TX_H1, hf = TX_H1;
        if (valid) {
            const u32 e = rec[k];
            while (L <= TX_MAX_WORD && L < e && tx_letter(ldg<u8>(src + e - 1 - L))) L++;
            start = e - L;
            for (u32 j = 0; j < L; j++) {
                const u32 c = ldg<u8>(src + start + j);
                h = tx_hash_step(h, c);
                hf = tx_hash_step(hf, j == 0 ? (c ^ 0x20u) : c);
            }
        }
        const u32 a1 = h & d.mask, a2 = hf & d.mask;
        unsigned long long pending = __ballot(valid), dirty = pending;
        u32 r = 0;
        bool want = false;
        while (pending) {
            if ((dirty >> lane) & 1) {
                const int s1 = (int)d.slot[a1] - 1;
                int hit = -1;
                u32 pos = 0;
                bool first = false;
                if (s1 >= 0) { const uint4 e = d.ent[s1]; if (e.x == h && e.z == L) { hit = s1; pos = e.y; first = true; } }
                if (!first) {
                    const int s2 = (int)d.slot[a2] - 1;
                    if (s2 >= 0) { const uint4 e = d.ent[s2]; if (e.x == hf && e.z == L) { hit = s2; pos = e.y; } }
                }
                if (hit >= 0)
                    for (u32 j = 1; j < L; j++) if (tx_text(src, pos, j) != ldg<u8>(src + start + j)) { hit = -1; break; }
                r = hit >= 0 ? (0x80000000u | (hit != s1 ? 0x40000000u : 0u) | (L << 20) | (u32)hit) : 0u;
                want = hit < 0 && s1 < 0 && L >= 3;
            }
            dirty = 0;
            const unsigned long long putMask = __ballot(want);
            for (;;) {
                const unsigned long long pm = putMask & pending, dm = dirty & pending;
                const u32 stopPut = pm ? (u32)__ffsll((long long)pm) - 1 : 64u, stopDirty = dm ? (u32)__ffsll((long long)dm) - 1 : 64u;
                const u32 stop = stopPut < stopDirty ? stopPut : stopDirty;
                pending = stop >= 64 ? 0ull : (pending & ~((1ull << stop) - 1ull));      // everything in front of `stop` stands
                if (stop >= 64 || stop == stopDirty) break;
                const u32 Lq = (u32)__shfl((int)L, (int)stop), hq = (u32)__shfl((int)h, (int)stop), sq = (u32)__shfl((int)start, (int)stop);
                if (Lq > 3 || d.at < TX_T2) {
                    bool grew;
                    const u32 sc = tx_put(d, sq, Lq, hq, lane, grew), sp = hq & d.mask;
                    const bool again = ((pending >> lane) & 1) && (u32)lane > stop
                                    && (a1 == sp || a2 == sp || a1 == sc || a2 == sc || (grew && (a1 == 0 || a2 == 0)));
                    dirty |= __ballot(again);
                }
                pending &= ~(1ull << stop);
            }
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            KNZ_WAVE_ORDER();
        }
        if (valid) res[k] = r;
    }
    if (d.broken && lane == 0) info->fail = 1;
}

template <bool C1> __device__ __forceinline__ u32 tx_ref_bytes(u32 r, u8* o4)
{
    const bool flipped = (r & 0x40000000u) != 0;
    u32 v = r & 0x7FFFFu, k = 0;
    if (C1) {
        o4[k++] = (u8)(flipped ? TX_ESC2 : TX_ESC1);
        if (v >= TX_T1) {
            if (v >= TX_T2) { o4[k++] = (u8)(0xE0 | (v >> 14)); o4[k++] = (u8)(0x80 | (v >> 7)); o4[k++] = (u8)(0x7F & v); }
            else { o4[k++] = (u8)(0x80 | (v >> 7)); o4[k++] = (u8)(0x7F & v); }
        } else o4[k++] = (u8)v;
    } else {
        if (flipped) o4[k++] = 0x80;
        v++;
        if (v >= TX_T3) {
            if (v >= TX_T4) { o4[k++] = (u8)(0xF0 | (v >> 16)); o4[k++] = (u8)(v >> 8); o4[k++] = (u8)v; }
            else { o4[k++] = (u8)(0xC0 | (v >> 8)); o4[k++] = (u8)v; }
        } else o4[k++] = (u8)(0x80 | v);
    }
    return k;
}

// What position idx of the chunk writes (o4, returns the size) and the bound its output offset has to stay below (0xFFFFFFFF: no test)
template <bool C1> __device__ __forceinline__ u32 tx_position(const u8* sb, const u8* mark, const u32* refv, u32 idx, bool crlf, u32 R, u8* o4, u32& bound)
{
    const u32 c = sb[idx], m = mark[idx];
    bound = 0xFFFFFFFFu;
    if (m & 1) {
        if (!(m & 4)) return 0;
        bound = R - (C1 ? 4u : 3u);
        return tx_ref_bytes<C1>(refv[idx], o4);
    }
    if (c == TX_SP && (m & 2) && (mark[idx + 1] & 4)) return 0;       // a single space between two word references is implied
    if (C1) {
        bound = R;
        if (c == TX_ESC1 || c == TX_ESC2) {
            const u32 v = TX_NSTATIC + (c == TX_ESC1 ? 1u : 0u);      // fixed - 1 / fixed - 2: two index bytes
            o4[0] = (u8)TX_ESC1; o4[1] = (u8)(0x80 | (v >> 7)); o4[2] = (u8)(0x7F & v);
            bound = R - 3;
            return 3;
        }
        if (c == TX_CR && crlf) return 0;                             // (dropped, but Enc1::literals tests the room first)
        o4[0] = (u8)c;
        return 1;
    }
    if (c == TX_ESC1) { o4[0] = o4[1] = (u8)TX_ESC1; bound = R - 1; return 2; }
    if (c == TX_CR && crlf) return 0;
    if (c >= 128) { o4[0] = (u8)TX_ESC1; o4[1] = (u8)c; bound = R - 1; return 2; }
    o4[0] = (u8)c; bound = R;
    return 1;
}

template <bool C1, bool WRITE>
__device__ void tx_emit_body(const XfStage& st, int b, u32* ws, TxInfo* info, u8* sb, u8* mark, u32* refv, u32* tot)
{
    const u32 n = st.len[b], c0 = blockIdx.x * TX_CHUNK, c1 = c0 + TX_CHUNK;
    tx_stage(sb, st.src[b], c0, 0, n);
    for (u32 i = threadIdx.x; i < TX_CHUNK + TX_HALO + 1; i += TX_T) mark[i] = 0;
    __syncthreads();
    // the replaced words that touch [c0, c1 + TX_HALO]: the chunk's own (by their delimiter) and the first few behind it
    const u32* off = tx_off(ws, st.maxLen);
    const u32* rec = tx_rec(ws, st.maxLen);
    const u32* res = tx_res(ws, st.maxLen);
    const u32 k0 = off[blockIdx.x], k1 = off[blockIdx.x + 1], nWords = info->nWords;
    for (u32 k = k0 + threadIdx.x; k < k1 + 16 && k < nWords; k += TX_T) {
        const u32 e = rec[k], r = res[k];
        if (r == 0 || e > c1 + TX_HALO - 1) continue;
        const u32 L = (r >> 20) & 31u, start = e - L;
        for (u32 p = start > c0 ? start : c0; p < e; p++) mark[p - c0] |= 1;
        if (start >= c0) { mark[start - c0] |= 4; refv[start - c0] = r; }
        mark[e - c0] |= 2;
    }
    __syncthreads();
    const bool crlf = (info->flags & TXF_CRLF) != 0;
    u32 v[TX_ROWS], o[TX_ROWS];
    for (int r = 0; r < TX_ROWS; r++) {
        const u32 idx = r * TX_T + threadIdx.x;
        u8 o4[4]; u32 bound;
        v[r] = c0 + idx < n ? tx_position<C1>(sb, mark, refv, idx, crlf, n, o4, bound) : 0u;
    }
    tx_chunk_scan(v, o, tot);
    if (!WRITE) { if (threadIdx.x == 0) tx_ocnt(ws, st.maxLen)[blockIdx.x] = tot[TX_ROWS * 4]; return; }
    const u32 base = 1 + tx_ooff(ws, st.maxLen)[blockIdx.x], cap = st.cap[b];
    u8* dst = st.dst[b];
    bool fail = false;
    for (int r = 0; r < TX_ROWS; r++) {
        const u32 idx = r * TX_T + threadIdx.x;
        if (c0 + idx >= n) break;
        u8 o4[4]; u32 bound;
        const u32 sz = tx_position<C1>(sb, mark, refv, idx, crlf, n, o4, bound);
        const u32 at = base + o[r];
        if (bound != 0xFFFFFFFFu && at >= bound) { fail = true; continue; }
        if (at + sz > cap) { fail = true; continue; }
        for (u32 j = 0; j < sz; j++) stg<u8>(dst + at + j, o4[j]);
    }
    if (fail) atomicOr(&info->fail, 1u);
}

template <bool WRITE>
__global__ __launch_bounds__(TX_T) void k_tx_emit(XfStage st, u32* scratch, size_t stride, int b0)
{
    const int b = b0 + (int)blockIdx.y;
    u32* ws = scratch + (size_t)blockIdx.y * stride;
    TxInfo* info = reinterpret_cast<TxInfo*>(ws + TX_INFO);
    if (!info->active) return;
    if (blockIdx.x * TX_CHUNK >= st.len[b]) { if (!WRITE && threadIdx.x == 0) tx_ocnt(ws, st.maxLen)[blockIdx.x] = 0; return; }
    __shared__ u8 sb[TX_CHUNK];
    __shared__ u8 mark[TX_CHUNK + TX_HALO + 4];
    __shared__ u32 refv[TX_CHUNK + TX_HALO];
    __shared__ u32 tot[TX_ROWS * 4 + 1];
    if (info->codec1) tx_emit_body<true, WRITE>(st, b, ws, info, sb, mark, refv, tot);
    else tx_emit_body<false, WRITE>(st, b, ws, info, sb, mark, refv, tot);
}

__global__ __launch_bounds__(TX_T) void k_tx_oscan(XfStage st, u32* scratch, size_t stride, int b0)
{
    const int b = b0 + (int)blockIdx.x;
    u32* ws = scratch + (size_t)blockIdx.x * stride;
    const TxInfo* info = reinterpret_cast<const TxInfo*>(ws + TX_INFO);
    if (!info->active) return;
    __shared__ u32 sh[4];
    tx_scan_array(tx_ocnt(ws, st.maxLen), tx_ooff(ws, st.maxLen), st.len[b] / TX_CHUNK + 1, sh);
}

__global__ __launch_bounds__(64) void k_tx_f_final(XfStage st, u32* scratch, size_t stride, int b0, int nb)
{
    const int i = (int)(blockIdx.x * 64 + threadIdx.x);
    if (i >= nb) return;
    const int b = b0 + i;
    u32* ws = scratch + (size_t)i * stride;
    const TxInfo* info = reinterpret_cast<const TxInfo*>(ws + TX_INFO);
    if (!info->active) return;
    const u32 total = 1 + tx_ooff(ws, st.maxLen)[st.len[b] / TX_CHUNK + 1];
    const bool ok = !info->fail && total <= st.cap[b];
    st.ok[b] = ok ? 1 : 0;
    st.newLen[b] = ok ? total : 0u;
    if (!ok) return;
    stg<u8>(st.dst[b], (u8)info->flags);      // (bitstream versions 7 and up would name the codec here; the library writes and reads up to 6)
}

// ---------------------------------------------------------------------------------------------------------------------
// inverse (wordsInverse of host/text_codec.cpp, statement for statement; every value but `lane` is the same in all lanes)
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void k_tx_inverse(XfStage st, u8* slots, u8* ents, size_t slotBytes, u32 entCap, int b0)
{
    const int b = b0 + (int)blockIdx.x, lane = lane_id();
    const u32 count = st.len[b];
    if (lane == 0) { st.ok[b] = count == 0 ? 1 : 0; st.newLen[b] = 0; }
    if (count < 2 || count > TX_MAX) return;
    const u8* __restrict__ src = st.src[b];
    u8* dst = st.dst[b];
    const bool esc = tx_codec1_of(st.entropyType);
    const u32 cap = st.cap[b], room = cap > st.capModel ? cap : st.capModel;
    TxDict d;
    const u32 logSlots = tx_log_slots(st.entropyType, st.blockSize);
    tx_dict_init(d, reinterpret_cast<u32*>(slots + (size_t)blockIdx.x * slotBytes), reinterpret_cast<uint4*>(ents) + (size_t)blockIdx.x * entCap, entCap,
                 logSlots, room, esc, true, lane);
    const bool crlf = (ldg<u8>(src) & TXF_CRLF) != 0;
    const bool oldIndexes = !esc && st.bsVersion < 6;
    const u32 end = count;
    u32 i = 1, o = 0;
    int delim = tx_letter(ldg<u8>(src + 1)) ? 0 : 1;
    bool afterWord = false, ok = d.broken == 0;
    auto rd = [src, end](u32 k) -> u32 { return k < end ? (u32)ldg<u8>(src + k) : 0u; };      // nothing is read behind src[end - 1]
    while (ok && i < end && o < room) {
        u32 c = ldg<u8>(src + i);
        const int t = tx_class(c);
        if (t == 0) {
            // a run of letters, 64 at a time
            const u32 p = i + (u32)lane;
            const unsigned long long m = __ballot(p < end && tx_letter(ldg<u8>(src + (p < end ? p : i))));
            u32 run = ~m ? (u32)__ffsll((long long)~m) - 1 : 64u;
            if (run > room - o) run = room - o;
            if (o + run > cap) { ok = false; break; }
            if ((u32)lane < run) stg<u8>(dst + o + lane, ldg<u8>(src + p));
            i += run; o += run;
            continue;
        }
        if ((int)i > delim + 3 && t > 0) {
            const u32 len = i - (u32)delim - 1;
            if (len <= TX_MAX_WORD) {
                const u32 wpos = (u32)delim + 1;
                const u32 wb = (u32)lane < len ? (u32)ldg<u8>(src + wpos + lane) : 0u;
                u32 h = TX_H1;
                for (u32 j = 0; j < len; j++) h = tx_hash_step(h, (u32)__shfl((int)wb, (int)j));
                const int s1 = (int)d.slot[h & d.mask] - 1;
                bool known = false;
                if (s1 >= 0) {
                    const uint4 e = d.ent[s1];
                    if (e.x == h && e.z == len) {
                        const bool differs = lane >= 1 && (u32)lane < len && tx_text(src, e.y, (u32)lane) != wb;
                        known = __ballot(differs) == 0;
                    }
                }
                if (!known && (len > 3 || d.at < TX_T2) && s1 < 0) {
                    bool grew;
                    tx_put(d, wpos, len, h, lane, grew);
                    if (d.broken) { ok = false; break; }
                    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
                    KNZ_WAVE_ORDER();
                }
            }
        }
        i++;
        bool isRef;
        u32 flip = 0, idx = 0;
        if (esc) {
            isRef = c == TX_ESC1 || c == TX_ESC2;
            if (isRef) {
                idx = rd(i++);
                if (idx >= 128) {
                    const u32 b2 = rd(i++);
                    if (b2 >= 128) { idx = ((idx & 0x1F) << 14) | ((b2 & 0x7F) << 7) | rd(i); i++; }
                    else idx = ((idx & 0x7F) << 7) | b2;
                    if (idx >= d.size) { ok = false; break; }
                }
                if (c == TX_ESC2) flip = 0x20;
            }
        } else {
            isRef = c >= 0x80;
            if (isRef) {
                if (oldIndexes) {
                    flip = c & 0x20;
                    idx = c & 0x1F;
                    if (c & 0x40) {
                        const u32 b2 = rd(i++);
                        if (b2 >= 128) { idx = (idx << 14) | ((b2 & 0x7F) << 7) | rd(i); i++; }
                        else idx = (idx << 7) | b2;
                        if (idx >= d.size) { ok = false; break; }
                    }
                } else {
                    if (c == 0x80) { flip = 0x20; c = rd(i++); }
                    idx = c & 0x7F;
                    if (idx >= 64) {
                        if (idx >= 112) { idx = ((idx & 0x0F) << 16) | (rd(i) << 8) | rd(i + 1); i += 2; }
                        else { idx = ((idx & 0x1F) << 8) | rd(i); i++; }
                        if (idx > d.size) { ok = false; break; }
                    }
                    if (idx == 0) { ok = false; break; }             // (index 0 names no word in any of its encodings)
                    idx--;
                }
            }
        }
        if (isRef) {
            const uint4 e = d.ent[idx];
            const u32 len = e.z & 0xFF;
            if (len > 1) {
                if (afterWord) { if (o >= cap) { ok = false; break; } if (lane == 0) stg<u8>(dst + o, (u8)TX_SP); o++; }
                afterWord = true;
                delim = (int)i;
            } else {
                if (len == 0) { ok = false; break; }
                afterWord = false;
                delim = (int)i - 1;
            }
            if (o + len > room || o + len > cap) { ok = false; break; }
            if ((u32)lane < len) stg<u8>(dst + o + lane, (u8)(tx_text(src, e.y, (u32)lane) ^ (lane == 0 ? flip : 0u)));
            o += len;
        } else {
            if (!esc && c == TX_ESC1) {
                if (o >= cap) { ok = false; break; }
                const u32 x = rd(i++);
                if (lane == 0) stg<u8>(dst + o, (u8)x);
                o++;
            } else {
                if (crlf && c == TX_LF) {
                    if (o >= cap) { ok = false; break; }
                    if (lane == 0) stg<u8>(dst + o, (u8)TX_CR);
                    o++;
                    if (o >= room) { ok = false; break; }
                }
                if (o >= cap) { ok = false; break; }
                if (lane == 0) stg<u8>(dst + o, (u8)c);
                o++;
            }
            afterWord = false;
            delim = (int)i - 1;
        }
    }
    if (lane == 0) { st.ok[b] = (ok && i == end) ? 1 : 0; st.newLen[b] = o; }
}

// KNZ_TEXT_TABLES_MAX=bytes: what the scratch of the blocks that run at once may take (default 4 GiB). A larger batch runs in slices of as
// many blocks as fit, at least one.
size_t tx_budget()
{
    const char* e = getenv("KNZ_TEXT_TABLES_MAX");
    const long long v = e ? atoll(e) : 0;
    return v > 0 ? (size_t)v : ((size_t)4 << 30);
}

struct TxLayout { size_t stride, slotBytes, tblBytes, perBlock; u32 entCap; int per; };

// slotLog: the hash map's size; the size function takes the largest a stream of that block size can ask for
TxLayout tx_layout(int nBlocks, u32 maxLen, u32 slotLog)
{
    TxLayout l;
    l.stride = tx_stride_u32(maxLen);
    l.entCap = tx_ent_cap(maxLen);
    l.slotBytes = (size_t)4 << slotLog;
    l.tblBytes = l.slotBytes + (size_t)16 * l.entCap;
    l.perBlock = l.stride * 4 + l.tblBytes;
    const size_t fit = tx_budget() / l.perBlock;
    l.per = (int)(fit < 1 ? 1 : fit > (size_t)nBlocks ? (size_t)nBlocks : fit);
    return l;
}

u32 tx_max_slot_log(u32 blockSize) { return tx_log_slots(KNZ_E_TPAQX, blockSize); }

}  // namespace

size_t text_scratch_bytes(int nBlocks, u32 maxLen, u32 blockSize)
{
    if (nBlocks <= 0) return 0;
    const TxLayout l = tx_layout(nBlocks, maxLen, tx_max_slot_log(blockSize));
    return (size_t)l.per * l.perBlock + 256;
}

#define TX_LAUNCH(name, k, grid, threads, ...) do { KScope ks_(name); hipLaunchKernelGGL(k, grid, dim3(threads), 0, s, __VA_ARGS__); } while (0)

// The tables of a slice: the hash maps of its blocks side by side (one memset clears them), the entries behind them.
void launch_text_forward(hipStream_t s, const XfStage& st, void* scratch)
{
    if (st.nBlocks <= 0) return;
    // (the slice size comes from the largest map, as in text_scratch_bytes; the map itself has the size the stream's coder asks for)
    const TxLayout l = tx_layout(st.nBlocks, st.maxLen, tx_max_slot_log(st.blockSize));
    const size_t slotBytes = (size_t)4 << tx_log_slots(st.entropyType, st.blockSize);
    u32* ws = reinterpret_cast<u32*>(scratch);
    u8* slots = reinterpret_cast<u8*>(ws + (size_t)l.per * l.stride);
    u8* ents = slots + (size_t)l.per * l.slotBytes;
    for (int b0 = 0; b0 < st.nBlocks; b0 += l.per) {
        const int nb = st.nBlocks - b0 < l.per ? st.nBlocks - b0 : l.per;
        const dim3 grid(tx_chunks(st.maxLen), (unsigned)nb), one((unsigned)nb), few((unsigned)(nb + 63) / 64);
        // (the forward pass writes every entry before it reads it: only the maps are cleared)
        (void)hipMemsetAsync(slots, 0, (size_t)nb * slotBytes, s);
        TX_LAUNCH("k_tx_f_head", k_tx_f_head, one, TX_T, st, ws, l.stride, b0);
        TX_LAUNCH("k_tx_stats", k_tx_stats, grid, TX_T, st, ws, l.stride, b0);
        TX_LAUNCH("k_tx_verdict", k_tx_verdict, one, TX_T, st, ws, l.stride, b0);
        TX_LAUNCH("k_tx_words", k_tx_words, grid, TX_T, st, ws, l.stride, b0);
        TX_LAUNCH("k_tx_walk", k_tx_walk, one, 64, st, ws, l.stride, slots, ents, slotBytes, l.entCap, b0);
        TX_LAUNCH("k_tx_count", k_tx_emit<false>, grid, TX_T, st, ws, l.stride, b0);
        TX_LAUNCH("k_tx_oscan", k_tx_oscan, one, TX_T, st, ws, l.stride, b0);
        TX_LAUNCH("k_tx_emit", k_tx_emit<true>, grid, TX_T, st, ws, l.stride, b0);
        TX_LAUNCH("k_tx_f_final", k_tx_f_final, few, 64, st, ws, l.stride, b0, nb);
    }
}

void launch_text_inverse(hipStream_t s, const XfStage& st, void* scratch)
{
    if (st.nBlocks <= 0) return;
    const TxLayout l = tx_layout(st.nBlocks, st.maxLen, tx_max_slot_log(st.blockSize));
    const size_t slotBytes = (size_t)4 << tx_log_slots(st.entropyType, st.blockSize);
    u32* ws = reinterpret_cast<u32*>(scratch);
    u8* slots = reinterpret_cast<u8*>(ws + (size_t)l.per * l.stride);
    u8* ents = slots + (size_t)l.per * l.slotBytes;
    for (int b0 = 0; b0 < st.nBlocks; b0 += l.per) {
        const int nb = st.nBlocks - b0 < l.per ? st.nBlocks - b0 : l.per;
        // (the kernel zeroes the entries as its index takes them in)
        (void)hipMemsetAsync(slots, 0, (size_t)nb * slotBytes, s);
        TX_LAUNCH("k_tx_inverse", k_tx_inverse, dim3((unsigned)nb), 64, st, slots, ents, slotBytes, l.entCap, b0);
    }
}

}  // namespace knz
