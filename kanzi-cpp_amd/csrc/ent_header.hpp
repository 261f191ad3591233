// The chunk-header language of the first-generation entropy coders (HUFFMAN, ANS0, ANS1, RANGE), from the reference's EntropyUtils: a
// presence-mask alphabet, frequencies in groups of 6 or 8 behind a width field, var-ints -- written and read by one wave whose lane owns
// symbols 4*lane .. 4*lane+3. Nothing here is rANS- or Huffman-specific (normalisation, the frequency-group writer and the rANS encoder
// table: ans_common.hpp). Everything is forced inline and compiles as plain C++ for the CPU emulation of tests/emu, which tests these
// helpers directly (tests/emu/ent_header_emu.cpp).
#pragma once
#include "common.hpp"

namespace knz {

// ================================================================================================
// write side
// ================================================================================================
// Byte counts of one chunk by one wave (Global.cpp:170-221): 16 bytes per lane per iteration into 8 private histograms chosen by lane
// -- one ds_add instruction never sends more than 8 lanes to the same copy, which is what bounds the same-address serialisation on
// skewed data (text: 15 % spaces). Row stride 264: copy c of a symbol sits 8c banks away, not in the same bank. `hist` must be zero;
// f[k] = count of symbol 4 * lane + k.
__device__ __forceinline__ void chunk_counts(int lane, const u8* blk, u32 n, u32 (*hist)[264], u32 f[4])
{
    u32* myHist = hist[lane & 7];
    const u32 n16 = n & ~15u;
    const bool aligned = ((reinterpret_cast<uintptr_t>(blk) & 15) == 0);
    if (aligned) {
        const uint4* p4 = reinterpret_cast<const uint4*>(blk);
        for (u32 i = lane; i < (n16 >> 4); i += 64) {
            const uint4 v = p4[i];
            const u32 w[4] = { v.x, v.y, v.z, v.w };
#pragma unroll
            for (int k = 0; k < 4; k++) {
                atomicAdd(&myHist[w[k] & 0xFF], 1u);
                atomicAdd(&myHist[(w[k] >> 8) & 0xFF], 1u);
                atomicAdd(&myHist[(w[k] >> 16) & 0xFF], 1u);
                atomicAdd(&myHist[w[k] >> 24], 1u);
            }
        }
    } else {
        for (u32 i = lane; i < n16; i += 64) atomicAdd(&myHist[blk[i]], 1u);
    }
    for (u32 i = n16 + lane; i < n; i += 64) atomicAdd(&myHist[blk[i]], 1u);
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int s = 4 * lane + k;
        u32 acc = 0;
#pragma unroll
        for (int c = 0; c < 8; c++) acc += hist[c][s];
        f[k] = acc;
    }
}

// The alphabet as the wave holds it: bit k of `present` = symbol 4*lane + k occurs, `asz` = how many symbols do (uniform), `rankBase`
// = the alphabet index of this lane's first present symbol.
struct Alphabet {
    u32 present, asz, rankBase;
};

__device__ __forceinline__ Alphabet alphabet_of_present(u32 present)
{
    const u32 myCount = __popc(present);
    const u32 inclCount = wave_incl_scan(myCount);
    Alphabet a;
    a.present = present;
    a.asz = (u32)__shfl((int)inclCount, 63, 64);
    a.rankBase = inclCount - myCount;
    return a;
}

__device__ __forceinline__ Alphabet alphabet_of(const u32 f[4])
{
    u32 present = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) present |= (f[k] != 0 ? 1u : 0u) << k;
    return alphabet_of_present(present);
}

// encodeAlphabet (EntropyUtils.cpp:57-89) into the LDS bit buffer `hdrw` (zeroed) at bit `pos`; returns the new position.
__device__ __forceinline__ u32 alphabet_put(int lane, u32 present, u32 asz, u32* hdrw, u32 pos)
{
    if (asz == 0) {
        if (lane == 0) or_bits_words(hdrw, pos, 1, 2);   // FULL_ALPHABET(0), ALPHABET_0(1)
        return pos + 2;
    }
    if (asz == 256) return pos + 2;                 // FULL_ALPHABET(0), ALPHABET_256(0)
    // PARTIAL_ALPHABET(1), 5 bits lastMask, masks
    const u64 anyMask = __ballot(present != 0);
    const int lastLane = 63 - __clzll((long long)anyMask);
    const u32 lastMask = (u32)lastLane >> 1;        // symbol >> 3 == lane >> 1
    if (lane == 0) {
        or_bits_words(hdrw, pos, 1, 1);
        or_bits_words(hdrw, pos + 1, lastMask, 5);
    }
    pos += 6;
    // mask byte m: low nibble from lane 2m, high nibble from lane 2m+1 ; bit (s&7) = symbol present
    const u32 other = (u32)__shfl_xor((int)present, 1, 64);
    if ((lane & 1) == 0 && ((u32)lane >> 1) <= lastMask) {
        const u32 byte = present | (other << 4);
        or_bits_words(hdrw, pos + 8 * ((u32)lane >> 1), byte, 8);
    }
    return pos + 8 * (lastMask + 1);
}

// the first `bits` bits of the LDS bit buffer to the chunk's header area (memory order = stream order)
__device__ __forceinline__ void header_flush(int lane, const u32* hdrw, u32 bits, void* dst)
{
    u32* hdrOut = reinterpret_cast<u32*>(dst);
    for (u32 i = lane; i < ((bits + 31) >> 5); i += 64) hdrOut[i] = bswap32(hdrw[i]);
}

// a chunk that is nothing but `bits` bits of its own text: tiny blocks and chunks, copy blocks, the NONE codec
__device__ __forceinline__ void desc_raw(ChunkDesc* cd, const u8* ptr, u32 bits)
{
    cd->hdrBits = 0; cd->midLen = 0; cd->trailerLen = 0; cd->aux = 0;
    cd->nPieces = 1; cd->pieceBits[0] = bits; cd->piecePtr[0] = ptr;
}

// ================================================================================================
// read side
// ================================================================================================
// Stream words by index, clamped to the last (possibly partial) word of the buffer: loads stay branch-free and never leave it. Bytes
// past the stream's end are never trusted -- positions past the block's limit are rejected before anything read there is used -- and
// an aligned dword never straddles a page. `raw` is the word as it lies in memory (bswap32 gives stream order).
struct ClampedWords {
    const u32* words;
    u64 last;
    __device__ __forceinline__ u32 raw(u64 w) const { return words[w < last ? w : last]; }
};

__device__ __forceinline__ ClampedWords clamped_words(const BitSrc& s)
{
    ClampedWords c;
    c.words = s.words;
    c.last = ((s.nBytes + 3) >> 2) - 1;
    return c;
}

// n in [1, 32]; rel = bit offset from the start of an LDS window whose words are in stream (bit) order
__device__ __forceinline__ u32 win_bits(const u32* win, u32 rel, u32 n)
{
    const u32 i = rel >> 5;
    const u64 v = ((u64)win[i] << 32) | (u64)win[i + 1];
    return (u32)((v << (rel & 31)) >> (64 - n));
}

// The header scans (k_ans_scan, k_huff_scan) stage a 1 KiB window of the stream in LDS (`win`, HDR_WIN_WORDS words declared by the
// kernel: 4 words per lane, byte-swapped to bit order, and 8 words a read past the last bit may touch). Everything a header walk reads
// there is wave-uniform: all lanes run the same short dependent chain, with no cross-lane traffic. A second window, loaded at a guessed
// position while a chunk is parsed, waits in registers for the next chunk.
constexpr u32 HDR_WIN_BITS = 8192;
constexpr u32 HDR_WIN_WORDS = HDR_WIN_BITS / 32 + 8;

struct HeaderWindow {
    u32* win;
    ClampedWords cw;
    int lane;
    u32x4 wr, guess;
    u64 bit0, guessBit0;             // stream bit of the window's first bit (a multiple of 32)
    bool valid, guessValid;

    __device__ __forceinline__ HeaderWindow(u32* w, const BitSrc& src, int l)
        : win(w), cw(clamped_words(src)), lane(l), wr{ 0, 0, 0, 0 }, guess{ 0, 0, 0, 0 }, bit0(0), guessBit0(0), valid(false), guessValid(false) {}

    __device__ __forceinline__ void issue(u64 at, u32x4& dstv) const
    {
        const u64 w = (at >> 5) + 4ull * (u32)lane;
        dstv.x = cw.raw(w);
        dstv.y = cw.raw(w + 1);
        dstv.z = cw.raw(w + 2);
        dstv.w = cw.raw(w + 3);
    }
    // make stream bits [pos, pos + need) readable through `win`: keep the current window if it still covers them, else take the
    // prefetched guess if it does, else load exactly (blocking)
    __device__ __forceinline__ void ensure(u64 pos, u32 need)
    {
        if (valid && bit0 <= pos && pos + need <= bit0 + HDR_WIN_BITS) return;
        if (guessValid && guessBit0 <= pos && pos + need <= guessBit0 + HDR_WIN_BITS) {
            wr = guess; bit0 = guessBit0;
        } else {
            bit0 = pos & ~31ull;
            issue(bit0, wr);
        }
        guessValid = false;
        __syncthreads();
        {
            u32x4 sw = { bswap32(wr.x), bswap32(wr.y), bswap32(wr.z), bswap32(wr.w) };
            *reinterpret_cast<u32x4*>(&win[4 * lane]) = sw;
        }
        __syncthreads();
        valid = true;
    }
    // start loading the window that begins at stream bit `at` (a multiple of 32); a later ensure() takes it if it fits
    __device__ __forceinline__ void prefetch(u64 at)
    {
        guessBit0 = at;
        issue(at, guess);
        guessValid = true;
    }
    __device__ __forceinline__ void forget() { guessValid = false; }
    // where to prefetch for the chunk after the one at `pos`, when the one before began at `prevPos`: the same compressed size again,
    // the window centred on the estimate
    static __device__ __forceinline__ u64 guess_at(u64 pos, u64 prevPos)
    {
        const u64 est = pos + (pos - prevPos);
        return (est > 2304 ? est - 2304 : 0) & ~31ull;
    }
    // n in [1, 32] bits at stream bit `pos`, which an ensure() has covered
    __device__ __forceinline__ u32 bits(u64 pos, u32 n) const { return win_bits(win, (u32)(pos - bit0), n); }
};

// EntropyUtils::readVarInt (entropy/EntropyUtils.cpp:261-285). fetch8() gives the next 8 bits and may set `err` itself (a read past
// the limit); a fifth byte with its continuation bit or one of bits 4-6 set is an error. The value is meaningless when err is set.
template <class Fetch8>
__device__ __forceinline__ u32 varint_get(Fetch8&& fetch8, int& err)
{
    u32 value = fetch8();
    u32 res = value & 0x7F;
    for (int shift = 7; value >= 128 && !err; shift += 7) {
        value = fetch8();
        if (shift == 28) {
            if (value >= 128 || (value & 0x70) != 0) err = 1;
            res |= (value & 0x0F) << shift;
            break;
        }
        res |= (value & 0x7F) << shift;
    }
    return res;
}

__device__ __forceinline__ u32 take_varint(const BitSrc& s, u64& pos, int& err)
{
    return varint_get([&]() { return take_bits(s, pos, 8, err); }, err);
}

// var-int at window-relative bit q of an LDS window; q moves behind it
__device__ __forceinline__ u32 win_varint(const u32* win, u32& q, int& err)
{
    return varint_get([&]() { const u32 v = win_bits(win, q, 8); q += 8; return v; }, err);
}

// this lane's four symbols in a presence-mask byte that covers symbols 8 * (lane >> 1) .. + 7
// (a bit-field extract at an offset that depends on the lane alone: inside a scan's chunk loop it is one instruction)
__device__ __forceinline__ u32 mask_nibble(u32 byte, int lane) { return (byte >> (4 * ((u32)lane & 1))) & 0xFu; }

// decodeAlphabet (EntropyUtils.cpp:91-123) at position p; fetch(pos, n) gives n <= 8 bits at a position of p's type (the LDS window or
// peek_bits). Returns the alphabet, its first symbol, and the position behind it; a partial alphabet's mask bytes start at p + 6.
template <class P>
struct AlphabetIn {
    Alphabet a;
    u32 firstSym;
    P next;
};

template <class P, class Fetch>
__device__ __forceinline__ AlphabetIn<P> alphabet_get(Fetch&& fetch, int lane, P p)
{
    AlphabetIn<P> r;
    r.firstSym = 0;
    const u32 hb = fetch(p, 7);                    // flag bits and (partial alphabets) the mask count
    if ((hb >> 6) == 0) {
        const bool none = (hb >> 5) & 1;
        r.a.present = none ? 0u : 0xFu;
        r.a.asz = none ? 0u : 256u;
        r.a.rankBase = none ? 0u : 4u * (u32)lane;
        r.next = p + 2;
        return r;
    }
    const u32 lastMask = (hb >> 1) & 31;
    p += 6;
    const u32 m = (u32)lane >> 1;
    const u32 byte = (m <= lastMask) ? fetch(p + 8u * m, 8) : 0u;
    const u32 present = mask_nibble(byte, lane);
    const u32 myCount = __popc(present);
    const u32 inclCount = wave_incl_scan(myCount);
    r.a.present = present;
    r.a.asz = rl(inclCount, 63);
    r.a.rankBase = inclCount - myCount;
    const u64 nz = __ballot(present != 0);
    if (nz) {
        const int fl = __ffsll((long long)nz) - 1;
        r.firstSym = 4u * (u32)fl + (u32)(__ffs((int)rl(present, (u32)fl)) - 1);
    }
    r.next = p + 8u * (lastMask + 1);
    return r;
}

// The frequencies of this lane's symbols from the groups of 6 or 8 (ANSRangeDecoder.cpp:113-171, RangeDecoder.cpp:87-124): the symbol
// of alphabet index r >= 1 is value (r - 1) % chk of group (r - 1) / chk; group(g, w) gives the position of that group's first value
// and sets its width w; fetch(pos, n) reads. The first symbol of the alphabet takes what the others leave of `scale`. Returns true
// (for the whole wave) when a frequency or their sum does not fit below scale; f[] is not complete then.
template <class Group, class Fetch>
__device__ __forceinline__ bool freqs_get(const Alphabet& a, u32 scale, Group&& group, Fetch&& fetch, u32 f[4])
{
    const u32 chk = (a.asz >= 64) ? 8u : 6u;
    u32 r = a.rankBase;
    u32 sum = 0;
    bool bad = false;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        f[k] = 0;
        if ((a.present >> k) & 1) {
            if (r >= 1) {
                const u32 g = (r - 1) / chk;
                u32 w;
                const u64 at = group(g, w);
                const u32 fv = w ? fetch(at + (u64)((r - 1) - g * chk) * w, w) + 1u : 1u;
                bad |= fv >= scale;
                f[k] = fv;
                sum += fv;
            }
            r++;
        }
    }
    const u32 total = wave_sum(sum);
    if (__ballot(bad) != 0 || scale <= total) return true;
    if (a.rankBase == 0 && a.present) {
        const int k0 = __ffs((int)a.present) - 1;
#pragma unroll
        for (int k = 0; k < 4; k++) if (k == k0) f[k] = scale - total;
    }
    return false;
}

}  // namespace knz
