// CPU-only check of the header helpers of kanzi-cpp_amd/csrc/ent_header.hpp on the fiber emulation of tools/hipemu: the alphabet
// writer against the reader through both fetchers (LDS window, peek_bits), the var-int reader in both forms, and HeaderWindow over a
// stream whose buffer ends with its last (partial) word, so that AddressSanitizer sees a read past it. This program only runs the
// helpers and prints what they gave; tests/test_emu_entropy_header.py builds it, writes the cases and judges the answers. Test
// infrastructure only.
//   usage: ent_header_emu <case file>
//   case file: u32 nCases, then per case u32 kind and
//     1 (alphabet)  u32 pos0, 32 mask bytes (bit s & 7 of byte s >> 3 = symbol s present)
//     2 (var-int)   u32 bit offset, u32 len, bytes
//     3 (window)    u32 len, bytes, u32 nOps, per op u32 what (0 read, 1 prefetch), u32 pos, u32 n, u32 need
//   output, one line per case:
//     A <bits> <header bytes, hex> then per fetcher: <asz> <first symbol> <next position> <present nibbles of lanes 0..63, hex> <ranks ...>
//     V then per form: <value> <bits taken> <err>
//     W per read op: <value>@<window origin>
#define KNZ_EMU 1
#include "hip/hip_runtime.h"
#include "../../kanzi-cpp_amd/csrc/ent_header.hpp"

#include <stdio.h>
#include <stdlib.h>
#include <vector>

namespace knz { thread_local ProfHook* g_prof = nullptr; }
using namespace knz;

struct AlphaOut {
    u32 bits;
    u32 asz[2], first[2], next[2];
    u32 present[2][64], rank[2][64];
};

__global__ void k_alphabet(const u8* mask, u32 pos0, u32* hdrMem, AlphaOut* out)
{
    __shared__ u32 hdrw[HDR_WORDS];
    const int lane = lane_id();
    for (int i = lane; i < (int)HDR_WORDS; i += 64) hdrw[i] = 0;
    __syncthreads();
    u32 f[4];
    for (int k = 0; k < 4; k++) f[k] = (mask[(4 * lane + k) >> 3] >> ((4 * lane + k) & 7)) & 1;
    const Alphabet al = alphabet_of(f);
    const u32 end = alphabet_put(lane, al.present, al.asz, hdrw, pos0);
    __syncthreads();
    header_flush(lane, hdrw, end, hdrMem);
    __syncthreads();
    BitSrc src;
    src.words = hdrMem; src.nWords = HDR_WORDS; src.nBytes = HDR_BYTES; src.limitBits = 8ull * HDR_BYTES;
    // the LDS bit buffer is a window already: words in stream order
    const AlphabetIn<u32> w = alphabet_get([&](u32 at, u32 nb) { return win_bits(hdrw, at, nb); }, lane, pos0);
    const AlphabetIn<u64> s = alphabet_get([&](u64 at, u32 nb) { return peek_bits(src, at, nb); }, lane, (u64)pos0);
    out->present[0][lane] = w.a.present; out->rank[0][lane] = w.a.rankBase;
    out->present[1][lane] = s.a.present; out->rank[1][lane] = s.a.rankBase;
    if (lane == 0) {
        out->bits = end - pos0;
        out->asz[0] = w.a.asz; out->first[0] = w.firstSym; out->next[0] = w.next;
        out->asz[1] = s.a.asz; out->first[1] = s.firstSym; out->next[1] = (u32)s.next;
    }
}

struct VarOut {
    u32 value[2], taken[2], err[2];
};

__global__ void k_varint(BitSrc src, u32 off, VarOut* out)
{
    __shared__ u32 win[64];
    const int lane = lane_id();
    win[lane] = ((u64)lane < src.nWords) ? bswap32(src.words[lane]) : 0u;
    __syncthreads();
    u32 q = off;
    int errW = 0;
    const u32 vw = win_varint(win, q, errW);
    u64 pos = off;
    int errS = 0;
    const u32 vs = take_varint(src, pos, errS);
    if (lane == 0) {
        out->value[0] = vw; out->taken[0] = q - off; out->err[0] = (u32)errW;
        out->value[1] = vs; out->taken[1] = (u32)(pos - off); out->err[1] = (u32)errS;
    }
}

struct WinOp {
    u32 what, pos, n, need;
};

__global__ void k_window(BitSrc src, const WinOp* ops, u32 nOps, u32* value, u64* origin)
{
    __shared__ u32 win[HDR_WIN_WORDS];
    const int lane = lane_id();
    HeaderWindow hw(win, src, lane);
    for (u32 i = 0; i < nOps; i++) {
        const WinOp op = ops[i];
        if (op.what == 1) { hw.prefetch(op.pos); continue; }
        hw.ensure(op.pos, op.need);
        const u32 v = hw.bits(op.pos, op.n);
        if (lane == 0) { value[i] = v; origin[i] = hw.bit0; }
    }
}

static bool rd(FILE* f, void* p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }

int main(int argc, char** argv)
{
    if (argc < 2) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    u32 nCases = 0;
    if (!rd(f, &nCases, 4)) return 2;
    for (u32 c = 0; c < nCases; c++) {
        u32 kind = 0;
        if (!rd(f, &kind, 4)) return 2;
        if (kind == 1) {
            u32 pos0 = 0;
            u8 mask[32];
            if (!rd(f, &pos0, 4) || !rd(f, mask, 32)) return 2;
            std::vector<u32> hdrMem(HDR_WORDS, 0);
            AlphaOut o;
            memset(&o, 0, sizeof(o));
            hipLaunchKernelGGL(k_alphabet, dim3(1), dim3(64), 0, nullptr, mask, pos0, hdrMem.data(), &o);
            printf("A %u ", o.bits);
            const u8* hb = reinterpret_cast<const u8*>(hdrMem.data());
            for (u32 i = 0; i < (pos0 + o.bits + 7) / 8; i++) printf("%02x", hb[i]);
            for (int k = 0; k < 2; k++) {
                printf(" %u %u %u ", o.asz[k], o.first[k], o.next[k]);
                for (int l = 0; l < 64; l++) printf("%x", o.present[k][l] & 0xF);
                for (int l = 0; l < 64; l++) printf("%c%u", l ? ',' : ' ', o.rank[k][l]);
            }
            printf("\n");
        } else if (kind == 2) {
            u32 off = 0, len = 0;
            if (!rd(f, &off, 4) || !rd(f, &len, 4)) return 2;
            std::vector<u32> words((len + 3) / 4 + 2, 0);
            if (!rd(f, words.data(), len)) return 2;
            BitSrc src;
            src.words = words.data(); src.nWords = words.size(); src.nBytes = 4 * words.size(); src.limitBits = 32ull * words.size();
            VarOut o;
            memset(&o, 0, sizeof(o));
            hipLaunchKernelGGL(k_varint, dim3(1), dim3(64), 0, nullptr, src, off, &o);
            printf("V %u %u %u %u %u %u\n", o.value[0], o.taken[0], o.err[0], o.value[1], o.taken[1], o.err[1]);
        } else if (kind == 3) {
            u32 len = 0, nOps = 0;
            if (!rd(f, &len, 4) || len == 0) return 2;
            // exactly the words the stream touches, the last one partial: a read past it is a heap overflow
            u32* words = static_cast<u32*>(malloc(((size_t)len + 3) / 4 * 4));
            if (!words) return 2;
            memset(words, 0, ((size_t)len + 3) / 4 * 4);
            if (!rd(f, words, len) || !rd(f, &nOps, 4)) return 2;
            std::vector<WinOp> ops(nOps);
            if (!rd(f, ops.data(), sizeof(WinOp) * nOps)) return 2;
            BitSrc src;
            src.words = words; src.nWords = len / 4; src.nBytes = len; src.limitBits = 8ull * len;
            std::vector<u32> value(nOps, 0);
            std::vector<u64> origin(nOps, 0);
            hipLaunchKernelGGL(k_window, dim3(1), dim3(64), 0, nullptr, src, ops.data(), nOps, value.data(), origin.data());
            printf("W");
            for (u32 i = 0; i < nOps; i++) if (ops[i].what == 0) printf(" %u@%llu", value[i], (unsigned long long)origin[i]);
            printf("\n");
            free(words);
        } else {
            return 2;
        }
    }
    fclose(f);
    return 0;
}
