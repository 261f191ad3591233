// CPU-only run of the LZ / LZX decoders of kanzi-cpp_amd/csrc/lz.hip on blocks taken as they are: encoded blocks with damage in them
// (tests/first_gen_damage.py). Every block goes through the data-parallel decoder (k_lz_i_pparse, k_lz_i_parse for what it hands on,
// expand, pointer jumping, emit) and through the one-wave-per-block decoder (k_lz_inverse), and both have to agree with the oracle's
// inverse on accept / refuse, on the length and on every byte of what is accepted. Test infrastructure only.
//   usage: lz_raw_emu <case file> <transform id: 3 LZ, 16 LZX>   (binary: u32 nBlocks, then per block u32 len, u32 destination capacity, bytes)
//   prints "block <i> ok <0|1> len <n>" per block (the oracle's answer) and "OK <n> blocks" or "FAILED ..."
#define KNZ_EMU 1
#include "hip/hip_runtime.h"
#include "../../kanzi-cpp_amd/csrc/lz.hip"

#include <stdio.h>
#include <vector>

extern "C" int knzo_transform_inverse(int ttype, const uint8_t* src, int n, uint8_t* dst, int dstCap, int* outLen);

namespace knz { thread_local ProfHook* g_prof = nullptr; }

int main(int argc, char** argv)
{
    using namespace knz;
    if (argc < 3) return 2;
    const int ttype = atoi(argv[2]);
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    u32 nBlocks = 0;
    if (fread(&nBlocks, 4, 1, f) != 1) return 2;
    std::vector<std::vector<u8>> enc(nBlocks), want(nBlocks), got(nBlocks);
    std::vector<u32> len(nBlocks), cap(nBlocks), newLen(nBlocks, 0);
    std::vector<int> wantOk(nBlocks), wantLen(nBlocks);
    u32 maxLen = 1, maxCap = 1;
    for (u32 b = 0; b < nBlocks; b++) {
        if (fread(&len[b], 4, 1, f) != 1 || fread(&cap[b], 4, 1, f) != 1) return 2;
        enc[b].assign((size_t)len[b] + 64, 0);                   // (as the other drivers: the kernels may read a few bytes past the end)
        if (len[b] && fread(enc[b].data(), 1, len[b], f) != len[b]) return 2;
        want[b].assign((size_t)cap[b] + 64, 0xEE);
        int ol = 0;
        wantOk[b] = knzo_transform_inverse(ttype, enc[b].data(), (int)len[b], want[b].data(), (int)cap[b], &ol) ? 1 : 0;
        wantLen[b] = ol;
        printf("block %u ok %d len %d\n", b, wantOk[b], wantLen[b]);
        maxLen = std::max(maxLen, len[b]); maxCap = std::max(maxCap, cap[b]);
    }
    fclose(f);
    std::vector<const u8*> src(nBlocks); std::vector<u8*> dst(nBlocks);
    std::vector<u8> ok(nBlocks, 0);
    XfStage st;
    st.src = src.data(); st.dst = dst.data(); st.len = len.data(); st.cap = cap.data(); st.ok = ok.data(); st.newLen = newLen.data();
    st.nBlocks = (int)nBlocks; st.maxLen = maxLen; st.scratchU32 = nullptr; st.entropyType = -1; st.bsVersion = 6;
    int bad = 0;
    for (int serial = 0; serial < 2; serial++) {
        for (u32 b = 0; b < nBlocks; b++) { got[b].assign((size_t)cap[b] + 64, 0xEE); src[b] = enc[b].data(); dst[b] = got[b].data(); ok[b] = 0; newLen[b] = 0; }
        std::vector<u8> scratch;
        if (serial) launch_lz_inverse(nullptr, st, nullptr, 0, 0);
        else {
            const size_t bytes = lz_inverse_scratch_bytes(st.nBlocks, maxCap);
            scratch.assign(bytes + 512, 0x7F);                   // (stale entries must not look like finished ones)
            void* sc = reinterpret_cast<void*>((reinterpret_cast<uintptr_t>(scratch.data()) + 255) & ~(uintptr_t)255);
            launch_lz_inverse(nullptr, st, sc, bytes, maxCap);
        }
        for (u32 b = 0; b < nBlocks; b++) {
            const bool same = (ok[b] != 0) == (wantOk[b] != 0) && (!wantOk[b] || ((int)newLen[b] == wantLen[b] && memcmp(got[b].data(), want[b].data(), (size_t)wantLen[b]) == 0));
            if (!same) { printf("FAIL %s block %u: ok %d/%d len %u/%d\n", serial ? "one wave per block" : "data parallel", b, ok[b], wantOk[b], newLen[b], wantLen[b]); bad++; }
        }
    }
    printf(bad ? "FAILED %d blocks\n" : "OK %u blocks\n", bad ? bad : nBlocks, nBlocks);
    return bad ? 1 : 0;
}
