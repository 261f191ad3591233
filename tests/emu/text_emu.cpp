// CPU-only check of the TEXT kernels' logic: kanzi-cpp_amd/csrc/text.hip compiled as plain C++ against the fiber emulation in
// tools/hipemu (no GPU involved; the product never runs this way). Built and run by tests/test_emu_text.py, which compares what it
// writes with tests/golden/text.json.
//   usage: text_emu <case file> <result file> <entropy id> <stream block size> [bitstream version]
// case file: u32 nBlocks, then per block u32 forward (1 / 0), u32 destination capacity, u32 data type, u32 len + bytes.
// result file, per block: u32 ok, u32 data type afterwards, u32 len + bytes. The forward blocks go through one batch, the inverse
// blocks through another; a write behind a block's capacity fails the run. KNZ_TEXT_TABLES_MAX makes the batches run in slices.
#include "hip/hip_runtime.h"
#include "../../kanzi-cpp_amd/csrc/text.hip"

#include <stdio.h>
#include <vector>

namespace knz { thread_local ProfHook* g_prof = nullptr; }

using namespace knz;

struct Case { u32 forward, cap, dtype; std::vector<u8> in, out; u32 ok = 0, newLen = 0, dtOut = 0; };

static int run(bool forward, std::vector<Case>& all, int entropy, u32 blockSize, int bsVersion)
{
    std::vector<Case*> cs;
    for (auto& c : all) if ((c.forward != 0) == forward) cs.push_back(&c);
    const int nBlocks = (int)cs.size();
    if (nBlocks == 0) return 0;
    u32 maxLen = 1;
    std::vector<const u8*> src(nBlocks); std::vector<u8*> dst(nBlocks);
    std::vector<u32> len(nBlocks), cap(nBlocks), newLen(nBlocks, 0);
    std::vector<u8> ok(nBlocks, 0), dt(nBlocks, 0);
    for (int b = 0; b < nBlocks; b++) {
        Case& c = *cs[b];
        c.out.assign((size_t)c.cap + 64, 0xEE);
        src[b] = c.in.data(); dst[b] = c.out.data(); len[b] = (u32)c.in.size(); cap[b] = c.cap; dt[b] = (u8)c.dtype;
        maxLen = std::max(maxLen, len[b]);
    }
    XfStage st;
    st.src = src.data(); st.dst = dst.data(); st.len = len.data(); st.cap = cap.data(); st.ok = ok.data(); st.newLen = newLen.data();
    st.nBlocks = nBlocks; st.maxLen = maxLen; st.scratchU32 = nullptr; st.entropyType = entropy; st.dtype = dt.data();
    st.blockSize = blockSize; st.bsVersion = bsVersion;
    std::vector<u8> scratch(text_scratch_bytes(nBlocks, maxLen, blockSize) + 256, 0xCD);
    u8* sc = reinterpret_cast<u8*>((reinterpret_cast<uintptr_t>(scratch.data()) + 255) & ~(uintptr_t)255);
    if (forward) launch_text_forward(nullptr, st, sc); else launch_text_inverse(nullptr, st, sc);
    int bad = 0;
    for (int b = 0; b < nBlocks; b++) {
        Case& c = *cs[b];
        c.ok = ok[b]; c.newLen = ok[b] ? newLen[b] : 0; c.dtOut = dt[b];
        if (c.newLen > c.cap) { printf("FAIL block %d: length %u beyond the capacity %u\n", b, c.newLen, c.cap); bad++; c.newLen = 0; }
        for (size_t k = c.cap; k < c.out.size(); k++)
            if (c.out[k] != 0xEE) { printf("FAIL %s block %d: write behind the capacity at %zu\n", forward ? "forward" : "inverse", b, k); bad++; break; }
        c.out.resize(c.newLen);
    }
    return bad;
}

int main(int argc, char** argv)
{
    if (argc < 5) return 2;
    const int entropy = atoi(argv[3]);
    const u32 blockSize = (u32)strtoul(argv[4], nullptr, 10);
    const int bsVersion = argc > 5 ? atoi(argv[5]) : 6;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    u32 nBlocks = 0;
    if (fread(&nBlocks, 4, 1, f) != 1) return 2;
    std::vector<Case> cs(nBlocks);
    for (auto& c : cs) {
        u32 h[4];
        if (fread(h, 4, 4, f) != 4) return 2;
        c.forward = h[0]; c.cap = h[1]; c.dtype = h[2];
        c.in.resize(h[3]);                                  // (no slack: the kernels read nothing behind a block)
        if (h[3] && fread(c.in.data(), 1, h[3], f) != h[3]) return 2;
    }
    fclose(f);
    const int bad = run(true, cs, entropy, blockSize, bsVersion) + run(false, cs, entropy, blockSize, bsVersion);
    FILE* o = fopen(argv[2], "wb");
    if (!o) return 2;
    for (auto& c : cs) {
        const u32 h[3] = { c.ok, c.dtOut, (u32)c.out.size() };
        fwrite(h, 4, 3, o);
        if (!c.out.empty()) fwrite(c.out.data(), 1, c.out.size(), o);
    }
    fclose(o);
    printf(bad ? "FAILED %d\n" : "OK %u blocks\n", bad ? bad : (int)nBlocks);
    return bad ? 1 : 0;
}
