// CPU-only check of the rANS order-1 encoder kernels and of the bit assembly in its 257-slots-per-chunk form (k_ans1_hist: the 256
// context histograms of a chunk; k_ans1_ctx: alphabet, normalised frequencies, header and encoding table of one context;
// k_ans1_encode: the chunk's four interleaved states; k_block_sum / k_block_scan / k_assemble): kanzi-cpp_amd/csrc/ans1.hip +
// bitasm.hip compiled as plain C++ against tools/hipemu, one block per call in the per-stage form (no framing), compared bit for
// bit with the oracle's ANS1 stream (ec_harness.hpp). Test infrastructure only.
//   usage: ans1_enc_emu <case file>    (binary: u32 nBlocks, then per block u32 len + bytes)
#define KNZ_EMU 1
#include "hip/hip_runtime.h"
#include "../../kanzi-cpp_amd/csrc/ans1.hip"
#include "../../kanzi-cpp_amd/csrc/bitasm.hip"
#include "ec_harness.hpp"

int main(int argc, char** argv)
{
    using namespace knz;
    std::vector<ChunkDesc> desc;
    std::vector<u8> hist, encTab, hdr, pay;
    return ec_encode_main(argc, argv, 8, [&](BlockView view, u32 n) {
        const int chunksPerBlock = n > ANS1_CHUNK ? (int)((n + ANS1_CHUNK - 1) / ANS1_CHUNK) : 1;
        const int maxChunks = chunksPerBlock * (int)ANS1_SLOTS;
        const size_t nCh = (size_t)chunksPerBlock;
        desc.assign((size_t)maxChunks, ChunkDesc());
        hist.assign(ans1_hist_bytes(nCh) + 64, 0);
        encTab.assign(ans1_enctab_bytes(nCh) + 64, 0);
        hdr.assign((size_t)HDR_BYTES * maxChunks + 256, 0);
        Ans1EncWs aw;
        aw.payStride = (2ull * (n < ANS1_CHUNK ? n : ANS1_CHUNK) + 511) & ~255ull;
        pay.assign((size_t)aw.payStride * nCh + 256, 0);
        aw.hist = reinterpret_cast<u32*>(hist.data()); aw.encTab = reinterpret_cast<uint2*>(encTab.data()); aw.hdr = hdr.data(); aw.pay = pay.data();
        launch_ans1_encode(nullptr, view, 1, chunksPerBlock, desc.data(), aw);
        return EcEncoded{ desc.data(), hdr.data(), maxChunks, ANS1_CHUNK, ANS1_SLOTS, HDR_BYTES };
    });
}
