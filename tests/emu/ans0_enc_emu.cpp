// CPU-only check of the rANS order-0 encoder kernels and of the bit assembly (k_ans0_stats: alphabet, normalised frequencies and
// chunk header; k_ans0_encode: four interleaved states per chunk; k_block_sum / k_block_scan / k_assemble: the chunk pieces OR-ed
// into the block's bit stream): kanzi-cpp_amd/csrc/ans.hip + bitasm.hip compiled as plain C++ against tools/hipemu, one block per
// call in the per-stage form (no framing), compared bit for bit with the oracle's ANS0 stream (ec_harness.hpp). Test infrastructure only.
//   usage: ans0_enc_emu <case file>    (binary: u32 nBlocks, then per block u32 len + bytes)
#define KNZ_EMU 1
#include "hip/hip_runtime.h"
#include "../../kanzi-cpp_amd/csrc/ans.hip"
#include "../../kanzi-cpp_amd/csrc/bitasm.hip"
#include "ec_harness.hpp"

int main(int argc, char** argv)
{
    using namespace knz;
    std::vector<ChunkDesc> desc;
    std::vector<uint2> encTab;
    std::vector<u8> tmp;
    return ec_encode_main(argc, argv, 5, [&](BlockView view, u32 n) {
        const int maxChunks = (int)((n + ENT_CHUNK - 1) / ENT_CHUNK);
        desc.assign((size_t)maxChunks, ChunkDesc());
        encTab.assign(256 * (size_t)maxChunks, uint2());
        tmp.assign((size_t)TMP_STRIDE * maxChunks + 256, 0);
        launch_ans0_encode(nullptr, view, 1, maxChunks, desc.data(), encTab.data(), tmp.data());
        return EcEncoded{ desc.data(), tmp.data(), maxChunks, ENT_CHUNK, 1u, TMP_STRIDE };
    });
}
