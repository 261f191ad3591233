// CPU-only check of the rANS order-0 decoder kernels (k_ans_scan<0>: per-block walk over the chunk headers; k_ans0_decode: slot tables,
// four interleaved states per chunk sharing one byte pointer, payload ring in LDS):
// kanzi-cpp_amd/csrc/ans_dec.hip compiled as plain C++ against tools/hipemu, fed with the oracle's ANS0 streams, must
// reproduce the input and consume exactly the stream's bits (ec_harness.hpp). Test infrastructure only.
//   usage: ans0_emu <case file>    (binary: u32 nBlocks, then per block u32 len + bytes)
#define KNZ_EMU 1
#include "hip/hip_runtime.h"
#include "../../kanzi-cpp_amd/csrc/ans_dec.hip"
#include "ec_harness.hpp"

int main(int argc, char** argv)
{
    using namespace knz;
    return ec_decode_main(argc, argv, 5, [](BitSrc src, DecBlock* blocks, int nBlocks, u32 maxLen, u8* const* outPtr, int) {
        const int maxChunks = (int)((maxLen + ENT_CHUNK - 1) / ENT_CHUNK);
        std::vector<u8> meta(ans0_dec_chunk_bytes() * (size_t)nBlocks * maxChunks + 64);
        launch_ans0_decode(nullptr, src, blocks, nBlocks, maxChunks, meta.data(), outPtr);
    });
}
