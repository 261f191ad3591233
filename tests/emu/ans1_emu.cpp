// CPU-only check of the rANS order-1 decoder kernels (k_ans_scan<1>: per-block walk over the 256 context headers of every chunk;
// k_ans1_tables: slot tables per context; k_ans1_decode: the chunk's four interleaved states, the context = the previous byte of the
// same quarter):
// kanzi-cpp_amd/csrc/ans_dec.hip compiled as plain C++ against tools/hipemu, fed with the oracle's ANS1 streams, must
// reproduce the input and consume exactly the stream's bits (ec_harness.hpp). Test infrastructure only.
//   usage: ans1_emu <case file>    (binary: u32 nBlocks, then per block u32 len + bytes)
#define KNZ_EMU 1
#include "hip/hip_runtime.h"
#include "../../kanzi-cpp_amd/csrc/ans_dec.hip"
#include "ec_harness.hpp"

int main(int argc, char** argv)
{
    using namespace knz;
    return ec_decode_main(argc, argv, 8, [](BitSrc src, DecBlock* blocks, int nBlocks, u32 maxLen, u8* const* outPtr, int) {
        const int chunksPerBlock = (int)((maxLen + ANS1_CHUNK - 1) / ANS1_CHUNK);
        const size_t nCh = (size_t)nBlocks * chunksPerBlock;
        std::vector<u8> meta(ans1_meta_bytes(nCh) + 64);
        std::vector<u32> slotTab(ans1_slottab_bytes(nCh) / 4 + 16);
        Ans1DecWs ws;
        ws.meta = meta.data(); ws.slotTab = slotTab.data();
        launch_ans1_decode(nullptr, src, blocks, nBlocks, chunksPerBlock, ws, outPtr);
    });
}
