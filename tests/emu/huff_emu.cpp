// CPU-only check of the Huffman decoder kernels' logic (k_huff_scan: per-block walk over the chunk headers with the table-driven
// parse of the Exp-Golomb code-length deltas; k_huff_decode: canonical tables and the four fragments of a chunk):
// kanzi-cpp_amd/csrc/huffman.hip compiled as plain C++ against tools/hipemu, fed with the oracle's Huffman streams, must
// reproduce the input and consume exactly the stream's bits (ec_harness.hpp). Test infrastructure only.
//   usage: huff_emu <case file> [bitstream version]   (binary: u32 nBlocks, then per block u32 len + bytes; a version below 6 makes the
//   oracle write, and the kernels read, the chunk layout of HuffmanDecoder.cpp:349-459)
#define KNZ_EMU 1
#include "hip/hip_runtime.h"
#include "../../kanzi-cpp_amd/csrc/huffman.hip"
#include "ec_harness.hpp"

int main(int argc, char** argv)
{
    using namespace knz;
    return ec_decode_main(argc, argv, 1, [](BitSrc src, DecBlock* blocks, int nBlocks, u32 maxLen, u8* const* outPtr, int bsVersion) {
        const int maxChunks = (int)((maxLen + ENT_CHUNK - 1) / ENT_CHUNK);
        std::vector<u8> meta(huffman_dec_chunk_bytes() * (size_t)nBlocks * maxChunks + 64);
        launch_huffman_decode(nullptr, src, blocks, nBlocks, maxChunks, meta.data(), outPtr, bsVersion);
    });
}
