// CPU-only check of the RANGE kernels' logic (kanzi-cpp_amd/csrc/range.hip compiled as plain C++ against tools/hipemu). Test
// infrastructure only; tests/test_emu_range.py compares the results with tests/range_model.py.
//   usage: range_emu <case file> <result file>
//   case file:   u32 nCases, then per case u32 mode (1 encode, 0 decode), u32 count, u32 startBit, u32 inBits, u32 len, bytes
//                (encode: the block; decode: the stream, count = bytes to decode)
//   result file: per case u32 error, u32 bits (encode: bits written; decode: bits used), u32 len, bytes
#include "hip/hip_runtime.h"
#include "../../kanzi-cpp_amd/csrc/range.hip"

#include <stdio.h>
#include <vector>

namespace knz { thread_local ProfHook* g_prof = nullptr; }

using namespace knz;

static void put_bits(std::vector<u8>& out, u64& nbits, const u8* src, u64 n)
{
    for (u64 i = 0; i < n; i++) {
        const u32 bit = (src[i >> 3] >> (7 - (i & 7))) & 1;
        if ((nbits & 7) == 0) out.push_back(0);
        out[nbits >> 3] |= (u8)(bit << (7 - (nbits & 7)));
        nbits++;
    }
}

int main(int argc, char** argv)
{
    if (argc < 3) return 2;
    FILE* f = fopen(argv[1], "rb");
    FILE* g = fopen(argv[2], "wb");
    if (!f || !g) return 2;
    u32 nCases = 0;
    if (fread(&nCases, 4, 1, f) != 1) return 2;
    for (u32 c = 0; c < nCases; c++) {
        u32 h[5];
        if (fread(h, 4, 5, f) != 5) return 2;
        const u32 mode = h[0], count = h[1], startBit = h[2], inBits = h[3], len = h[4];
        std::vector<u8> data(len);
        if (len && fread(data.data(), 1, len, f) != len) return 2;
        u32 res[3] = { 0, 0, 0 };
        std::vector<u8> out;
        if (mode == 1) {
            // 16-byte aligned copy of the block, as the library's buffers are
            std::vector<u8> in(len + 32);
            u8* ip = reinterpret_cast<u8*>((reinterpret_cast<uintptr_t>(in.data()) + 15) & ~(uintptr_t)15);
            memcpy(ip, data.data(), len);
            const u8* ptr = ip;
            u32 blen = len, olen = len;
            BlockView view; view.ptr = &ptr; view.len = &blen;
            const int maxChunks = (int)((len + RANGE_CHUNK - 1) / RANGE_CHUNK);
            std::vector<ChunkDesc> desc(maxChunks);
            std::vector<u32> cumFreq((size_t)maxChunks * 256);
            std::vector<u8> tmp((size_t)maxChunks * RANGE_STRIDE + 256);
            u8* tb = reinterpret_cast<u8*>((reinterpret_cast<uintptr_t>(tmp.data()) + 255) & ~(uintptr_t)255);
            launch_range_encode(nullptr, view, &olen, count /* copy threshold */, 1, maxChunks, desc.data(), cumFreq.data(), tb);
            u64 nbits = 0;
            std::vector<u64> chunkBit(maxChunks);
            for (int ci = 0; ci < maxChunks; ci++) {
                const ChunkDesc& cd = desc[ci];
                chunkBit[ci] = nbits;
                put_bits(out, nbits, tb + (size_t)ci * RANGE_STRIDE, cd.hdrBits);
                for (u32 k = 0; k < cd.nPieces; k++) {
                    if (cd.pieceBits[k] > 8u * RANGE_PAY_BYTES) { fprintf(stderr, "piece of %u bits exceeds the staging region\n", cd.pieceBits[k]); return 1; }
                    put_bits(out, nbits, cd.piecePtr[k], cd.pieceBits[k]);
                }
            }
            // chunks with a wide frequency: the reference's unmasked writes, as k_assemble adds them (the stream starts at bit 0 here)
            std::vector<u32> words((out.size() + 3) / 4 + 1, 0);
            memcpy(words.data(), out.data(), out.size());
            for (int ci = 0; ci < maxChunks; ci++)
                if (desc[ci].aux >> 31) range_wide_spill(words.data(), chunkBit[ci], chunkBit[ci], desc[ci]);
            memcpy(out.data(), words.data(), out.size());
            res[1] = (u32)nbits; res[2] = (u32)out.size();
        } else {
            // the stream in a buffer of exactly the words the kernel may touch (the last, partial word included), so that AddressSanitizer sees a read past it
            const u64 nBytes = ((u64)inBits + 7) >> 3;
            std::vector<u32> words((nBytes + 3) / 4 + (nBytes == 0 ? 1 : 0));
            memcpy(words.data(), data.data(), (size_t)std::min<u64>(nBytes, len));
            BitSrc src; src.words = words.data(); src.nBytes = nBytes; src.nWords = nBytes >> 2; src.limitBits = inBits;
            DecBlock db; memset(&db, 0, sizeof(db));
            db.payloadBit = startBit; db.bits = inBits - startBit; db.entropyBit = startBit; db.preLen = count;
            out.assign(count, 0xEE);
            std::vector<u32> guard(count / 4 + 2);                          // 4-byte aligned destination of exactly `count` bytes
            u8* op = reinterpret_cast<u8*>(guard.data());
            u8* const* outPtr = &op;
            launch_range_decode(nullptr, src, &db, 1, outPtr, 0);
            res[0] = (u32)db.error; res[1] = (u32)db.usedBits; res[2] = db.error ? 0 : db.preLen;
            out.assign(op, op + res[2]);
        }
        fwrite(res, 4, 3, g);
        if (!out.empty()) fwrite(out.data(), 1, res[2], g);
    }
    fclose(f);
    fclose(g);
    printf("OK %u cases\n", nCases);
    return 0;
}
