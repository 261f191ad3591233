// CPU-only check of the TPAQ / TPAQX kernels' logic (kanzi-cpp_amd/csrc/tpaq.hip compiled as plain C++ against tools/hipemu). Test
// infrastructure only; tests/test_emu_tpaq.py compares the results with tests/tpaq_model.py.
//   usage: tpaq_emu <case file> <result file>
//   case file:   u32 nCases, then per case u32 mode (1 encode, 0 decode), u32 extra (1 = TPAQX), u32 rbsz (the stream's block size),
//                u32 count, u32 startBit, u32 inBits, u32 len, bytes
//                (encode: the block, count = copy threshold; decode: the stream, count = bytes to decode)
//   result file: per case u32 error (encode: blocks that were coded a second time), u32 bits (encode: bits written; decode: bits
//                used), u32 len, bytes
#include "hip/hip_runtime.h"
#include "../../kanzi-cpp_amd/csrc/cm.hip"
#include "../../kanzi-cpp_amd/csrc/tpaq.hip"

#include <stdio.h>
#include <vector>

namespace knz { thread_local ProfHook* g_prof = nullptr; }

using namespace knz;

static std::vector<u8> g_big;
static void* big_alloc(void*, size_t bytes)
{
    g_big.assign(bytes + 256, 0xEE);
    return reinterpret_cast<u8*>((reinterpret_cast<uintptr_t>(g_big.data()) + 255) & ~(uintptr_t)255);
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
        u32 h[7];
        if (fread(h, 4, 7, f) != 7) return 2;
        const u32 mode = h[0], extra = h[1], rbsz = h[2], count = h[3], startBit = h[4], inBits = h[5], len = h[6];
        std::vector<u8> data(len);
        if (len && fread(data.data(), 1, len, f) != len) return 2;
        u32 res[3] = { 0, 0, 0 };
        std::vector<u8> out;
        // the tables in an allocation of exactly their size (filled with a pattern: the launchers have to zero them)
        const u32 abszMax = mode == 1 ? len : count;
        const size_t tb = tpaq_table_bytes(rbsz, abszMax, (int)extra);
        if (tpaq_slice_blocks(tb, 1) != 1) return 2;
        u8* tables = static_cast<u8*>(aligned_alloc(256, tb));
        if (!tables) return 2;
        memset(tables, 0xA5, tb);
        if (mode == 1) {
            std::vector<u8> in(len + 32);
            u8* ip = reinterpret_cast<u8*>((reinterpret_cast<uintptr_t>(in.data()) + 15) & ~(uintptr_t)15);
            memcpy(ip, data.data(), len);
            const u8* ptr = ip;
            u32 blen = len, olen = len;
            BlockView view; view.ptr = &ptr; view.len = &blen;
            const int maxChunks = cm_max_chunks(len);
            std::vector<ChunkDesc> desc(maxChunks);
            const u64 stride = cm_stage_stride(len);
            u8* st = static_cast<u8*>(aligned_alloc(256, (size_t)stride));       // exactly the stride: AddressSanitizer's redzone sits right behind it
            if (!st) return 2;
            std::vector<u64> ctrl(cm_ctrl_bytes(1) / 8 + 1);
            launch_tpaq_encode(nullptr, (int)extra, view, &olen, count /* copy threshold */, 1, maxChunks, desc.data(), st, stride, ctrl.data(), tables, rbsz, abszMax);
            int again = 0;
            if (*reinterpret_cast<const u32*>(ctrl.data()) != 0)
                again = launch_tpaq_encode_again(nullptr, (int)extra, view, &olen, count, 1, maxChunks, desc.data(), st, stride, ctrl.data(), big_alloc, nullptr,
                                                 tables, rbsz, abszMax);
            if (again < 0) { fprintf(stderr, "launch_tpaq_encode_again: %d\n", again); return 1; }
            for (int ci = 0; ci < maxChunks; ci++) {
                const ChunkDesc& cd = desc[ci];
                for (u32 i = 0; i < cd.midLen; i++) out.push_back((u8)(cd.mid[i >> 2] >> (8 * (i & 3))));
                for (u32 k = 0; k < cd.nPieces; k++) {
                    const u8* p = cd.piecePtr[k];
                    const size_t nb = cd.pieceBits[k] / 8;
                    const bool inTmp = p >= st && p + nb <= st + stride, inBig = !g_big.empty() && p >= g_big.data() && p + nb <= g_big.data() + g_big.size();
                    if (!(p == ip && olen <= count) && !inTmp && !inBig) { fprintf(stderr, "piece of %zu bytes outside the staging\n", nb); return 1; }
                    out.insert(out.end(), p, p + nb);
                }
                for (u32 i = 0; i < cd.trailerLen; i++) out.push_back((u8)(cd.trailer[i >> 2] >> (8 * (i & 3))));
            }
            res[0] = (u32)again; res[1] = 8 * (u32)out.size(); res[2] = (u32)out.size();
            free(st);
        } else {
            const u64 nBytes = ((u64)inBits + 7) >> 3;
            std::vector<u32> words((nBytes + 3) / 4 + (nBytes == 0 ? 1 : 0));
            memcpy(words.data(), data.data(), (size_t)std::min<u64>(nBytes, len));
            BitSrc src; src.words = words.data(); src.nBytes = nBytes; src.nWords = nBytes >> 2; src.limitBits = inBits;
            DecBlock db; memset(&db, 0, sizeof(db));
            db.payloadBit = startBit; db.bits = inBits - startBit; db.entropyBit = startBit; db.preLen = count;
            std::vector<u8> exact(count);                                   // a destination of exactly `count` bytes
            u8* op = exact.data();
            u8* const* outPtr = &op;
            launch_tpaq_decode(nullptr, (int)extra, src, &db, 1, outPtr, tables, rbsz, abszMax);
            res[0] = (u32)db.error; res[1] = (u32)db.usedBits; res[2] = db.error ? 0 : db.preLen;
            out.assign(op, op + res[2]);
        }
        free(tables);
        fwrite(res, 4, 3, g);
        if (!out.empty()) fwrite(out.data(), 1, res[2], g);
    }
    fclose(f);
    fclose(g);
    printf("OK %u cases\n", nCases);
    return 0;
}
