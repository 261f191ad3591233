// Shared driver of the entropy-coder emulation tests (tests/emu/{ans0,ans1,huff}{,_enc}_emu.cpp), in the manner of xf_harness.hpp for
// the transforms. The including file includes its .hip file(s) first and keeps what is its own: an entropy id, its workspaces and one
// launch. Test infrastructure only.
//   decode side  ec_decode_main: reads the case file (u32 nBlocks, then per block u32 len + bytes), has the oracle encode every block,
//                packs the streams back to back at odd bit offsets, damages them when asked to (emu_corrupt), and hands BitSrc and
//                DecBlocks to the driver's launch. The kernels must reproduce the input and consume exactly the stream's bits; on damaged
//                input they only have to come back. A second argument is a bitstream version for the oracle and the launch.
//   encode side  ec_encode_main: per block the oracle's stream, the driver's launch (which says where its ChunkDescs and headers are),
//                then k_block_sum / k_block_scan / k_assemble in the per-stage form (no framing), compared bit for bit.
#include <stdio.h>
#include <stdlib.h>
#include <vector>
#include "emu_corrupt.hpp"

extern "C" int64_t knzo_entropy_encode(int etype, const uint8_t* in, uint32_t n, uint8_t* out, size_t cap);
extern "C" void knzo_set_bs_version(int v);

namespace knz { thread_local ProfHook* g_prof = nullptr; }

namespace knz {

// room for the oracle's stream of n bytes (order 1 writes 256 frequency tables per chunk: noise comes out longer than it went in)
inline size_t ec_stream_cap(u32 n) { return (size_t)2 * n + (1 << 18); }

// launch(src, blocks, nBlocks, maxLen, outPtr, bsVersion)
template <class Launch>
int ec_decode_main(int argc, char** argv, int etype, Launch&& launch)
{
    if (argc < 2) return 2;
    const int bsVersion = argc > 2 ? atoi(argv[2]) : 6;
    knzo_set_bs_version(bsVersion);
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    u32 nBlocks = 0;
    if (fread(&nBlocks, 4, 1, f) != 1) return 2;
    std::vector<std::vector<u8>> plain(nBlocks), out(nBlocks);
    std::vector<u8> stream;
    std::vector<DecBlock> blocks(nBlocks);
    u32 maxLen = 1;
    for (u32 b = 0; b < nBlocks; b++) {
        u32 n = 0;
        if (fread(&n, 4, 1, f) != 1) return 2;
        plain[b].resize(n);
        if (n && fread(plain[b].data(), 1, n, f) != n) return 2;
        std::vector<u8> enc(ec_stream_cap(n));
        const int64_t bits = knzo_entropy_encode(etype, plain[b].data(), n, enc.data(), enc.size());
        if (bits < 0) { printf("oracle refused block %u\n", b); return 2; }
        // blocks back to back at bit granularity, like in a stream: an odd bit offset for every second block
        const u64 at = (u64)stream.size() * 8 + ((b & 1) ? 3 : 0);
        stream.resize((size_t)((at + (u64)bits + 7) / 8) + 1, 0);
        for (int64_t i = 0; i < bits; i++) if ((enc[(size_t)(i >> 3)] >> (7 - (i & 7))) & 1) stream[(size_t)((at + (u64)i) >> 3)] |= (u8)(0x80 >> ((at + (u64)i) & 7));
        DecBlock& d = blocks[b];
        memset(&d, 0, sizeof(d));
        d.payloadBit = at; d.bits = (u64)bits; d.entropyBit = at; d.preLen = n;
        out[b].assign((size_t)n + 64, 0xEE);
        maxLen = std::max(maxLen, n);
    }
    fclose(f);
    emu_corrupt(stream.data(), stream.size(), 1);
    stream.resize((stream.size() + 64 + 3) & ~(size_t)3, 0);
    std::vector<u32> words(stream.size() / 4);
    memcpy(words.data(), stream.data(), stream.size());
    BitSrc src;
    src.words = words.data(); src.nWords = words.size(); src.nBytes = stream.size(); src.limitBits = (u64)stream.size() * 8;
    std::vector<u8*> outPtr(nBlocks);
    for (u32 b = 0; b < nBlocks; b++) outPtr[b] = out[b].data();
    launch(src, blocks.data(), (int)nBlocks, maxLen, outPtr.data(), bsVersion);
    int bad = 0;
    if (emu_corrupt_on()) { int errs = 0; for (u32 b = 0; b < nBlocks; b++) errs += blocks[b].error != 0; printf("damaged input: %d of %u blocks refused\n", errs, nBlocks); return 0; }
    for (u32 b = 0; b < nBlocks; b++) {
        const u32 n = (u32)plain[b].size();
        if (blocks[b].error || blocks[b].usedBits != blocks[b].bits || memcmp(out[b].data(), plain[b].data(), n) != 0) {
            u32 at = 0;
            while (at < n && out[b][at] == plain[b][at]) at++;
            printf("FAIL block %u (n=%u): error %d used %llu of %llu bits, first difference at %u\n", b, n, blocks[b].error,
                   (unsigned long long)blocks[b].usedBits, (unsigned long long)blocks[b].bits, at);
            bad++;
        }
    }
    printf(bad ? "FAILED %d blocks\n" : "OK %u blocks\n", bad ? bad : nBlocks, nBlocks);
    return bad ? 1 : 0;
}

// What an encoder launch leaves for the bit assembly: one ChunkDesc per slot, `slots` slots per chunk of `chunk` bytes, the headers
// `hdrStride` bytes apart from `hdr` on. The driver owns the memory until its next launch.
struct EcEncoded {
    ChunkDesc* desc;
    const u8* hdr;
    int maxChunks;       // slots of the block
    u32 chunk, slots, hdrStride;
};

// launch(view, n) -> EcEncoded, for one block of n bytes
template <class Launch>
int ec_encode_main(int argc, char** argv, int etype, Launch&& launch)
{
    if (argc < 2) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    u32 nBlocks = 0;
    if (fread(&nBlocks, 4, 1, f) != 1) return 2;
    int bad = 0;
    for (u32 b = 0; b < nBlocks; b++) {
        u32 n = 0;
        if (fread(&n, 4, 1, f) != 1) return 2;
        std::vector<u8> plain((size_t)n + 64, 0);
        if (n && fread(plain.data(), 1, n, f) != n) return 2;
        std::vector<u8> want(ec_stream_cap(n), 0);
        const int64_t wantBits = knzo_entropy_encode(etype, plain.data(), n, want.data(), want.size());
        if (wantBits < 0) { printf("oracle refused block %u\n", b); return 2; }
        std::vector<BlockInfo> info(1);
        const u8* ptr = plain.data();
        u32 len = n, origLen = n;
        u8 skip = 0;
        u64 total = 0;
        BlockView view; view.ptr = &ptr; view.len = &len;
        const EcEncoded e = launch(view, n);
        FrameParams fp; fp.framing = 0; fp.nTransforms = 1; fp.checksumBits = 0; fp.finish = 0; fp.prologueBits = 0;
        launch_block_sum(nullptr, e.desc, info.data(), &len, 1, e.maxChunks, e.chunk, e.slots);
        launch_block_scan(nullptr, info.data(), &len, &origLen, 1, fp, &total);
        std::vector<u32> out(((size_t)((total + 7) >> 3) + 8 + 3) / 4 + 16, 0);
        launch_assemble(nullptr, e.desc, info.data(), &len, &origLen, &skip, nullptr, e.hdr, 1, e.maxChunks, e.chunk, e.slots, e.hdrStride, fp, out.data());
        const u8* got = reinterpret_cast<const u8*>(out.data());
        const size_t bytes = (size_t)((wantBits + 7) >> 3);
        if ((int64_t)total != wantBits || memcmp(got, want.data(), bytes) != 0) {
            size_t at = 0;
            while (at < bytes && got[at] == want[at]) at++;
            printf("FAIL block %u (n=%u): %llu bits, oracle %lld, first different byte %zu\n", b, n, (unsigned long long)total, (long long)wantBits, at);
            bad++;
        }
    }
    fclose(f);
    printf(bad ? "FAILED %d blocks\n" : "OK %u blocks\n", bad ? bad : nBlocks, nBlocks);
    return bad ? 1 : 0;
}

}  // namespace knz
