// kanzi_amd::compressMany / decompressMany against one CompressedOutputStream / CompressedInputStream per item: the same bytes, whether
// the device library behind them has the batch entry points or not. Prints "batched 0|1" (which path the pair took) and "OK <items>".
//   usage: streams_pair_test TRANSFORM ENTROPY BLOCKSIZE CHECKSUM
#include <cstdio>
#include <cstdlib>
#include <sstream>
#include <string>
#include <vector>

#include "kanzi_amd.hpp"

using namespace kanzi_amd;

int main(int argc, char** argv)
{
    if (argc < 5) return 2;
    const std::string transform = argv[1], entropy = argv[2];
    const int bs = atoi(argv[3]), checksum = atoi(argv[4]);
    // 40 buffers of 0 .. 3 blocks: words, runs and noise from a fixed generator
    std::vector<std::vector<byte>> bufs;
    uint32_t x = 12345;
    auto rnd = [&]() { x = x * 1664525u + 1013904223u; return x >> 8; };
    const char* words[] = { "stream ", "block ", "device ", "kanzi ", "batch ", "of ", "the ", "many ", "\n" };
    for (int i = 0; i < 40; i++) {
        const size_t n = i == 3 ? 0 : i == 7 ? size_t(2 * bs + 300) : i == 11 ? 15 : rnd() % size_t(bs + bs / 2);
        std::vector<byte> b;
        while (b.size() < n) {
            const uint32_t k = rnd() % 10;
            if (k < 6) for (const char* w = words[rnd() % 9]; *w; w++) b.push_back(byte(*w));
            else if (k < 8) b.insert(b.end(), 1 + rnd() % 40, byte(rnd() % 4));
            else for (int j = 0; j < 16; j++) b.push_back(byte(rnd()));
        }
        b.resize(n);
        bufs.push_back(b);
    }
    std::vector<ByteSpan> spans;
    for (auto& b : bufs) spans.push_back(ByteSpan{ b.data(), b.size() });
    std::vector<std::vector<byte>> streams, back;
    std::vector<int> errs;
    std::vector<std::string> msg;
    compressMany(spans, entropy, transform, bs, checksum, 1, streams, errs, &msg);
    int bad = 0;
    for (size_t i = 0; i < bufs.size(); i++) {
        if (errs[i]) { printf("FAIL item %zu: error %d (%s)\n", i, errs[i], msg[i].c_str()); bad++; continue; }
        std::ostringstream os(std::ios::binary);
        CompressedOutputStream cos(os, 1, entropy, transform, bs, checksum, uint64(bufs[i].size()), false);
        if (!bufs[i].empty()) cos.write(reinterpret_cast<const char*>(bufs[i].data()), std::streamsize(bufs[i].size()));
        cos.close();
        const std::string want = os.str();
        if (want.size() != streams[i].size() || !std::equal(want.begin(), want.end(), reinterpret_cast<const char*>(streams[i].data()))) {
            printf("FAIL item %zu (%zu bytes): %zu bytes, the stream class writes %zu\n", i, bufs[i].size(), streams[i].size(), want.size());
            bad++;
        }
    }
    // the way back, one stream damaged and one cut short: they alone fail
    std::vector<std::vector<byte>> in = streams;
    in[5][in[5].size() / 2 + 3] ^= 0x21;
    in[9].resize(in[9].size() - 3);
    spans.clear();
    for (auto& s : in) spans.push_back(ByteSpan{ s.data(), s.size() });
    decompressMany(spans, 1, back, errs, &msg);
    for (size_t i = 0; i < bufs.size(); i++) {
        const bool damaged = i == 5 || i == 9;
        if (damaged ? ((errs[i] == 0 && back[i] == bufs[i]) || msg[i].empty()) : (errs[i] != 0 || back[i] != bufs[i] || !msg[i].empty())) { printf("FAIL item %zu on the way back: error %d\n", i, errs[i]); bad++; }
    }
    printf("batched %d\n", deviceBatchesStreams() ? 1 : 0);
    printf(bad ? "FAILED %d\n" : "OK %zu\n", bad ? size_t(bad) : bufs.size());
    return bad ? 1 : 0;
}
