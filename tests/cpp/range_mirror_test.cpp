// RangeEncoder / RangeDecoder of the C++ host mirror (include/kanzi_amd.hpp) the way src/test/TestEntropyCodec.cpp exercises the
// reference's: round trips from a bit offset, directly and through the factories and the stream classes, and the constructor checks.
// Runs on the GPU box (tests/test_gpu_range.py drives it); returns 0 / non-zero.
#include <cstdio>
#include <cstring>
#include <sstream>
#include <stdexcept>
#include <string>
#include <vector>

#include "kanzi_amd.hpp"

using namespace kanzi_amd;

static int fails = 0;
#define CHECK(c) do { if (!(c)) { printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); fails++; } } while (0)

static std::vector<byte> gen(int kind, size_t n, unsigned seed)
{
    std::vector<byte> v(n);
    unsigned x = seed * 2654435761u + 12345u;
    for (size_t i = 0; i < n; i++) {
        x = x * 1664525u + 1013904223u;
        switch (kind) {
        case 0: v[i] = byte(x >> 24); break;                                   // random
        case 1: v[i] = byte(65 + ((x >> 24) % 4)); break;                      // small alphabet
        case 2: v[i] = byte((i / 37) & 1 ? 0 : (x >> 28)); break;              // zero heavy
        default: v[i] = byte(7); break;                                        // one symbol
        }
    }
    return v;
}

template <class F> static std::string refusal(F f)
{
    try { f(); } catch (const std::invalid_argument& e) { return e.what(); }
    return "";
}

int main()
{
    for (int viaFactory = 0; viaFactory < 2; viaFactory++) {
        for (int kind = 0; kind < 4; kind++) {
            for (size_t n : { size_t(1), size_t(20), size_t(4096), size_t(32769), size_t(100000) }) {
                std::vector<byte> in = gen(kind, n, unsigned(kind + n));
                std::stringstream ss;
                Context ctx;
                {
                    DefaultOutputBitStream obs(ss, 16384);
                    obs.writeBits(uint64(5), 3);                               // the codec starts at a non-aligned bit
                    EntropyEncoder* ee = viaFactory ? EntropyEncoderFactory::newEncoder(obs, ctx, EntropyEncoderFactory::RANGE_TYPE) : new RangeEncoder(obs);
                    CHECK(ee->encode(in.data(), 0, uint(n)) == int(n));
                    ee->dispose();
                    delete ee;
                    obs.close();
                }
                std::vector<byte> out(n);
                DefaultInputBitStream ibs(ss, 16384);
                CHECK(ibs.readBits(3) == 5);
                EntropyDecoder* ed = viaFactory ? EntropyDecoderFactory::newDecoder(ibs, ctx, EntropyEncoderFactory::RANGE_TYPE) : new RangeDecoder(ibs);
                CHECK(ed->decode(out.data(), 0, uint(n)) == int(n));
                ed->dispose();
                delete ed;
                CHECK(memcmp(out.data(), in.data(), n) == 0);
            }
        }
    }
    CHECK(EntropyEncoderFactory::getType("range") == EntropyEncoderFactory::RANGE_TYPE && std::string(EntropyEncoderFactory::getName(4)) == "RANGE");

    // constructor checks: the reference's messages, then the refusal of valid values the kernels are not built for
    std::stringstream ss;
    DefaultOutputBitStream obs(ss, 16384);
    DefaultInputBitStream ibs(ss, 16384);
    CHECK(refusal([&] { RangeEncoder e(obs, 1023); }) == "The chunk size must be at least 1024");
    CHECK(refusal([&] { RangeEncoder e(obs, (1 << 30) + 1); }) == "The chunk size must be at most 2^30");
    CHECK(refusal([&] { RangeEncoder e(obs, 1 << 15, 7); }) == "Invalid range parameter: 7 (must be in [8..15])");
    CHECK(refusal([&] { RangeEncoder e(obs, 1 << 15, 16); }) == "Invalid range parameter: 16 (must be in [8..15])");
    CHECK(refusal([&] { RangeDecoder d(ibs, 1023); }) == "The chunk size must be at least 1024");
    CHECK(refusal([&] { RangeDecoder d(ibs, (1 << 30) + 1); }) == "The chunk size must be at most 2^30");
    CHECK(!refusal([&] { RangeEncoder e(obs, 1 << 16); }).empty());
    CHECK(!refusal([&] { RangeEncoder e(obs, 1 << 15, 11); }).empty());
    CHECK(!refusal([&] { RangeDecoder d(ibs, 1 << 14); }).empty());
    CHECK(refusal([&] { RangeEncoder e(obs); RangeDecoder d(ibs); }).empty());

    // the stream classes with "RANGE"
    {
        std::vector<byte> in = gen(2, 3 * 65536 + 777, 9);
        std::stringstream s2;
        {
            CompressedOutputStream cos(s2, 2, "RANGE", "BWT+MTFT+ZRLT", 65536, 32);
            cos.write(reinterpret_cast<const char*>(in.data()), std::streamsize(in.size()));
            cos.close();
        }
        CompressedInputStream cis(s2, 2);
        std::vector<byte> out(in.size() + 16);
        cis.read(reinterpret_cast<char*>(out.data()), std::streamsize(out.size()));
        CHECK(size_t(cis.gcount()) == in.size() && memcmp(out.data(), in.data(), in.size()) == 0);
        cis.close();
    }
    printf(fails ? "FAILED %d checks\n" : "OK\n", fails);
    return fails ? 1 : 0;
}
