// CMPredictor / BinaryEntropyEncoder / BinaryEntropyDecoder of the C++ host mirror (include/kanzi_amd.hpp) the way
// src/test/TestEntropyCodec.cpp exercises the reference's: round trips from a bit offset, directly and through the factories and the
// stream classes, and the constructor checks. Runs on the GPU box (tests/test_gpu_cm.py drives it); returns 0 / non-zero.
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

struct Other : Predictor { void update(int) {} int get() { return 2048; } };

int main()
{
    Context ctx;
    ctx.putInt("bsVersion", 6);
    for (int viaFactory = 0; viaFactory < 2; viaFactory++) {
        for (int kind = 0; kind < 4; kind++) {
            for (size_t n : { size_t(1), size_t(20), size_t(65), size_t(4097), size_t(20000) }) {
                std::vector<byte> in = gen(kind, n, unsigned(kind + n));
                std::stringstream ss;
                {
                    DefaultOutputBitStream obs(ss, 16384);
                    obs.writeBits(uint64(5), 3);                               // the codec starts at a non-aligned bit
                    EntropyEncoder* ee = viaFactory ? EntropyEncoderFactory::newEncoder(obs, ctx, EntropyEncoderFactory::CM_TYPE)
                                                    : new BinaryEntropyEncoder(obs, new CMPredictor(&ctx));
                    CHECK(ee->encode(in.data(), 0, uint(n)) == int(n));
                    ee->dispose();
                    delete ee;
                    obs.close();
                }
                std::vector<byte> out(n);
                DefaultInputBitStream ibs(ss, 16384);
                CHECK(ibs.readBits(3) == 5);
                EntropyDecoder* ed = viaFactory ? EntropyDecoderFactory::newDecoder(ibs, ctx, EntropyEncoderFactory::CM_TYPE)
                                                : new BinaryEntropyDecoder(ibs, new CMPredictor(&ctx));
                CHECK(ed->decode(out.data(), 0, uint(n)) == int(n));
                ed->dispose();
                delete ed;
                CHECK(memcmp(out.data(), in.data(), n) == 0);
            }
        }
    }
    CHECK(EntropyEncoderFactory::getType("cm") == EntropyEncoderFactory::CM_TYPE && std::string(EntropyEncoderFactory::getName(6)) == "CM");

    // the predictor on its own: the first split is 2048 + 1 / 2 rounded as get() rounds, and a run of ones raises it
    {
        CMPredictor p(&ctx);
        const int first = p.get();
        CHECK(first == (32768 + 32768 + 3 * (32768 + 36864) + 64) >> 7);
        for (int i = 0; i < 64; i++) { p.get(); p.update(1); }
        CHECK(p.get() > first && p.get() <= 4095);
    }

    // constructor checks: a predictor that would stand for the table of version 7, a null predictor, a predictor without a kernel
    std::stringstream ss;
    DefaultOutputBitStream obs(ss, 16384);
    DefaultInputBitStream ibs(ss, 16384);
    Context v7, none;
    v7.putInt("bsVersion", 7);
    CHECK(refusal([&] { CMPredictor p; }).find("without a Context") != std::string::npos);
    CHECK(refusal([&] { CMPredictor p(&v7); }).find("version 7") != std::string::npos);
    CHECK(refusal([&] { CMPredictor p(&none); }).find("version 7") != std::string::npos);      // (the reference's default is 7)
    CHECK(refusal([&] { EntropyEncoderFactory::newEncoder(obs, none, EntropyEncoderFactory::CM_TYPE); }).find("version 7") != std::string::npos);
    CHECK(refusal([&] { BinaryEntropyEncoder e(obs, nullptr); }) == "Invalid null predictor parameter");
    CHECK(refusal([&] { BinaryEntropyDecoder d(ibs, nullptr); }) == "Invalid null predictor parameter");
    { Other other; CHECK(!refusal([&] { BinaryEntropyEncoder e(obs, &other, false); }).empty()); }
    { CMPredictor keep(&ctx); CHECK(refusal([&] { BinaryEntropyEncoder e(obs, &keep, false); BinaryEntropyDecoder d(ibs, &keep, false); }).empty()); }

    // the stream classes with "CM": zero-heavy bytes, and random ones (which do not compress: with KNZ_CM_TIER1_DIV set, as
    // tests/test_gpu_cm.py runs this program a second time, the batch takes the second tier)
    for (int kind : { 2, 0 }) {
        std::vector<byte> in = gen(kind, 3 * 16384 + 777, 9);
        std::stringstream s2;
        {
            CompressedOutputStream cos(s2, 2, "CM", "BWT+RANK+ZRLT", 16384, 32);
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
