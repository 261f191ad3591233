// TPAQPredictor<false / true> / BinaryEntropyEncoder / BinaryEntropyDecoder of the C++ host mirror (include/kanzi_amd.hpp) the way
// src/test/TestEntropyCodec.cpp exercises the reference's: round trips from a bit offset, directly and through the factories and the
// stream classes, and the constructor checks. Runs on the GPU box (tests/test_gpu_tpaq.py drives it); returns 0 / non-zero.
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
        default: v[i] = byte((i / 37) & 1 ? 0 : (x >> 28)); break;             // zero heavy
        }
    }
    return v;
}

template <class F> static std::string refusal(F f)
{
    try { f(); } catch (const std::invalid_argument& e) { return e.what(); }
    return "";
}

static Predictor* make(bool x, Context& ctx) { return x ? static_cast<Predictor*>(new TPAQPredictor<true>(&ctx)) : new TPAQPredictor<false>(&ctx); }

// the bytes an encoder writes for `in` in a stream of block size bs
static std::string code(bool x, bool viaFactory, const std::vector<byte>& in, int bs)
{
    Context ctx;
    ctx.putInt("bsVersion", 6);
    ctx.putInt("blockSize", bs);
    ctx.putInt("size", int(in.size()));
    const short type = x ? EntropyEncoderFactory::TPAQX_TYPE : EntropyEncoderFactory::TPAQ_TYPE;
    std::stringstream ss;
    {
        DefaultOutputBitStream obs(ss, 16384);
        obs.writeBits(uint64(5), 3);                               // the codec starts at a non-aligned bit
        EntropyEncoder* ee = viaFactory ? EntropyEncoderFactory::newEncoder(obs, ctx, type) : new BinaryEntropyEncoder(obs, make(x, ctx));
        CHECK(ee->encode(in.data(), 0, uint(in.size())) == int(in.size()));
        ee->dispose();
        delete ee;
        obs.close();
    }
    const std::string bytes = ss.str();
    std::vector<byte> out(in.size());
    DefaultInputBitStream ibs(ss, 16384);
    CHECK(ibs.readBits(3) == 5);
    EntropyDecoder* ed = viaFactory ? EntropyDecoderFactory::newDecoder(ibs, ctx, type) : new BinaryEntropyDecoder(ibs, make(x, ctx));
    CHECK(ed->decode(out.data(), 0, uint(in.size())) == int(in.size()));
    ed->dispose();
    delete ed;
    CHECK(memcmp(out.data(), in.data(), in.size()) == 0);
    return bytes;
}

int main()
{
    for (int x = 0; x < 2; x++)
        for (int viaFactory = 0; viaFactory < 2; viaFactory++)
            for (int kind = 0; kind < 3; kind++)
                for (size_t n : { size_t(1), size_t(20), size_t(65), size_t(4097) })
                    code(x != 0, viaFactory != 0, gen(kind, n, unsigned(kind + n)), 65536);
    // the stream's block size reaches the device: 10,000 (masks 9,999 and 159,999) codes the same bytes differently from 65,536,
    // and each decodes with its own
    {
        std::vector<byte> in = gen(1, 9000, 3);
        CHECK(code(false, false, in, 10000) != code(false, false, in, 65536));
        CHECK(code(true, true, in, 10000) != code(true, true, in, 65536));
    }
    CHECK(EntropyEncoderFactory::getType("tpaq") == EntropyEncoderFactory::TPAQ_TYPE && std::string(EntropyEncoderFactory::getName(7)) == "TPAQ");
    CHECK(EntropyEncoderFactory::getType("TPAQX") == EntropyEncoderFactory::TPAQX_TYPE && std::string(EntropyEncoderFactory::getName(9)) == "TPAQX");

    // constructor checks
    std::stringstream ss;
    DefaultOutputBitStream obs(ss, 16384);
    DefaultInputBitStream ibs(ss, 16384);
    Context v6, v7, none;
    v6.putInt("bsVersion", 6);
    v7.putInt("bsVersion", 7);
    CHECK(refusal([&] { TPAQPredictor<false> p; }).find("without a Context") != std::string::npos);
    CHECK(refusal([&] { TPAQPredictor<true> p; }).find("without a Context") != std::string::npos);
    CHECK(refusal([&] { TPAQPredictor<false> p(&v7); }).find("version 7") != std::string::npos);
    CHECK(refusal([&] { TPAQPredictor<true> p(&none); }).find("version 7") != std::string::npos);      // (the reference's default is 7)
    CHECK(refusal([&] { EntropyEncoderFactory::newEncoder(obs, none, EntropyEncoderFactory::TPAQ_TYPE); }).find("version 7") != std::string::npos);
    CHECK(refusal([&] { EntropyDecoderFactory::newDecoder(ibs, v7, EntropyEncoderFactory::TPAQX_TYPE); }).find("version 7") != std::string::npos);
    {
        // defaults of the reference: "blockSize" 32768, "size" the block size
        TPAQPredictor<false> p(&v6);
        CHECK(p.blockSize() == 32768 && p.size() == 32768);
        bool threw = false;
        try { p.get(); } catch (const std::logic_error&) { threw = true; }
        CHECK(threw);
        // a length other than the Context's "size" is refused: the device sizes the tables by the length it is given
        byte b[100] = { 0 };
        CHECK(!refusal([&] { BinaryEntropyEncoder e(obs, &p, false); e.encode(b, 0, 100); }).empty());
    }

    // the stream classes with both coders: zero-heavy bytes, and random ones (which do not compress: with KNZ_CM_TIER1_DIV set, as
    // tests/test_gpu_tpaq.py runs this program a second time, the batch takes the second tier)
    for (const char* coder : { "TPAQ", "TPAQX" }) {
        for (int kind : { 2, 0 }) {
            std::vector<byte> in = gen(kind, 2 * 4096 + 777, 9);
            std::stringstream s2;
            {
                CompressedOutputStream cos(s2, 2, coder, "BWT+RANK+ZRLT", 4096, 32);
                cos.write(reinterpret_cast<const char*>(in.data()), std::streamsize(in.size()));
                cos.close();
            }
            CompressedInputStream cis(s2, 2);
            std::vector<byte> out(in.size() + 16);
            cis.read(reinterpret_cast<char*>(out.data()), std::streamsize(out.size()));
            CHECK(size_t(cis.gcount()) == in.size() && memcmp(out.data(), in.data(), in.size()) == 0);
            cis.close();
        }
    }
    printf(fails ? "FAILED %d checks\n" : "OK\n", fails);
    return fails ? 1 : 0;
}
