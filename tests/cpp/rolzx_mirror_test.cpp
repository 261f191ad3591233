// ROLZCodec of the C++ host mirror (include/kanzi_amd.hpp): the constructors (the Context's "transform" string picks ROLZX, anything
// else is ROLZ, which has no device kernel and is refused), getMaxEncodedLength, the data type written back, and round trips directly,
// through TransformFactory and through the stream classes. Runs on the GPU box (tests/test_gpu_rolzx.py drives it); returns 0 / non-zero.
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
        case 1: v[i] = byte("ACGT"[(x >> 24) % 4]); break;                     // DNA for detectSimpleType
        default: v[i] = byte(i % 11 == 0 ? 32 : 97 + ((i * 7 + (i / 61) * 3) % 23)); break;      // text-like with spaces (letters alone would be BASE64 for detectSimpleType)
        }
    }
    return v;
}

template <class F> static std::string refusal(F f)
{
    try { f(); } catch (const std::invalid_argument& e) { return e.what(); }
    return "";
}

static bool roundTrip(Transform<byte>& t, const std::vector<byte>& in, int maxEnc)
{
    std::vector<byte> mid(size_t(maxEnc) + 16), out(in.size() + 16);
    SliceArray<byte> a(const_cast<byte*>(in.data()), int(in.size()), 0), b(mid.data(), maxEnc, 0);
    if (!t.forward(a, b, int(in.size()))) return false;
    const int n = b._index;
    CHECK(a._index == int(in.size()) && n < int(in.size()));
    SliceArray<byte> c(mid.data(), n, 0), d(out.data(), int(in.size()), 0);
    CHECK(t.inverse(c, d, n));
    CHECK(d._index == int(in.size()) && memcmp(out.data(), in.data(), in.size()) == 0);
    return true;
}

int main()
{
    // constructors: ROLZCodec.cpp:40-50
    CHECK(refusal([] { ROLZCodec c; }).find("ROLZ has no device kernel") != std::string::npos);
    CHECK(refusal([] { ROLZCodec c(5u); }).find("ROLZ has no device kernel") != std::string::npos);
    Context none, rolz, rolzx;
    rolz.putString("transform", "TEXT+ROLZ");
    rolzx.putString("transform", "PACK+ROLZX");
    CHECK(refusal([&] { ROLZCodec c(none); }).find("ROLZ has no device kernel") != std::string::npos);
    CHECK(refusal([&] { ROLZCodec c(rolz); }).find("ROLZ has no device kernel") != std::string::npos);
    CHECK(refusal([&] { delete TransformFactory<byte>::newTransform(rolz, TransformFactory<byte>::getType("ROLZ")); }).find("ROLZ") != std::string::npos);
    CHECK(TransformFactory<byte>::getType("ROLZX") >> TransformFactory<byte>::MAX_SHIFT == 12 && TransformFactory<byte>::getName(TransformFactory<byte>::getType("ROLZX+RLT")) == "ROLZX+RLT");
    {
        ROLZCodec c(rolzx);
        // ROLZCodec.hpp:168-173
        CHECK(c.getMaxEncodedLength(100) == 1124 && c.getMaxEncodedLength(32767) == 33791 && c.getMaxEncodedLength(32768) == 33792 && c.getMaxEncodedLength(1 << 20) == (1 << 20) + 32768);
        std::vector<byte> text = gen(2, 20000, 1), dna = gen(1, 5000, 2), rnd = gen(0, 5000, 3), tiny = gen(2, 63, 4);
        CHECK(roundTrip(c, text, c.getMaxEncodedLength(int(text.size()))));
        CHECK(rolzx.getInt("dataType", 0) == 0);                                  // nothing detected: nothing written
        CHECK(roundTrip(c, dna, c.getMaxEncodedLength(int(dna.size()))));
        CHECK(rolzx.getInt("dataType", 0) == 6);                                  // DNA (Global::DataType), written back
        rolzx.putInt("dataType", 0);
        CHECK(!roundTrip(c, rnd, c.getMaxEncodedLength(int(rnd.size()))));        // no gain: refused
        CHECK(!roundTrip(c, tiny, c.getMaxEncodedLength(int(tiny.size()))));      // below 64 bytes: refused
        CHECK(!roundTrip(c, text, c.getMaxEncodedLength(int(text.size())) - 1));  // a destination below the bound: refused
        rolzx.putInt("dataType", 0);
    }
    {
        // through the factory: the context's "transform" is what the stream classes put there
        Context ctx;
        ctx.putString("transform", "ROLZX+RLT");
        ctx.putString("entropy", "FPAQ");
        TransformSequence<byte>* seq = TransformFactory<byte>::newTransform(ctx, TransformFactory<byte>::getType("ROLZX+RLT"));
        std::vector<byte> in = gen(2, 30000, 5), mid(size_t(seq->getMaxEncodedLength(30000)) + 16), out(in.size() + 16);
        SliceArray<byte> a(in.data(), int(in.size()), 0), b(mid.data(), seq->getMaxEncodedLength(30000), 0);
        CHECK(seq->forward(a, b, int(in.size())));
        const int n = b._index;
        const byte skip = seq->getSkipFlags();
        CHECK((skip & 0x80) == 0);                                                // ROLZX applied
        seq->setSkipFlags(skip);
        SliceArray<byte> c(mid.data(), n, 0), d(out.data(), int(in.size()), 0);
        CHECK(seq->inverse(c, d, n));
        CHECK(d._index == int(in.size()) && memcmp(out.data(), in.data(), in.size()) == 0);
        delete seq;
    }
    // the stream classes: ROLZX alone, behind PACK, in front of RLT, behind the host stage
    for (const char* chain : { "ROLZX", "PACK+ROLZX", "ROLZX+RLT", "TEXT+ROLZX" }) {
        for (int kind : { 2, 1, 0 }) {
            std::vector<byte> in = gen(kind, 2 * 65536 + 777, 9);
            std::stringstream s2;
            {
                CompressedOutputStream cos(s2, 2, "HUFFMAN", chain, 65536, 32);
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
    {
        // a stream that names ROLZ: the device library refuses the chain
        std::stringstream s2;
        std::string what;
        try { CompressedOutputStream cos(s2, 1, "NONE", "ROLZ", 65536, 0); char z[100] = { 0 }; cos.write(z, 100); cos.close(); }
        catch (const std::exception& e) { what = e.what(); }
        CHECK(what.find("11") != std::string::npos);
    }
    printf(fails ? "FAILED %d checks\n" : "OK\n", fails);
    return fails ? 1 : 0;
}
