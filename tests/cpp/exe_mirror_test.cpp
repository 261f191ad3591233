// EXECodec of the C++ host mirror (include/kanzi_amd.hpp): the constructors, getMaxEncodedLength, the data type written back, and round
// trips directly, through TransformFactory and through the stream classes. Runs on the GPU box (tests/test_gpu_exe.py drives it);
// returns 0 / non-zero.
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

// kind 0: x86-like code (30 plain bytes, a call or jump with a rel32 within +-60,000, 6 zero bytes, over and over; the 256 byte values
// once): detectType takes it. kind 1: text. kind 2: random bytes.
static std::vector<byte> gen(int kind, size_t n, unsigned seed)
{
    std::vector<byte> v;
    v.reserve(n + 64);
    unsigned x = seed * 2654435761u + 12345u;
    auto next = [&] { x = x * 1664525u + 1013904223u; return x >> 8; };
    while (v.size() < n) {
        if (kind == 1) { const size_t i = v.size(); v.push_back(byte(i % 11 == 0 ? 32 : 97 + ((i * 7 + (i / 61) * 3) % 23))); continue; }
        if (kind == 2) { v.push_back(byte(next() >> 8)); continue; }
        for (int k = 0; k < 30; k++) {
            unsigned b = 16 + next() % 240;
            if (b == 0x9B || b == 0xE8 || b == 0xE9) b = 0x90;
            v.push_back(byte(b));
        }
        const int rel = int(next() % 120000) - 60000;
        v.push_back(byte(next() & 1 ? 0xE8 : 0xE9));
        for (int k = 0; k < 4; k++) v.push_back(byte(unsigned(rel) >> (8 * k)));
        for (int k = 0; k < 6; k++) v.push_back(byte(0));
    }
    v.resize(n);
    if (kind == 0 && n >= 1024) for (int k = 0; k < 256; k++) v[n / 2 + size_t(k)] = byte(k);
    return v;
}

// forward into maxEnc bytes, then the inverse into a destination of the original length (smaller than its input)
static bool roundTrip(Transform<byte>& t, const std::vector<byte>& in, int maxEnc)
{
    std::vector<byte> mid(size_t(maxEnc) + 16), out(in.size() + 16);
    SliceArray<byte> a(const_cast<byte*>(in.data()), int(in.size()), 0), b(mid.data(), maxEnc, 0);
    if (!t.forward(a, b, int(in.size()))) return false;
    const int n = b._index;
    CHECK(a._index == int(in.size()) && n > int(in.size()) && n <= int(in.size()) + int(in.size()) / 50);
    SliceArray<byte> c(mid.data(), n, 0), d(out.data(), int(in.size()), 0);
    CHECK(t.inverse(c, d, n));
    CHECK(d._index == int(in.size()) && memcmp(out.data(), in.data(), in.size()) == 0);
    return true;
}

int main()
{
    const std::vector<byte> code = gen(0, 20000, 1), text = gen(1, 20000, 2), rnd = gen(2, 20000, 3), small = gen(0, 4095, 4);
    {
        EXECodec c;                                                               // no Context: every block starts UNDEFINED
        // EXECodec.hpp:96-100
        CHECK(c.getMaxEncodedLength(100) == 132 && c.getMaxEncodedLength(256) == 288 && c.getMaxEncodedLength(257) == 289 && c.getMaxEncodedLength(1 << 20) == (1 << 20) + (1 << 17));
        CHECK(roundTrip(c, code, c.getMaxEncodedLength(int(code.size()))));
        CHECK(!roundTrip(c, text, c.getMaxEncodedLength(int(text.size()))));
        CHECK(!roundTrip(c, small, c.getMaxEncodedLength(int(small.size()))));    // below 4,096 bytes: refused
        CHECK(!roundTrip(c, code, c.getMaxEncodedLength(int(code.size())) - 1));  // a destination below the bound: refused
    }
    {
        Context ctx;
        EXECodec c(ctx);
        CHECK(roundTrip(c, code, c.getMaxEncodedLength(int(code.size()))));
        CHECK(ctx.getInt("dataType", 0) == 3);                                    // EXE (Global::DataType), written back
        CHECK(!roundTrip(c, rnd, c.getMaxEncodedLength(int(rnd.size()))));
        CHECK(ctx.getInt("dataType", 0) == 7);                                    // detection rejected the block: BIN overwrites EXE
        CHECK(roundTrip(c, code, c.getMaxEncodedLength(int(code.size()))));       // BIN passes the gate
        CHECK(ctx.getInt("dataType", 0) == 3);
        CHECK(!roundTrip(c, text, c.getMaxEncodedLength(int(text.size()))));
        CHECK(ctx.getInt("dataType", 0) == 0);                                    // ... and so does UNDEFINED
        ctx.putInt("dataType", 1);
        CHECK(!roundTrip(c, code, c.getMaxEncodedLength(int(code.size()))));      // TEXT: refused at the gate, the type stays
        CHECK(ctx.getInt("dataType", 0) == 1);
        ctx.putInt("dataType", 3);
        CHECK(!roundTrip(c, small, c.getMaxEncodedLength(int(small.size()))));    // refused by its size: the type stays
        CHECK(ctx.getInt("dataType", 0) == 3);
    }
    {
        // through the factory
        CHECK(TransformFactory<byte>::getType("EXE") >> TransformFactory<byte>::MAX_SHIFT == 9 && TransformFactory<byte>::getName(TransformFactory<byte>::getType("EXE+RLT")) == "EXE+RLT");
        Context ctx;
        ctx.putString("transform", "EXE+RLT");
        ctx.putString("entropy", "HUFFMAN");
        TransformSequence<byte>* seq = TransformFactory<byte>::newTransform(ctx, TransformFactory<byte>::getType("EXE+RLT"));
        const int cap = seq->getMaxEncodedLength(int(code.size()));
        CHECK(cap == int(code.size()) + int(code.size()) / 8);
        std::vector<byte> in = code, mid(size_t(cap) + 16), out(in.size() + 16);
        SliceArray<byte> a(in.data(), int(in.size()), 0), b(mid.data(), cap, 0);
        CHECK(seq->forward(a, b, int(in.size())));
        const int n = b._index;
        const byte skip = seq->getSkipFlags();
        CHECK((skip & 0x80) == 0);                                                // EXE applied
        CHECK(ctx.getInt("dataType", 0) == 3);
        seq->setSkipFlags(skip);
        SliceArray<byte> c(mid.data(), n, 0), d(out.data(), cap, 0);
        CHECK(seq->inverse(c, d, n));
        CHECK(d._index == int(in.size()) && memcmp(out.data(), in.data(), in.size()) == 0);
        delete seq;
    }
    // the stream classes: EXE alone, in front of RLT, ROLZX (which reads the type EXE leaves) and PACK (which refuses EXE blocks),
    // behind the host stage
    for (const char* chain : { "EXE", "EXE+RLT", "EXE+ROLZX", "EXE+PACK+ZRLT", "TEXT+EXE+RLT" }) {
        for (int kind : { 0, 1, 2 }) {
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
    printf(fails ? "FAILED %d checks\n" : "OK\n", fails);
    return fails ? 1 : 0;
}
