// The stream classes of the C++ host mirror (include/kanzi_amd.hpp) over chains with TEXT on the device: in front of the chain, behind a
// device stage (which the mirror refused before the device had the stage) and twice in one chain, in both encodings, on text and on
// bytes TEXT refuses; and DNA (AliasCodec with packOnlyDNA) through TransformFactory. Runs on the GPU box (tests/test_gpu_text.py drives it); returns 0 / non-zero.
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

// kind 0: words of a small vocabulary with line ends; kind 1: random bytes
static std::vector<byte> gen(int kind, size_t n, unsigned seed)
{
    static const char* words[] = { "the", "quick", "brown", "fox", "jumps", "over", "lazy", "dog", "because", "Through", "zyxwv", "compression", "of", "it" };
    std::vector<byte> v;
    v.reserve(n + 64);
    unsigned x = seed * 2654435761u + 12345u;
    auto next = [&] { x = x * 1664525u + 1013904223u; return x >> 8; };
    while (v.size() < n) {
        if (kind == 1) { v.push_back(byte(next() >> 8)); continue; }
        const char* w = words[next() % 14];
        for (const char* p = w; *p; p++) v.push_back(byte(*p));
        v.push_back(byte(next() % 13 == 0 ? '\n' : ' '));
    }
    v.resize(n);
    return v;
}

int main()
{
    struct { const char* chain; const char* entropy; } cases[] = {
        { "TEXT+UTF+BWT+RANK+ZRLT", "ANS0" }, { "LZP+TEXT+UTF+BWT+LZP", "CM" }, { "RLT+TEXT", "HUFFMAN" }, { "TEXT+RLT+TEXT", "FPAQ" },
        { "EXE+RLT+TEXT+UTF+DNA", "TPAQ" }, { "EXE+RLT+TEXT+UTF+DNA", "TPAQX" }, { "DNA+RLT", "HUFFMAN" },
    };
    for (const auto& cs : cases) {
        for (int kind : { 0, 1 }) {
            std::vector<byte> in = gen(kind, 2 * 65536 + 777, 9);
            std::stringstream s2;
            {
                CompressedOutputStream cos(s2, 2, cs.entropy, cs.chain, 65536, 32);
                cos.write(reinterpret_cast<const char*>(in.data()), std::streamsize(in.size()));
                cos.close();
            }
            if (kind == 0 && strstr(cs.chain, "TEXT")) CHECK(s2.str().size() < in.size() / 2);
            CompressedInputStream cis(s2, 2);
            std::vector<byte> out(in.size() + 16);
            cis.read(reinterpret_cast<char*>(out.data()), std::streamsize(out.size()));
            CHECK(size_t(cis.gcount()) == in.size() && memcmp(out.data(), in.data(), in.size()) == 0);
            cis.close();
        }
    }
    {
        // DNA through the factory: an ACGT block is packed to a quarter and comes back, its type written; text is refused
        CHECK(TransformFactory<byte>::getType("DNA") >> TransformFactory<byte>::MAX_SHIFT == 19 && TransformFactory<byte>::getName(TransformFactory<byte>::getType("DNA+RLT")) == "DNA+RLT");
        for (int kind : { 0, 2 }) {
            Context ctx;
            ctx.putString("transform", "DNA");
            TransformSequence<byte>* seq = TransformFactory<byte>::newTransform(ctx, TransformFactory<byte>::getType("DNA"));
            CHECK(ctx.getInt("packOnlyDNA", 0) == 1);
            std::vector<byte> in = gen(kind, 20000, 5);
            if (kind == 2) for (size_t i = 0; i < in.size(); i++) in[i] = byte("ACGT"[(i * 7 + i / 13 + (i >> 5)) & 3]);
            const int cap = seq->getMaxEncodedLength(int(in.size()));
            CHECK(cap == int(in.size()) + 1024);
            std::vector<byte> mid(size_t(cap) + 16), out(in.size() + 16);
            SliceArray<byte> a(in.data(), int(in.size()), 0), b(mid.data(), cap, 0);
            const bool applied = seq->forward(a, b, int(in.size()));
            CHECK(applied == (kind == 2));                                        // the ACGT block only; text is refused: no stage ran
            if (!applied) { delete seq; continue; }
            const byte skip = seq->getSkipFlags();
            CHECK((skip & 0x80) == 0);
            CHECK(b._index < int(in.size()) / 3);
            CHECK(ctx.getInt("dataType", 0) == 6);
            seq->setSkipFlags(skip);
            SliceArray<byte> c(mid.data(), b._index, 0), d(out.data(), cap, 0);
            CHECK(seq->inverse(c, d, b._index));
            CHECK(d._index == int(in.size()) && memcmp(out.data(), in.data(), in.size()) == 0);
            delete seq;
        }
    }
    printf(fails ? "FAILED %d checks\n" : "OK\n", fails);
    return fails ? 1 : 0;
}
