// CPU-only check of the many-stream framing (kanzi-cpp_amd/csrc/streams.hip compiled as plain C++ against tools/hipemu): the segmented
// framing scan and the multi-stream walk against today's single-stream kernels (k_block_scan / k_walk_blocks of bitasm.hip, run here one
// stream at a time on a copy of that stream alone). Test infrastructure only.
//   usage: streams_emu            every case below; prints OK <cases>
#include "hip/hip_runtime.h"
#include "../../kanzi-cpp_amd/csrc/bitasm.hip"
#include "../../kanzi-cpp_amd/csrc/streams.hip"

#include <stdio.h>
#include <random>
#include <vector>

namespace knz { thread_local ProfHook* g_prof = nullptr; }
using namespace knz;

static int g_bad = 0;
static int g_verdicts[4] = { 0, 0, 0, 0 };      // streams the walk accepted / refused as unreadable / as too long for their room / otherwise (none: a length field holds no more than the format allows)
#define CHECK(cond, ...) do { if (!(cond)) { if (g_bad < 20) { printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } g_bad++; } } while (0)

struct WalkRes { u64 endBit; int64_t nBlocks; int32_t ended; int32_t error; };

// ---------------------------------------------------------------- the framing scan
// empties: 0 = blocks per stream at random (0-5), 1 = the first, the middle and the last stream empty, 2 = every stream empty
// big: payloads of about 2^31 bits each (no bytes behind them: the scan only adds lengths), so that the batch crosses 2^32 bits early
static void frame_case(int nItems, unsigned seed, int empties, bool big)
{
    std::mt19937_64 rng(seed);
    FrameParams fp;
    fp.framing = 1; fp.nTransforms = (seed & 1) ? 5 : 3; fp.checksumBits = (int)(seed % 3) * 32; fp.finish = (int)((seed >> 2) & 1); fp.prologueBits = 0;
    std::vector<StreamEnc> st((size_t)nItems + 1);
    std::vector<u32> itemOf, blockLen, origLen;
    std::vector<BlockInfo> info;
    for (int i = 0; i < nItems; i++) {
        int nb = (int)(rng() % 6);
        if (empties == 2 || (empties == 1 && (i == 0 || i == nItems / 2 || i == nItems - 1))) nb = 0;
        st[(size_t)i].first = (u32)info.size();
        st[(size_t)i].prologueBits = (rng() % 4 == 0) ? 0u : (u32)(rng() % 1601);
        st[(size_t)i].prologueOff = 0; st[(size_t)i].pad = 0;
        for (int k = 0; k < nb; k++) {
            BlockInfo bi; memset(&bi, 0, sizeof(bi));
            const u32 kind = (u32)(rng() % 4);
            const u32 len = kind == 0 ? 1 + (u32)(rng() % 15) : kind == 1 ? 1 + (u32)(rng() % 255) : kind == 2 ? 256 + (u32)(rng() % 65000) : 65536 + (u32)(rng() % 200000);
            bi.payloadBits = big ? (1ull << 31) + rng() % (1ull << 30) : (kind == 0 ? 8ull * len : rng() % (9ull * len + 64));
            bi.written = bi.bitOff = 0xDEADBEEFull; bi.hdrBits = bi.lw = 0xABCDu;
            info.push_back(bi);
            blockLen.push_back(len);
            origLen.push_back(kind == 0 ? len : len + (u32)(rng() % 100));
            itemOf.push_back((u32)i);
        }
    }
    const int nBlocks = (int)info.size();
    st[(size_t)nItems].first = (u32)nBlocks; st[(size_t)nItems].prologueBits = st[(size_t)nItems].prologueOff = st[(size_t)nItems].pad = 0;
    // today's scan, stream by stream
    std::vector<BlockInfo> want = info;
    std::vector<u64> wantBits((size_t)nItems), wantBase((size_t)nItems);
    u64 at = 0;
    for (int i = 0; i < nItems; i++) {
        const u32 b0 = st[(size_t)i].first, nb = st[(size_t)i + 1].first - b0;
        FrameParams f1 = fp; f1.prologueBits = st[(size_t)i].prologueBits;
        u64 total = 0;
        if (nb) launch_block_scan(nullptr, want.data() + b0, blockLen.data() + b0, origLen.data() + b0, (int)nb, f1, &total);
        else total = (u64)f1.prologueBits + (fp.finish ? 8 : 0);
        wantBits[(size_t)i] = total; wantBase[(size_t)i] = at;
        for (u32 b = b0; b < b0 + nb; b++) want[b].bitOff += 8 * at;
        at += (((total + 7) >> 3) + 15) & ~15ull;
    }
    std::vector<u64> excl((size_t)nBlocks + 1, 0x5555555555555555ull);
    std::vector<StreamOut> res((size_t)nItems + 1);
    u64 totalBytes = ~0ull;
    info.reserve(info.size() + 1); blockLen.reserve(blockLen.size() + 1); origLen.reserve(origLen.size() + 1); itemOf.reserve(itemOf.size() + 1);
    launch_stream_frame(nullptr, info.data(), blockLen.data(), origLen.data(), itemOf.data(), nBlocks, st.data(), nItems, fp, excl.data(), res.data(), &totalBytes);
    CHECK(totalBytes == at, "frame n=%d seed=%u: total %llu, want %llu", nItems, seed, (unsigned long long)totalBytes, (unsigned long long)at);
    if (big && nItems > 4) CHECK(8 * at > (1ull << 33), "the big case does not cross 2^32 bits");
    for (int i = 0; i < nItems; i++)
        CHECK(res[(size_t)i].base == wantBase[(size_t)i] && res[(size_t)i].bits == wantBits[(size_t)i] && (res[(size_t)i].base & 15) == 0,
              "frame n=%d seed=%u stream %d: base %llu bits %llu, want %llu %llu", nItems, seed, i, (unsigned long long)res[(size_t)i].base,
              (unsigned long long)res[(size_t)i].bits, (unsigned long long)wantBase[(size_t)i], (unsigned long long)wantBits[(size_t)i]);
    for (int b = 0; b < nBlocks; b++)
        CHECK(info[(size_t)b].bitOff == want[(size_t)b].bitOff && info[(size_t)b].written == want[(size_t)b].written && info[(size_t)b].lw == want[(size_t)b].lw &&
              info[(size_t)b].hdrBits == want[(size_t)b].hdrBits && info[(size_t)b].payloadBits == want[(size_t)b].payloadBits,
              "frame n=%d seed=%u block %d: bitOff %llu written %llu lw %u hdr %u, want %llu %llu %u %u", nItems, seed, b, (unsigned long long)info[(size_t)b].bitOff,
              (unsigned long long)info[(size_t)b].written, info[(size_t)b].lw, info[(size_t)b].hdrBits, (unsigned long long)want[(size_t)b].bitOff,
              (unsigned long long)want[(size_t)b].written, want[(size_t)b].lw, want[(size_t)b].hdrBits);
}

// ---------------------------------------------------------------- the walk
struct BitW {
    std::vector<u8> v; u64 n = 0;
    void put(u64 val, u32 bits) { for (u32 i = bits; i-- > 0;) { if ((n & 7) == 0) v.push_back(0); if ((val >> i) & 1) v[n >> 3] |= (u8)(0x80 >> (n & 7)); n++; } }
};

// damage: 0 none, 1 some streams with flipped bits in their length prefixes, cut short, or without room for their blocks
static void walk_case(int nItems, unsigned seed, int empties, int damage)
{
    std::mt19937_64 rng(seed);
    const u32 bs = 1024;
    const int checksumBits = (int)(seed % 3) * 32;
    std::vector<StreamDec> sd((size_t)nItems);
    std::vector<u8> in;
    std::vector<std::vector<u8>> alone((size_t)nItems);
    u64 outAt = 0;
    for (int i = 0; i < nItems; i++) {
        int nb = (int)(rng() % 6);
        if (empties == 2 || (empties == 1 && (i == 0 || i == nItems / 2 || i == nItems - 1))) nb = 0;
        BitW w;
        const u32 hdr = (u32)(rng() % 3) * 8 * (u32)(rng() % 20);          // a byte-aligned header in front, or none
        for (u32 k = 0; k < hdr; k += 8) w.put(rng() & 0xFF, 8);
        std::vector<u64> prefixAt;
        for (int k = 0; k < nb; k++) {
            const bool last = k + 1 == nb;
            const u32 pre = last ? 1 + (u32)(rng() % bs) : bs;
            const bool copy = pre <= 15;
            const bool skipByte = !copy && (rng() & 1);
            const u32 ds = pre < 256 ? 1 : 2;
            const u32 fill = (u32)(rng() % 300);
            const u64 len = 8 + (skipByte ? 8 : 0) + 8 * ds + (u64)checksumBits + fill;
            const u32 lw = len < 8 ? 3 : (u32)(31 - __builtin_clz((u32)(len >> 3))) + 4;
            prefixAt.push_back(w.n);
            w.put(lw - 3, 5); w.put(len, lw);
            w.put((copy ? 0x80u : 0u) | (skipByte ? 0x10u : (u32)(rng() & 0x0F)) | ((ds - 1) << 5), 8);
            if (skipByte) w.put(rng() & 0xFF, 8);
            w.put(pre, 8 * ds);
            if (checksumBits) w.put(rng() & ((1ull << checksumBits) - 1), (u32)checksumBits);
            for (u32 f = 0; f < fill; f++) w.put(rng() & 1, 1);
        }
        const bool marker = rng() % 8 != 0;                                 // (a stream may end at its bit limit without a marker)
        if (damage && rng() % 16 == 0) { w.put(31, 5); w.put((1ull << 33) + 5, 34); }      // the widest length field: a block far beyond the stream
        if (marker) w.put(0, 8);
        u64 bits = w.n;
        u64 cap = (u64)(nb ? (nb - 1) * bs + 1 + rng() % bs : 0) + (rng() & 1 ? bs : 0);
        if (nb && !(rng() & 3)) cap = (u64)nb * bs;
        if (damage && rng() % 3 == 0) {
            const u32 how = (u32)(rng() % 4);
            if (how == 0 && !prefixAt.empty()) { const u64 at = prefixAt[rng() % prefixAt.size()] + rng() % 9; w.v[at >> 3] ^= (u8)(0x80 >> (at & 7)); }
            else if (how == 1 && bits > hdr + 1) bits = hdr + rng() % (bits - hdr);
            else if (how == 2 && nb > 1) cap = (u64)(nb - 2) * bs + rng() % bs;
            else if (how == 3 && nb > 2) cap = rng() % bs;
        }
        while (in.size() & 15) in.push_back(0xFF);
        StreamDec& d = sd[(size_t)i];
        d.inOff = in.size(); d.inBits = bits; d.startBit = hdr; d.outOff = outAt; d.outCap = cap;
        outAt += (cap + 15) & ~15ull;
        const size_t bytes = (size_t)((bits + 7) >> 3);
        alone[(size_t)i].assign(w.v.begin(), w.v.begin() + (long)std::min(bytes, w.v.size()));
        alone[(size_t)i].resize(bytes + 64, 0);
        // behind the stream's bits: ones where its neighbours would be, zeros in its copy -- a read behind the limit would tell
        std::vector<u8> placed(alone[(size_t)i].begin(), alone[(size_t)i].begin() + (long)bytes);
        if (bits & 7) placed[bytes - 1] |= (u8)(0xFF >> (bits & 7));
        in.insert(in.end(), placed.begin(), placed.end());
    }
    in.resize(in.size() + 64, 0xFF);
    std::vector<StreamWalk> res((size_t)nItems + 1);
    launch_walk_streams_count(nullptr, in.data(), sd.data(), nItems, checksumBits, bs, res.data());
    const u64 all = res[(size_t)nItems].first;
    std::vector<DecBlock> blocks((size_t)all + 1);
    std::vector<u64> outOff((size_t)all + 1, ~0ull), room((size_t)all + 1, ~0ull);
    memset(blocks.data(), 0xEE, sizeof(DecBlock) * blocks.size());
    launch_walk_streams_fill(nullptr, in.data(), sd.data(), nItems, checksumBits, bs, res.data(), blocks.data(), outOff.data(), room.data());
    u64 first = 0;
    for (int i = 0; i < nItems; i++) {
        const StreamDec& d = sd[(size_t)i];
        BitSrc src; src.words = reinterpret_cast<const u32*>(alone[(size_t)i].data()); src.nBytes = (d.inBits + 7) >> 3; src.nWords = src.nBytes >> 2; src.limitBits = d.inBits;
        const int64_t most = (int64_t)(d.outCap / bs) + 2;
        std::vector<DecBlock> ref((size_t)most);
        WalkRes wr; memset(&wr, 0, sizeof(wr));
        launch_walk_blocks(nullptr, src, d.startBit, most, 1, 0, checksumBits, bs, ref.data(), &wr);
        int error = wr.error;
        if (!error && (u64)wr.nBlocks * bs > d.outCap + bs) error = KNZ_ERR_WRITE_FILE;
        const u32 count = error ? 0u : (u32)wr.nBlocks;
        g_verdicts[error == 0 ? 0 : error == KNZ_ERR_READ_FILE ? 1 : error == KNZ_ERR_WRITE_FILE ? 2 : 3]++;
        const StreamWalk& g = res[(size_t)i];
        CHECK(g.error == error && g.count == count && g.first == first && (error || g.ended == wr.ended),
              "walk n=%d seed=%u stream %d: error %d count %u first %llu ended %d, want %d %u %llu %d", nItems, seed, i, g.error, g.count,
              (unsigned long long)g.first, g.ended, error, count, (unsigned long long)first, wr.ended);
        for (u32 k = 0; k < count && g.count == count && g.first == first; k++) {
            const DecBlock& a = blocks[(size_t)first + k];
            const DecBlock& r = ref[k];
            CHECK(a.payloadBit == r.payloadBit + 8 * d.inOff && a.entropyBit == r.entropyBit + 8 * d.inOff && a.bits == r.bits && a.checksum == r.checksum &&
                  a.preLen == r.preLen && a.skipFlags == r.skipFlags && a.copyBlock == r.copyBlock && a.error == r.error && a.usedBits == 0,
                  "walk n=%d seed=%u stream %d block %u differs", nItems, seed, i, k);
            const u64 at = (u64)k * bs;
            CHECK(outOff[(size_t)first + k] == d.outOff + at && room[(size_t)first + k] == (d.outCap > at ? d.outCap - at : 0), "walk n=%d seed=%u stream %d block %u: place", nItems, seed, i, k);
        }
        first += count;
    }
    CHECK(all == first, "walk n=%d seed=%u: %llu blocks, want %llu", nItems, seed, (unsigned long long)all, (unsigned long long)first);
    CHECK(blocks[(size_t)all].payloadBit == 0xEEEEEEEEEEEEEEEEull && outOff[(size_t)all] == ~0ull, "walk n=%d seed=%u: a slot behind the last block was written", nItems, seed);
}

int main()
{
    int cases = 0;
    const int sizes[] = { 1, 63, 64, 65, 257, 1000 };
    unsigned seed = 1;
    for (int n : sizes)
        for (int empties = 0; empties < 3; empties++) {
            frame_case(n, seed++, empties, false);
            frame_case(n, seed++, empties, false);
            walk_case(n, seed++, empties, 0);
            walk_case(n, seed++, empties, 1);
            cases += 4;
        }
    for (int n : { 3, 65, 1000 }) { frame_case(n, seed++, 1, true); cases++; }      // totals beyond 2^32 bits
    frame_case(0, seed++, 0, false); walk_case(0, seed++, 0, 0); cases += 2;         // no stream at all
    for (int k = 0; k < 6; k++) { walk_case(300, seed++, 0, 1); cases++; }
    // (the damaged cases must have met every verdict, or they test nothing)
    if (!g_verdicts[0] || !g_verdicts[1] || !g_verdicts[2]) { printf("FAIL verdicts met: %d ok, %d unreadable, %d too long, %d other\n", g_verdicts[0], g_verdicts[1], g_verdicts[2], g_verdicts[3]); g_bad++; }
    printf(g_bad ? "FAILED %d checks\n" : "OK %d cases (%d / %d / %d / %d streams accepted / unreadable / too long / otherwise refused)\n", g_bad ? g_bad : cases, g_verdicts[0], g_verdicts[1], g_verdicts[2], g_verdicts[3]);
    return g_bad ? 1 : 0;
}
