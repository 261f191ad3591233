// CPU-only check of kanzi-cpp_amd/csrc/prims.hpp (device-wide scans and the segmented LSD radix sort) on the fiber emulation of
// tools/hipemu, against std::stable_sort / plain loops. Built and run by tests/test_emu_kernels.py. Test infrastructure only.
#include "hip/hip_runtime.h"
#include "../../kanzi-cpp_amd/csrc/prims.hpp"

#include <algorithm>
#include <numeric>
#include <random>
#include <vector>
#include <stdio.h>
#include <string.h>

namespace knz { thread_local ProfHook* g_prof = nullptr; }
using namespace knz;

static constexpr u32 T = prims::RS_TILE, G = prims::RS_GROUP, S = prims::SC_TILE;

template <class KEY>
static void make_keys(std::mt19937_64& rng, std::vector<KEY>& k, std::vector<u32>& v, size_t n, int keyKind)
{
    for (size_t i = 0; i < n; i++) {
        const u64 r = rng();
        k[i] = (KEY)(keyKind == 0 ? r : keyKind == 1 ? (r & 0x0303030303030303ull) : keyKind == 2 ? 0 : (r | 0xFFFF000000000000ull));
        v[i] = (u32)i;
    }
}

// every segment of (ko, vo) = the stable sort of its segment of k0 on bits [loBit, hiBit); values started as the global index
template <class KEY, bool HAS_VAL>
static int compare_sorted(const std::vector<KEY>& k0, const KEY* ko, const u32* vo, const std::vector<u32>& segLens, const std::vector<u32>& base, int loBit, int hiBit)
{
    const int nb = hiBit - loBit;
    const KEY mask = (nb >= (int)(8 * sizeof(KEY))) ? (KEY)~(KEY)0 : (KEY)((((KEY)1) << nb) - 1);
    int bad = 0;
    for (size_t sgm = 0; sgm < segLens.size(); sgm++) {
        std::vector<u32> idx(segLens[sgm]);
        std::iota(idx.begin(), idx.end(), base[sgm]);
        std::stable_sort(idx.begin(), idx.end(), [&](u32 a, u32 b) { return ((k0[a] >> loBit) & mask) < ((k0[b] >> loBit) & mask); });
        for (u32 i = 0; i < segLens[sgm]; i++) {
            if (ko[base[sgm] + i] != k0[idx[i]] || (HAS_VAL && vo[base[sgm] + i] != idx[i])) { bad++; break; }
        }
    }
    return bad;
}

struct SortWs {
    std::vector<u32> base;
    std::vector<u8> mem;
    prims::RsWs rs;
    size_t n, maxSeg;
    explicit SortWs(const std::vector<u32>& segLens)
    {
        const int nSeg = (int)segLens.size();
        base.assign(nSeg + 1, 0);
        for (int i = 0; i < nSeg; i++) base[i + 1] = base[i] + segLens[i];
        n = base[nSeg];
        mem.resize(prims::rs_ws_bytes(n + 1, nSeg) + 256);
        u8* p = reinterpret_cast<u8*>((reinterpret_cast<uintptr_t>(mem.data()) + 255) & ~(uintptr_t)255);
        rs = prims::rs_carve(p, n + 1, nSeg, base.data(), nSeg);
        prims::rs_launch_layout(nullptr, rs);
        maxSeg = 1;
        for (u32 l : segLens) maxSeg = std::max<size_t>(maxSeg, l);
    }
};

template <class KEY, bool HAS_VAL>
static int check_sort(std::mt19937_64& rng, const std::vector<u32>& segLens, int loBit, int hiBit, int keyKind, bool oneRead = true)
{
    SortWs w(segLens);
    const size_t n = w.n;
    std::vector<KEY> ka(n + 1), kb(n + 1);
    std::vector<u32> va(n + 1), vb(n + 1);
    make_keys(rng, ka, va, n, keyKind);
    std::vector<KEY> k0 = ka;
    const int r = prims::rs_sort<KEY, HAS_VAL>(nullptr, w.rs, ka.data(), kb.data(), va.data(), vb.data(), w.maxSeg, loBit, hiBit, oneRead);
    const int bad = compare_sorted<KEY, HAS_VAL>(k0, r ? kb.data() : ka.data(), r ? vb.data() : va.data(), segLens, w.base, loBit, hiBit);
    if (bad) printf("FAIL sort: key bytes %d val %d segs %d n %zu bits [%d,%d) kind %d one-read %d\n", (int)sizeof(KEY), (int)HAS_VAL, (int)segLens.size(), n, loBit, hiBit, keyKind, (int)oneRead);
    return bad;
}

// rs_sort_keep (the LZ candidate sort): the same result in one of the two spare pairs, and the input as it was
template <class KEY, bool HAS_VAL>
static int check_sort_keep(std::mt19937_64& rng, const std::vector<u32>& segLens, int loBit, int hiBit, int keyKind, bool oneRead = true)
{
    SortWs w(segLens);
    const size_t n = w.n;
    std::vector<KEY> kin(n + 1), kb(n + 1), kc(n + 1);
    std::vector<u32> vin(n + 1), vb(n + 1), vc(n + 1);
    make_keys(rng, kin, vin, n, keyKind);
    const std::vector<KEY> k0 = kin;
    const std::vector<u32> v0 = vin;
    const int r = prims::rs_sort_keep<KEY, HAS_VAL>(nullptr, w.rs, kin.data(), vin.data(), kb.data(), kc.data(), vb.data(), vc.data(), w.maxSeg, loBit, hiBit, oneRead);
    int bad = compare_sorted<KEY, HAS_VAL>(k0, r ? kc.data() : kb.data(), r ? vc.data() : vb.data(), segLens, w.base, loBit, hiBit);
    if (kin != k0 || vin != v0) bad++;
    if (bad) printf("FAIL sort (keep): key bytes %d val %d segs %d n %zu bits [%d,%d) kind %d one-read %d\n", (int)sizeof(KEY), (int)HAS_VAL, (int)segLens.size(), n, loBit, hiBit, keyKind, (int)oneRead);
    return bad;
}

// dev: the size comes from device memory (nMax = n + 7); inPlace: in == out
template <int OP>
static int check_scan(std::mt19937_64& rng, size_t n, bool dev, bool inPlace = false)
{
    std::vector<u32> in(n + 16), out(n + 16, 0xDEADBEEF), tmp(prims::scan_tmp_bytes(n + 16) / 4 + 64);
    for (size_t i = 0; i < n; i++) in[i] = (u32)rng();                   // full 32 bits: the sum wraps, max / min see bit 31
    for (size_t i = n; i < n + 16; i++) in[i] = 0xDEADBEEF;
    const std::vector<u32> in0 = in;
    u32* o = inPlace ? in.data() : out.data();
    u32 nDev = (u32)n, total = 0x12345678u;
    prims::launch_scan<OP>(nullptr, in.data(), o, dev ? n + 7 : n, dev ? &nDev : nullptr, tmp.data(), OP == prims::SCAN_SUM_EXCL ? &total : nullptr);
    u32 run = OP == prims::SCAN_MIN_INCL ? 0xFFFFFFFFu : 0u;
    for (size_t i = 0; i < n; i++) {
        u32 want;
        if (OP == prims::SCAN_SUM_EXCL) { want = run; run += in0[i]; }
        else if (OP == prims::SCAN_MAX_INCL) { run = std::max(run, in0[i]); want = run; }
        else { run = std::min(run, in0[i]); want = run; }
        if (o[i] != want) { printf("FAIL scan op %d n %zu in place %d at %zu: %u vs %u\n", OP, n, (int)inPlace, i, o[i], want); return 1; }
    }
    for (size_t i = n; i < n + 16; i++) if (o[i] != 0xDEADBEEF) { printf("FAIL scan op %d n %zu: wrote behind the end\n", OP, n); return 1; }
    if (OP == prims::SCAN_SUM_EXCL && total != run) { printf("FAIL scan total n %zu\n", n); return 1; }
    return 0;
}

// *nDev == 0 under nMax > 0: nothing is written but the total, which is 0
template <int OP>
static int check_scan_empty(size_t nMax)
{
    std::vector<u32> in(nMax + 16, 7u), out(nMax + 16, 0xDEADBEEF), tmp(prims::scan_tmp_bytes(nMax + 16) / 4 + 64);
    u32 nDev = 0, total = 0x12345678u;
    prims::launch_scan<OP>(nullptr, in.data(), out.data(), nMax, &nDev, tmp.data(), OP == prims::SCAN_SUM_EXCL ? &total : nullptr);
    for (u32 x : out) if (x != 0xDEADBEEF) { printf("FAIL empty scan op %d nMax %zu: wrote to out\n", OP, nMax); return 1; }
    if (OP == prims::SCAN_SUM_EXCL && total != 0) { printf("FAIL empty scan nMax %zu: total %u\n", nMax, total); return 1; }
    return 0;
}

int main(int argc, char** argv)
{
    std::mt19937_64 rng(12345);
    int bad = 0;
    const bool quick = argc > 1 && argv[1][0] == 'q';        // a short form for the runs under other switches (the sorts only)
    // one key, one tile and its neighbours, ragged segments with an empty one, three tiles, nine tiles (still one group of the column
    // scan: the segments of several groups follow below), two segments that end on and just behind a tile border
    const std::vector<u32> ragged = { 100, 0, T / 2 + T / 8, T / 2, 1 };
    const std::vector<std::vector<u32>> layouts = quick ? std::vector<std::vector<u32>>{ ragged, {2 * T + T / 2} }
        : std::vector<std::vector<u32>>{ {1}, {T - 1}, {T}, {T + 1}, ragged, {2 * T + T / 2}, {8 * T + T / 2}, {4 * T, 4 * T + 1} };
    for (const auto& lay : layouts) {
        for (int kind = 0; kind < (quick ? 2 : 4); kind++) {
            bad += check_sort<u64, false>(rng, lay, 0, 64, kind);
            bad += check_sort<u64, true>(rng, lay, 3, 45, kind);
            bad += check_sort<u32, true>(rng, lay, 0, 21, kind);
            bad += check_sort<u32, false>(rng, lay, 8, 32, kind);
            bad += check_sort_keep<u32, true>(rng, lay, 0, 21, kind);
        }
    }
    // More than RS_GROUP tiles in a segment: the second level of the column scan (k_rs_colscan1 over several groups, k_rs_colscan2, the
    // group carry in k_rs_scatter, grpOff behind a segment of one group and in front of a short one) and look-back over a group border.
    // A reduced matrix, the emulator being slow: u32 keys without values, one pass, the one-read pass and count + scatter.
    for (const auto& lay : std::vector<std::vector<u32>>{ {G * T + 1}, {T + 1, G * T + 1, 3} })
        for (int oneRead = 0; oneRead < 2; oneRead++) bad += check_sort<u32, false>(rng, lay, 8, 16, 0, oneRead != 0);
    if (!quick) {
        for (size_t n : { (size_t)1, (size_t)15, (size_t)16, (size_t)S - 1, (size_t)S, (size_t)S + 1, (size_t)100000, (size_t)300000 })
            for (int dev = 0; dev < 2; dev++) {
                bad += check_scan<prims::SCAN_SUM_EXCL>(rng, n, dev != 0);
                bad += check_scan<prims::SCAN_MAX_INCL>(rng, n, dev != 0);
                bad += check_scan<prims::SCAN_MIN_INCL>(rng, n, dev != 0);
            }
        for (size_t n : { (size_t)17, (size_t)S + 1, (size_t)3 * S + 5 })
            for (int dev = 0; dev < 2; dev++) {
                bad += check_scan<prims::SCAN_SUM_EXCL>(rng, n, dev != 0, true);
                bad += check_scan<prims::SCAN_MAX_INCL>(rng, n, dev != 0, true);
                bad += check_scan<prims::SCAN_MIN_INCL>(rng, n, dev != 0, true);
            }
        for (size_t nMax : { (size_t)1, (size_t)3 * S + 5 }) {
            bad += check_scan_empty<prims::SCAN_SUM_EXCL>(nMax);
            bad += check_scan_empty<prims::SCAN_MAX_INCL>(nMax);
            bad += check_scan_empty<prims::SCAN_MIN_INCL>(nMax);
        }
    }
    printf(bad ? "FAILED %d\n" : "OK\n", bad);
    return bad ? 1 : 0;
}
