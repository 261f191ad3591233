// CPU-only check of the batched copy kernel (kanzi-cpp_amd/csrc/copy_many.hip compiled as plain C++ against tools/hipemu, with a small
// tile: -DKNZ_EMU_COPY_TILE). Every (src mod 16, dst mod 16) pair with lengths around 0, 16 and the tile size; launches of 1, 63, 64, 65
// and 1,000 copies with empty copies first, in the middle and last. Every source is an allocation of its own that ends with the source's
// last byte (built with AddressSanitizer, a load behind it is a report); every destination has its pad bytes and 32 guard bytes on both
// sides compared afterwards. Test infrastructure only.
//   usage: copy_many_emu            prints OK <copies checked> cases
#include "hip/hip_runtime.h"
#include "../../kanzi-cpp_amd/csrc/copy_many.hip"

#include <stdio.h>
#include <stdlib.h>
#include <vector>

namespace knz { thread_local ProfHook* g_prof = nullptr; }
using namespace knz;

static int g_bad = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (g_bad < 20) { printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } g_bad++; } } while (0)

constexpr u32 GUARD = 32;
struct Case { u32 smod, dmod, len; };
struct Live { Case c; u8* srcBuf; u8* dstBuf; u8* src; u8* dst; size_t dstBytes; };

static u8 guard_byte(size_t i, u32 salt) { return (u8)(0xA5 ^ (i * 131) ^ salt); }
static u8 data_byte(size_t i, u32 salt) { return (u8)((i * 29 + salt * 7 + (i >> 8)) ^ 0x3C); }

static Live make(const Case& c, u32 salt)
{
    Live l; l.c = c;
    l.srcBuf = (u8*)malloc((size_t)c.smod + c.len + (c.smod + c.len == 0));       // (malloc returns 16-byte aligned memory)
    l.src = l.srcBuf + c.smod;
    for (u32 i = 0; i < c.len; i++) l.src[i] = data_byte(i, salt);
    l.dstBytes = (size_t)GUARD + c.dmod + c.len + GUARD;
    l.dstBuf = (u8*)malloc(l.dstBytes);
    l.dst = l.dstBuf + GUARD + c.dmod;
    for (size_t i = 0; i < l.dstBytes; i++) l.dstBuf[i] = guard_byte(i, salt);
    return l;
}

static void check(const Live& l, u32 salt, int launch)
{
    const size_t lo = (size_t)(l.dst - l.dstBuf), hi = lo + l.c.len;
    size_t wrong = 0, spilled = 0;
    for (size_t i = 0; i < l.dstBytes; i++) {
        if (i >= lo && i < hi) wrong += l.dstBuf[i] != data_byte(i - lo, salt);
        else spilled += l.dstBuf[i] != guard_byte(i, salt);
    }
    CHECK(wrong == 0 && spilled == 0, "launch %d, src mod %u, dst mod %u, len %u: %zu bytes wrong, %zu bytes outside the destination changed", launch, l.c.smod, l.c.dmod, l.c.len, wrong, spilled);
}

int main()
{
    const u32 T = CM_TILE;
    const u32 lens[] = { 0, 1, 15, 16, 17, 31, 33, T - 1, T, T + 1, 2 * T + 5 };
    std::vector<Case> matrix;
    for (u32 s = 0; s < 16; s++) for (u32 d = 0; d < 16; d++) for (u32 len : lens) matrix.push_back({ s, d, len });
    const int sizes[] = { 1, 63, 64, 65, 1000 };
    size_t next = 0;
    int launch = 0, checked = 0;
    while (next < matrix.size()) {
        const int k = sizes[launch % 5];
        std::vector<Live> live;
        for (int i = 0; i < k; i++) {
            const bool empty = k >= 3 && (i == 0 || i == k / 2 || i == k - 1);
            Case c = matrix[next % matrix.size()];
            if (empty) c.len = 0; else next++;
            live.push_back(make(c, (u32)(launch * 1000 + i)));
        }
        std::vector<knz_copy> copies((size_t)k);
        std::vector<u32> first((size_t)k + 1);
        u64 at = 0;
        for (int i = 0; i < k; i++) {
            copies[i].src = (u64)(uintptr_t)live[i].src; copies[i].dst = (u64)(uintptr_t)live[i].dst; copies[i].len = live[i].c.len;
            first[i] = (u32)at;
            const u64 tiles = copy_many_tiles(copies[i].dst, copies[i].len);
            CHECK(tiles == (live[i].c.len ? (live[i].c.dmod + live[i].c.len + T - 1) / T : 0u), "tiles of dst mod %u, len %u", live[i].c.dmod, live[i].c.len);
            at += tiles;
        }
        first[k] = (u32)at;
        launch_copy_many(nullptr, copies.data(), first.data(), (u32)k, (u32)at);
        for (int i = 0; i < k; i++) { check(live[i], (u32)(launch * 1000 + i), launch); free(live[i].srcBuf); free(live[i].dstBuf); checked++; }
        launch++;
    }
    CHECK(copy_many_tile_bytes() == T, "tile size");
    printf(g_bad ? "FAILED %d of %d cases\n" : "OK %d cases\n", g_bad ? g_bad : checked, checked);
    return g_bad ? 1 : 0;
}
