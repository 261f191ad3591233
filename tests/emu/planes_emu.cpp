// CPU-only check of the byte-plane kernels (kanzi-cpp_amd/csrc/planes.hip compiled as plain C++ against tools/hipemu, with a small tile:
// -DKNZ_EMU_PLANES_TILE). Both directions; elements of 1, 2, 4 and 8 bytes; every (src mod 16, dst mod 16) pair with element counts 0, 1,
// 15, 16, 17, tile / width - 1, tile / width, tile / width + 1 and 2 tiles + 5; launches of 1, 63, 64, 65 and 1,000 entries with empty
// entries first, in the middle and last, the widths mixed in every launch. Every source is an allocation of its own that ends with the
// source's last byte (built with AddressSanitizer, a load behind it is a report); every destination has 32 guard bytes on both sides
// compared afterwards. What has to come out is computed by a scalar loop here. Test infrastructure only.
//   usage: planes_emu [step]        every step-th alignment pair (default 1: all of them); prints OK <entries checked> cases
#include "hip/hip_runtime.h"
#include "../../kanzi-cpp_amd/csrc/planes.hip"

#include <stdio.h>
#include <stdlib.h>
#include <vector>

namespace knz { thread_local ProfHook* g_prof = nullptr; }
using namespace knz;

static int g_bad = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (g_bad < 20) { printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } g_bad++; } } while (0)

constexpr u32 GUARD = 32;
struct Case { u32 smod, dmod, elem, m; };
struct Live { Case c; u8* srcBuf; u8* dstBuf; u8* src; u8* dst; size_t dstBytes; };

static u8 guard_byte(size_t i, u32 salt) { return (u8)(0xA5 ^ (i * 131) ^ salt); }
static u8 data_byte(size_t i, u32 salt) { return (u8)((i * 29 + salt * 7 + (i >> 8)) ^ 0x3C); }

static Live make(const Case& c, u32 salt)
{
    Live l; l.c = c;
    const u32 len = c.elem * c.m;
    l.srcBuf = (u8*)malloc((size_t)c.smod + len + (c.smod + len == 0));            // (malloc returns 16-byte aligned memory)
    l.src = l.srcBuf + c.smod;
    for (u32 i = 0; i < len; i++) l.src[i] = data_byte(i, salt);
    l.dstBytes = (size_t)GUARD + c.dmod + len + GUARD;
    l.dstBuf = (u8*)malloc(l.dstBytes);
    l.dst = l.dstBuf + GUARD + c.dmod;
    for (size_t i = 0; i < l.dstBytes; i++) l.dstBuf[i] = guard_byte(i, salt);
    return l;
}

static void check(const Live& l, u32 salt, int launch, bool split)
{
    const u32 w = l.c.elem, m = l.c.m, len = w * m;
    std::vector<u8> want(len);
    for (u32 i = 0; i < m; i++)
        for (u32 k = 0; k < w; k++) {
            if (split) want[(size_t)k * m + i] = l.src[(size_t)i * w + k];
            else want[(size_t)i * w + k] = l.src[(size_t)k * m + i];
        }
    const size_t lo = (size_t)(l.dst - l.dstBuf), hi = lo + len;
    size_t wrong = 0, spilled = 0;
    for (size_t i = 0; i < l.dstBytes; i++) {
        if (i >= lo && i < hi) wrong += l.dstBuf[i] != want[i - lo];
        else spilled += l.dstBuf[i] != guard_byte(i, salt);
    }
    CHECK(wrong == 0 && spilled == 0, "%s, launch %d, src mod %u, dst mod %u, %u elements of %u bytes: %zu bytes wrong, %zu bytes outside the destination changed",
          split ? "split" : "join", launch, l.c.smod, l.c.dmod, m, w, wrong, spilled);
}

int main(int argc, char** argv)
{
    const u32 T = PL_TILE, step = argc > 1 ? (u32)atoi(argv[1]) : 1;
    const u32 widths[] = { 1, 2, 4, 8 };
    std::vector<Case> matrix;
    for (u32 pair = 0; pair < 256; pair += step)
        for (u32 sel = 0; sel < 9; sel++)
            for (u32 w : widths) {                                   // (the widths go round fastest: every launch mixes them)
                const u32 counts[] = { 0, 1, 15, 16, 17, T / w - 1, T / w, T / w + 1, 2 * (T / w) + 5 };
                matrix.push_back({ pair >> 4, pair & 15, w, counts[sel] });
            }
    const int sizes[] = { 1, 63, 64, 65, 1000 };
    int launch = 0, checked = 0;
    for (int dir = 0; dir < 2; dir++) {
        const bool split = dir == 0;
        size_t next = 0;
        while (next < matrix.size()) {
            const int k = sizes[launch % 5];
            std::vector<Live> live;
            for (int i = 0; i < k; i++) {
                const bool empty = k >= 3 && (i == 0 || i == k / 2 || i == k - 1);
                Case c = matrix[next % matrix.size()];
                if (empty) c.m = 0; else next++;
                live.push_back(make(c, (u32)(launch * 1000 + i)));
            }
            std::vector<knz_plane_copy> entries((size_t)k);
            std::vector<u32> first((size_t)k + 1);
            u64 at = 0;
            for (int i = 0; i < k; i++) {
                const Case& c = live[i].c;
                entries[i].src = (u64)(uintptr_t)live[i].src; entries[i].dst = (u64)(uintptr_t)live[i].dst;
                entries[i].len = (u64)c.elem * c.m; entries[i].elem = c.elem; entries[i].reserved = 0;
                first[i] = (u32)at;
                const u64 tiles = planes_tiles(entries[i].len);
                CHECK(tiles == ((u64)c.elem * c.m + T - 1) / T, "tiles of %u elements of %u bytes", c.m, c.elem);
                at += tiles;
            }
            first[k] = (u32)at;
            (split ? launch_split_many : launch_join_many)(nullptr, entries.data(), first.data(), (u32)k, (u32)at);
            for (int i = 0; i < k; i++) { check(live[i], (u32)(launch * 1000 + i), launch, split); free(live[i].srcBuf); free(live[i].dstBuf); checked++; }
            launch++;
        }
    }
    CHECK(planes_tile_bytes() == T, "tile size");
    printf(g_bad ? "FAILED %d of %d cases\n" : "OK %d cases\n", g_bad ? g_bad : checked, checked);
    return g_bad ? 1 : 0;
}
