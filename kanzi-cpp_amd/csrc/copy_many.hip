// Many independent device-to-device copies in one launch (knz_hip_copy_many): gathering scattered buffers into the packed, 16-aligned
// input of a many-streams call, compacting its 16-aligned output streams into one tight blob, and the way back.
//
// The host cuts every copy into tiles of CM_TILE destination bytes; tile boundaries are 16-byte boundaries of the DESTINATION (tile k of
// a copy covers the destination addresses [(dst & ~15) + k * CM_TILE, + CM_TILE), cut to [dst, dst + len)), so the stores of a tile's
// body are aligned 16-byte stores whatever the source's alignment is. One workgroup copies one tile; it finds its copy by a binary search
// in the exclusive prefix of the tile counts, which is uniform over the workgroup and runs on the scalar unit. A tile is three parts: the
// bytes up to the first 16-byte boundary of the destination (only a copy's first tile has any), the 16-byte body, the bytes behind the last
// boundary (only the last tile). Every load reads source bytes whose destination bytes the same lane writes: nothing outside
// [src, src + len) is read, nothing outside [dst, dst + len) is written.
//
// A full tile is 16 KiB: four 16-byte loads in flight per lane, then four stores, 1 KiB contiguous per wave instruction on both sides.
#include "common.hpp"
#include "stages.hpp"

namespace knz {

#ifdef KNZ_EMU_COPY_TILE
constexpr u32 CM_TILE = KNZ_EMU_COPY_TILE;        // (tests/emu: tile boundaries cheap to cross)
#else
constexpr u32 CM_TILE = 16384;
#endif
constexpr int CM_THREADS = 256;
constexpr u32 CM_PASS = 16 * CM_THREADS;          // body bytes the workgroup moves per load
static_assert(CM_TILE % 16 == 0 && CM_TILE >= 16, "tiles end at 16-byte boundaries");

// 16 bytes from any address (the source is aligned only when src = dst mod 16), 16 bytes to a 16-byte boundary
__device__ __forceinline__ u32x4 cm_load(u64 p) { return ldg_u<u32x4>(reinterpret_cast<const void*>((uintptr_t)p)); }
__device__ __forceinline__ void cm_store(u64 p, u32x4 v) { stg<u32x4>(reinterpret_cast<void*>((uintptr_t)p), v); }
__device__ __forceinline__ void cm_byte(u64 dst, u64 delta) { stg<u8>(reinterpret_cast<void*>((uintptr_t)dst), ldg<u8>(reinterpret_cast<const void*>((uintptr_t)(dst + delta)))); }

u64 copy_many_tiles(u64 dst, u64 len) { return len ? ((dst & 15) + len + CM_TILE - 1) / CM_TILE : 0; }
u32 copy_many_tile_bytes() { return CM_TILE; }

// tileFirst: n + 1 words, tileFirst[i] = tiles of the copies before i. One workgroup of CM_THREADS threads per tile.
__global__ __launch_bounds__(CM_THREADS) void k_copy_many(const knz_copy* __restrict__ copies, const u32* __restrict__ tileFirst, u32 n)
{
    const u32 t = blockIdx.x;
    // the copy i with tileFirst[i] <= t < tileFirst[i + 1] (an empty copy has no tile and is never found): 20 steps for the most copies a call takes
    u32 lo = 0, hi = n;
    while (hi - lo > 1) {
        const u32 mid = (lo + hi) >> 1;
        if (tileFirst[mid] <= t) lo = mid; else hi = mid;
    }
    const knz_copy c = copies[lo];
    const u64 tileLo = (c.dst & ~15ull) + (u64)(t - tileFirst[lo]) * CM_TILE, end = c.dst + c.len;
    const u64 a = c.dst > tileLo ? c.dst : tileLo, b = end < tileLo + CM_TILE ? end : tileLo + CM_TILE;      // the tile's destination bytes
    const u64 up = (a + 15) & ~15ull, bodyLo = up < b ? up : b;
    const u64 bodyHi = (b & ~15ull) > bodyLo ? (b & ~15ull) : bodyLo;
    const u64 delta = c.src - c.dst;
    const u32 tid = threadIdx.x;
    if (a + tid < bodyLo) cm_byte(a + tid, delta);                 // at most 15 bytes each
    if (bodyHi + tid < b) cm_byte(bodyHi + tid, delta);
    u64 p = bodyLo + 16u * tid;
    for (; p + 3 * CM_PASS < bodyHi; p += 4 * CM_PASS) {
        const u32x4 v0 = cm_load(p + delta), v1 = cm_load(p + CM_PASS + delta), v2 = cm_load(p + 2 * CM_PASS + delta), v3 = cm_load(p + 3 * CM_PASS + delta);
        cm_store(p, v0); cm_store(p + CM_PASS, v1); cm_store(p + 2 * CM_PASS, v2); cm_store(p + 3 * CM_PASS, v3);
    }
    for (; p < bodyHi; p += CM_PASS) cm_store(p, cm_load(p + delta));
}

void launch_copy_many(hipStream_t s, const knz_copy* copies, const u32* tileFirst, u32 n, u32 nTiles)
{
    if (nTiles == 0) return;
    { KScope ks_("k_copy_many"); hipLaunchKernelGGL(k_copy_many, dim3(nTiles), dim3(CM_THREADS), 0, s, copies, tileFirst, n); }
}

}  // namespace knz
