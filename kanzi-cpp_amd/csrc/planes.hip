// Byte planes of many device buffers in one launch (knz_hip_split_many / knz_hip_join_many): an entry of len bytes holds m = len / elem
// elements of elem bytes (1, 2, 4 or 8); split writes byte k of every element to plane k, dst[k * m + i] = src[i * elem + k], join is the
// way back, dst[i * elem + k] = src[k * m + i]. With elem = 1 both are a plain copy. What TensorCodec gathers its input with when the
// tensors are coded as planes: the payload is still moved once.
//
// The host cuts every entry into tiles of PL_TILE bytes of the interleaved side, PL_TILE / elem elements each, counted from the entry's
// first element (no boundary depends on an address); one workgroup moves one tile and finds its entry by a binary search in the exclusive
// prefix of the tile counts, as k_copy_many does. Inside a tile a lane takes a unit of 16 elements: elem consecutive 16-byte chunks of the
// interleaved side and 16 bytes of each of the elem planes, turned into each other in registers with v_perm_b32. The fewer than 16
// elements a tile has left behind its last unit (only an entry's last tile has any) go byte by byte.
//
// Every 16-byte access is an UNALIGNED vector access: plane k starts at k * m behind plane 0 and m is arbitrary, so no choice of unit
// boundaries aligns more than one plane, and aligning each plane by itself would read the interleaved side once per plane (DESIGN.md
// section 3.3). A unit's loads and stores cover exactly its 16 elements on both sides, so nothing outside [src, src + len) is read and
// nothing outside [dst, dst + len) is written, whatever the alignment is.
#include "common.hpp"
#include "stages.hpp"

namespace knz {

#ifdef KNZ_EMU_PLANES_TILE
constexpr u32 PL_TILE = KNZ_EMU_PLANES_TILE;      // (tests/emu: tile boundaries cheap to cross)
#else
constexpr u32 PL_TILE = 16384;
#endif
constexpr int PL_THREADS = 256;
constexpr u32 PL_UNIT = 16;                       // elements of a lane's unit
static_assert(PL_TILE % 8 == 0 && PL_TILE >= 8, "a tile holds whole elements of every width");

// four words from and to any address
__device__ __forceinline__ void pl_load(u64 p, u32* w)
{
    const u32x4 v = ldg_u<u32x4>(reinterpret_cast<const void*>((uintptr_t)p));
    w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
}
__device__ __forceinline__ void pl_store(u64 p, const u32* w)
{
    u32x4 v; v.x = w[0]; v.y = w[1]; v.z = w[2]; v.w = w[3];
    stg_u<u32x4>(reinterpret_cast<void*>((uintptr_t)p), v);
}
__device__ __forceinline__ void pl_byte(u64 dst, u64 src) { stg<u8>(reinterpret_cast<void*>((uintptr_t)dst), ldg<u8>(reinterpret_cast<const void*>((uintptr_t)src))); }

// the 4 x 4 byte transpose: byte j of r_i = byte i of w_j (its own inverse)
__device__ __forceinline__ void pl_tr4(u32 w0, u32 w1, u32 w2, u32 w3, u32& r0, u32& r1, u32& r2, u32& r3)
{
    const u32 lo01 = __builtin_amdgcn_perm(w1, w0, 0x05010400u), hi01 = __builtin_amdgcn_perm(w1, w0, 0x07030602u);
    const u32 lo23 = __builtin_amdgcn_perm(w3, w2, 0x05010400u), hi23 = __builtin_amdgcn_perm(w3, w2, 0x07030602u);
    r0 = __builtin_amdgcn_perm(lo23, lo01, 0x05040100u); r1 = __builtin_amdgcn_perm(lo23, lo01, 0x07060302u);
    r2 = __builtin_amdgcn_perm(hi23, hi01, 0x05040100u); r3 = __builtin_amdgcn_perm(hi23, hi01, 0x07060302u);
}

// w: the 16 elements of a unit as they lie interleaved (4 * ELEM words); p: their planes, plane k in p[4 * k .. 4 * k + 3]
template <int ELEM>
__device__ __forceinline__ void pl_to_planes(const u32* w, u32* p)
{
    if (ELEM == 1) { for (int q = 0; q < 4; q++) p[q] = w[q]; }
    if (ELEM == 2) {
        for (int q = 0; q < 4; q++) {
            p[q] = __builtin_amdgcn_perm(w[2 * q + 1], w[2 * q], 0x06040200u);
            p[4 + q] = __builtin_amdgcn_perm(w[2 * q + 1], w[2 * q], 0x07050301u);
        }
    }
    if (ELEM == 4) { for (int q = 0; q < 4; q++) pl_tr4(w[4 * q], w[4 * q + 1], w[4 * q + 2], w[4 * q + 3], p[q], p[4 + q], p[8 + q], p[12 + q]); }
    if (ELEM == 8) {
        for (int q = 0; q < 4; q++) {
            pl_tr4(w[8 * q], w[8 * q + 2], w[8 * q + 4], w[8 * q + 6], p[q], p[4 + q], p[8 + q], p[12 + q]);
            pl_tr4(w[8 * q + 1], w[8 * q + 3], w[8 * q + 5], w[8 * q + 7], p[16 + q], p[20 + q], p[24 + q], p[28 + q]);
        }
    }
}

template <int ELEM>
__device__ __forceinline__ void pl_from_planes(const u32* p, u32* w)
{
    if (ELEM == 1) { for (int q = 0; q < 4; q++) w[q] = p[q]; }
    if (ELEM == 2) {
        for (int q = 0; q < 4; q++) {
            w[2 * q] = __builtin_amdgcn_perm(p[4 + q], p[q], 0x05010400u);
            w[2 * q + 1] = __builtin_amdgcn_perm(p[4 + q], p[q], 0x07030602u);
        }
    }
    if (ELEM == 4) { for (int q = 0; q < 4; q++) pl_tr4(p[q], p[4 + q], p[8 + q], p[12 + q], w[4 * q], w[4 * q + 1], w[4 * q + 2], w[4 * q + 3]); }
    if (ELEM == 8) {
        for (int q = 0; q < 4; q++) {
            pl_tr4(p[q], p[4 + q], p[8 + q], p[12 + q], w[8 * q], w[8 * q + 2], w[8 * q + 4], w[8 * q + 6]);
            pl_tr4(p[16 + q], p[20 + q], p[24 + q], p[28 + q], w[8 * q + 1], w[8 * q + 3], w[8 * q + 5], w[8 * q + 7]);
        }
    }
}

// B units, PL_THREADS units apart: all their loads, then all their stores. inter: the first unit's first element on the interleaved
// side, plane: its byte in plane 0; the planes are m bytes apart.
template <int ELEM, bool SPLIT, int B>
__device__ __forceinline__ void pl_units(u64 inter, u64 plane, u64 m)
{
    constexpr u64 stepI = (u64)PL_THREADS * PL_UNIT * ELEM, stepP = (u64)PL_THREADS * PL_UNIT;
    u32 w[B][4 * ELEM], p[B][4 * ELEM];
#pragma unroll
    for (int b = 0; b < B; b++) {
#pragma unroll
        for (int j = 0; j < ELEM; j++) {
            if (SPLIT) pl_load(inter + b * stepI + 16u * j, &w[b][4 * j]);
            else pl_load(plane + b * stepP + j * m, &p[b][4 * j]);
        }
    }
#pragma unroll
    for (int b = 0; b < B; b++) {
        if (SPLIT) pl_to_planes<ELEM>(w[b], p[b]); else pl_from_planes<ELEM>(p[b], w[b]);
#pragma unroll
        for (int j = 0; j < ELEM; j++) {
            if (SPLIT) pl_store(plane + b * stepP + j * m, &p[b][4 * j]);
            else pl_store(inter + b * stepI + 16u * j, &w[b][4 * j]);
        }
    }
}

// the elements [e0, e0 + cnt) of an entry of m elements
template <int ELEM, bool SPLIT>
__device__ __forceinline__ void pl_tile(u64 src, u64 dst, u64 m, u64 e0, u32 cnt)
{
    constexpr int B = ELEM >= 4 ? 1 : 4 / ELEM;            // 64 bytes in flight per lane, as k_copy_many has
    const u64 inter = (SPLIT ? src : dst) + e0 * ELEM, plane = (SPLIT ? dst : src) + e0;
    const u32 units = cnt / PL_UNIT, tid = threadIdx.x;
    u32 u = tid;
    if (B > 1) for (; u + (B - 1) * PL_THREADS < units; u += B * PL_THREADS) pl_units<ELEM, SPLIT, B>(inter + (u64)u * PL_UNIT * ELEM, plane + (u64)u * PL_UNIT, m);
    for (; u < units; u += PL_THREADS) pl_units<ELEM, SPLIT, 1>(inter + (u64)u * PL_UNIT * ELEM, plane + (u64)u * PL_UNIT, m);
    // fewer than 16 elements are left: one byte per lane
    const u32 body = units * PL_UNIT, rest = (cnt - body) * ELEM;
    for (u32 j = tid; j < rest; j += PL_THREADS) {
        const u32 e = body + j / ELEM, k = j % ELEM;
        const u64 pi = inter + (u64)e * ELEM + k, pp = plane + k * m + e;
        if (SPLIT) pl_byte(pp, pi); else pl_byte(pi, pp);
    }
}

u64 planes_tiles(u64 len) { return (len + PL_TILE - 1) / PL_TILE; }
u32 planes_tile_bytes() { return PL_TILE; }

// tileFirst: n + 1 words, tileFirst[i] = tiles of the entries before i. One workgroup of PL_THREADS threads per tile.
template <bool SPLIT>
__device__ __forceinline__ void pl_many(const knz_plane_copy* __restrict__ entries, const u32* __restrict__ tileFirst, u32 n)
{
    const u32 t = blockIdx.x;
    // the entry i with tileFirst[i] <= t < tileFirst[i + 1] (an empty entry has no tile and is never found)
    u32 lo = 0, hi = n;
    while (hi - lo > 1) {
        const u32 mid = (lo + hi) >> 1;
        if (tileFirst[mid] <= t) lo = mid; else hi = mid;
    }
    const knz_plane_copy c = entries[lo];
    const u32 sh = c.elem == 8 ? 3 : c.elem == 4 ? 2 : c.elem == 2 ? 1 : 0, tileElems = PL_TILE >> sh;
    const u64 m = c.len >> sh, e0 = (u64)(t - tileFirst[lo]) * tileElems;
    const u32 cnt = m - e0 < tileElems ? (u32)(m - e0) : tileElems;
    switch (sh) {                                            // (uniform over the workgroup)
    case 0: pl_tile<1, SPLIT>(c.src, c.dst, m, e0, cnt); break;
    case 1: pl_tile<2, SPLIT>(c.src, c.dst, m, e0, cnt); break;
    case 2: pl_tile<4, SPLIT>(c.src, c.dst, m, e0, cnt); break;
    default: pl_tile<8, SPLIT>(c.src, c.dst, m, e0, cnt); break;
    }
}

__global__ __launch_bounds__(PL_THREADS) void k_split_many(const knz_plane_copy* __restrict__ entries, const u32* __restrict__ tileFirst, u32 n)
{
    pl_many<true>(entries, tileFirst, n);
}

__global__ __launch_bounds__(PL_THREADS) void k_join_many(const knz_plane_copy* __restrict__ entries, const u32* __restrict__ tileFirst, u32 n)
{
    pl_many<false>(entries, tileFirst, n);
}

void launch_split_many(hipStream_t s, const knz_plane_copy* entries, const u32* tileFirst, u32 n, u32 nTiles)
{
    if (nTiles == 0) return;
    { KScope ks_("k_split_many"); hipLaunchKernelGGL(k_split_many, dim3(nTiles), dim3(PL_THREADS), 0, s, entries, tileFirst, n); }
}

void launch_join_many(hipStream_t s, const knz_plane_copy* entries, const u32* tileFirst, u32 n, u32 nTiles)
{
    if (nTiles == 0) return;
    { KScope ks_("k_join_many"); hipLaunchKernelGGL(k_join_many, dim3(nTiles), dim3(PL_THREADS), 0, s, entries, tileFirst, n); }
}

}  // namespace knz
