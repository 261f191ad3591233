// TEST INFRASTRUCTURE ONLY -- a small CPU emulation of the HIP constructs the kernels in kanzi-cpp_amd/csrc use,
// so that kernel logic (index arithmetic, wave-level ranking, LDS protocols) can be exercised in the CPU-only test
// suite, where no GPU exists. A kernel's threads run as cooperative fibers on one OS thread: a workgroup is run to
// completion before the next one starts, __syncthreads() and the wave intrinsics (64 lanes) are rendezvous points.
// Nothing here is part of the product; the product path has no CPU fallback (the GPU build never sees this file:
// it is only on the include path of tests/emu/*.cpp, ahead of /opt/rocm/include).
#pragma once
#define KNZ_EMU 1
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <functional>
#include <vector>

#define __global__
#define __device__
#define __host__
#define __forceinline__ inline
#define __noinline__
#define __launch_bounds__(...)
#define __shared__ static

struct dim3 {
    unsigned x, y, z;
    dim3(unsigned a = 1, unsigned b = 1, unsigned c = 1) : x(a), y(b), z(c) {}
};
struct uint2 { unsigned x, y; };
static inline uint2 make_uint2(unsigned a, unsigned b) { uint2 r; r.x = a; r.y = b; return r; }
struct uint4 { unsigned x, y, z, w; };
static inline uint4 make_uint4(unsigned a, unsigned b, unsigned c, unsigned d) { uint4 r; r.x = a; r.y = b; r.z = c; r.w = d; return r; }

typedef void* hipStream_t;
typedef int hipError_t;
enum { hipSuccess = 0 };
enum hipMemcpyKind { hipMemcpyHostToDevice, hipMemcpyDeviceToHost, hipMemcpyDeviceToDevice };
static inline hipError_t hipMemsetAsync(void* p, int v, size_t n, hipStream_t) { memset(p, v, n); return hipSuccess; }
static inline hipError_t hipMemcpyAsync(void* d, const void* s, size_t n, hipMemcpyKind, hipStream_t) { memcpy(d, s, n); return hipSuccess; }
static inline hipError_t hipStreamSynchronize(hipStream_t) { return hipSuccess; }
static inline hipError_t hipGetLastError() { return hipSuccess; }
static inline const char* hipGetErrorString(hipError_t) { return "emu"; }

namespace hipemu {

struct Fiber {
    void* sp;
    char* stack;
    dim3 tid;
    int state;          // 0 runnable, 1 waiting at block barrier, 2 waiting at wave rendezvous, 3 done
    unsigned long long xval;
};

struct Block {
    dim3 bIdx, bDim, gDim;
    std::vector<Fiber> fibers;
    std::function<void()> body;
    void* schedSp;
    Fiber* cur;
    int nLive;
};

Block& blk();
void yield_to_scheduler();
void launch(const std::function<void()>& body, dim3 grid, dim3 block);
void block_barrier();
// rendezvous of the (live) lanes of the calling fiber's wave: every lane deposits v, gets the array of all 64
void wave_exchange(unsigned long long v, unsigned long long out[64], unsigned long long* activeMask);
// the same rendezvous for a wave that polls memory written by another wave of its block: the other waves run before it returns
void wave_spin();
// a rendezvous of the named lanes only (wave intrinsics inside divergent control flow)
void wave_exchange_subset(unsigned long long v, unsigned long long out[64], unsigned long long lanes);

}  // namespace hipemu

#define threadIdx (hipemu::blk().cur->tid)
#define blockIdx (hipemu::blk().bIdx)
#define blockDim (hipemu::blk().bDim)
#define gridDim (hipemu::blk().gDim)

namespace hipemu {
template <class F, class... A>
static inline void launch_k(F f, dim3 grid, dim3 block, size_t, hipStream_t, A... args) { launch([=]() { f(args...); }, grid, block); }
}
#define hipLaunchKernelGGL(kernel, ...) hipemu::launch_k(kernel, __VA_ARGS__)

static inline void __syncthreads() { hipemu::block_barrier(); }

static inline unsigned long long __ballot(int pred)
{
    unsigned long long v[64], act;
    hipemu::wave_exchange(pred ? 1ull : 0ull, v, &act);
    unsigned long long m = 0;
    for (int i = 0; i < 64; i++) if (((act >> i) & 1) && v[i]) m |= 1ull << i;
    return m;
}
// ballot among the lanes of `lanes` (every one of them calls it, nobody else does)
static inline unsigned long long hipemu_ballot_of(int pred, unsigned long long lanes)
{
    unsigned long long v[64];
    hipemu::wave_exchange_subset(pred ? 1ull : 0ull, v, lanes);
    unsigned long long m = 0;
    for (int i = 0; i < 64; i++) if (((lanes >> i) & 1) && v[i]) m |= 1ull << i;
    return m;
}
static inline int __shfl(int var, int src, int width = 64)
{
    unsigned long long v[64], act;
    hipemu::wave_exchange((unsigned long long)(unsigned)var, v, &act);
    const int lane = (int)(threadIdx.x & 63);
    const int s = (lane & ~(width - 1)) | (src & (width - 1));
    return (int)(unsigned)v[s];
}
static inline int __shfl_up(int var, unsigned delta, int width = 64)
{
    unsigned long long v[64], act;
    hipemu::wave_exchange((unsigned long long)(unsigned)var, v, &act);
    const int lane = (int)(threadIdx.x & 63);
    const int s = lane - (int)delta;
    return ((s >= (lane & ~(width - 1))) ? (int)(unsigned)v[s] : var);
}
static inline int __shfl_down(int var, unsigned delta, int width = 64)
{
    unsigned long long v[64], act;
    hipemu::wave_exchange((unsigned long long)(unsigned)var, v, &act);
    const int lane = (int)(threadIdx.x & 63);
    const int s = lane + (int)delta;
    return ((s < ((lane & ~(width - 1)) + width)) ? (int)(unsigned)v[s] : var);
}
static inline int __shfl_xor(int var, int mask, int width = 64)
{
    unsigned long long v[64], act;
    hipemu::wave_exchange((unsigned long long)(unsigned)var, v, &act);
    const int lane = (int)(threadIdx.x & 63);
    (void)width;
    return (int)(unsigned)v[lane ^ mask];
}
static inline int __builtin_amdgcn_readlane(int var, int src) { return __shfl(var, src & 63, 64); }
// DPP data movement, the controls the kernels use: 0x130 / 0x138 = wave_shl:1 / wave_shr:1, 0x134 / 0x13C = wave_rol:1 / wave_ror:1,
// 0x111-0x11F = row_shr:n (inside rows of 16 lanes), 0x142 / 0x143 = row_bcast:15 / row_bcast:31 (lane 15 of a row to the next row,
// lane 31 to rows 2 and 3), 0x00-0xFF = quad_perm. A lane without a source lane keeps `old` (0 with bound_ctrl); a lane whose row or
// bank (group of 4 lanes inside its row) is masked out keeps `old`.
static inline int __builtin_amdgcn_update_dpp(int old, int src, int ctrl, int rowMask, int bankMask, bool boundCtrl)
{
    unsigned long long v[64], act;
    hipemu::wave_exchange((unsigned long long)(unsigned)src, v, &act);
    const int lane = (int)(threadIdx.x & 63);
    const int row = lane >> 4, inRow = lane & 15;
    if (!((rowMask >> row) & 1) || !((bankMask >> (inRow >> 2)) & 1)) return old;
    const int none = boundCtrl ? 0 : old;
    if (ctrl == 0x138) return lane == 0 ? none : (int)(unsigned)v[lane - 1];
    if (ctrl == 0x130) return lane == 63 ? none : (int)(unsigned)v[lane + 1];
    if (ctrl == 0x134) return (int)(unsigned)v[(lane + 1) & 63];
    if (ctrl == 0x13C) return (int)(unsigned)v[(lane + 63) & 63];
    if (ctrl > 0x110 && ctrl < 0x120) { const int n = ctrl & 15; return inRow >= n ? (int)(unsigned)v[lane - n] : none; }
    if (ctrl == 0x142) return row >= 1 ? (int)(unsigned)v[16 * row - 1] : none;
    if (ctrl == 0x143) return row >= 2 ? (int)(unsigned)v[31] : none;
    if (ctrl >= 0 && ctrl < 0x100) return (int)(unsigned)v[(lane & ~3) + ((ctrl >> (2 * (lane & 3))) & 3)];     // quad_perm
    fprintf(stderr, "hipemu: DPP control 0x%x not emulated\n", ctrl);
    abort();
}
static inline int __builtin_amdgcn_readfirstlane(int var)
{
    unsigned long long v[64], act;
    hipemu::wave_exchange((unsigned long long)(unsigned)var, v, &act);
    return (int)(unsigned)v[__builtin_ctzll(act)];
}
static inline unsigned long long __lanemask_lt() { const int lane = (int)(threadIdx.x & 63); return lane ? (~0ull >> (64 - lane)) : 0ull; }
static inline int __popcll(unsigned long long x) { return __builtin_popcountll(x); }
static inline int __popc(unsigned x) { return __builtin_popcount(x); }
static inline unsigned __builtin_amdgcn_alignbit(unsigned hi, unsigned lo, unsigned sh) { return (unsigned)(((((unsigned long long)hi) << 32) | lo) >> (sh & 31)); }
// v_perm_b32: result byte i = byte sel[i] of the 8 bytes {b (0-3), a (4-7)} (the constant selectors 0x0C.. are not used by the kernels)
static inline unsigned __builtin_amdgcn_perm(unsigned a, unsigned b, unsigned sel)
{
    const unsigned long long v = ((unsigned long long)a << 32) | b;
    unsigned r = 0;
    for (int i = 0; i < 4; i++) {
        const unsigned s = (sel >> (8 * i)) & 0xFF;
        if (s > 7) { fprintf(stderr, "hipemu: v_perm selector 0x%x not emulated\n", s); abort(); }
        r |= (unsigned)((v >> (8 * s)) & 0xFF) << (8 * i);
    }
    return r;
}
static inline unsigned __umul24(unsigned a, unsigned b) { return (a & 0xFFFFFFu) * (b & 0xFFFFFFu); }
static inline unsigned __umulhi(unsigned a, unsigned b) { return (unsigned)(((unsigned long long)a * b) >> 32); }
static inline int __ffsll(long long x) { return __builtin_ffsll(x); }
static inline int __ffs(int x) { return __builtin_ffs(x); }
static inline int __clz(int x) { return x == 0 ? 32 : __builtin_clz((unsigned)x); }
static inline int __clzll(long long x) { return x == 0 ? 64 : __builtin_clzll((unsigned long long)x); }

template <class T> static inline T atomicAdd(T* p, T v) { const T o = *p; *p = o + v; return o; }
template <class T> static inline T atomicOr(T* p, T v) { const T o = *p; *p = o | v; return o; }
template <class T> static inline T atomicAnd(T* p, T v) { const T o = *p; *p = o & v; return o; }
// scoped atomic accesses: fibers run one at a time, so a plain access is atomic at every scope
#define __HIP_MEMORY_SCOPE_WORKGROUP 3
#define __HIP_MEMORY_SCOPE_AGENT 4
template <class T> static inline T __hip_atomic_load(const T* p, int, int) { return *p; }
template <class T> static inline void __hip_atomic_store(T* p, T v, int, int) { *p = v; }
static inline unsigned long long __ballot(int pred);
static inline void __threadfence_block() { (void)__ballot(1); }      // (issued by the kernels in workgroup-uniform control flow)
static inline void __threadfence() {}
// a wave-scope fence orders the memory operations of the wave's lanes: in the emulation, where lanes only meet at wave
// intrinsics, it has to be a rendezvous (the kernels issue it in wave-uniform control flow)
#define __builtin_amdgcn_fence(order, scope) ((void)__ballot(1))
template <class T> static inline T min(T a, T b) { return a < b ? a : b; }
template <class T> static inline T max(T a, T b) { return a > b ? a : b; }
template <class T> static inline T atomicMax(T* p, T v) { const T o = *p; if (v > o) *p = v; return o; }
template <class T> static inline T atomicMin(T* p, T v) { const T o = *p; if (v < o) *p = v; return o; }
