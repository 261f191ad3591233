// Bijective Burrows-Wheeler transform (BWTS, Scott's variant) on gfx950, forward and inverse, every block of a batch in the same launches.
//
// Reference being replaced: transform/BWTS.cpp (forward :29-138, inverse :180-247), BWTS.hpp (getMaxEncodedLength = n). No header,
// no primary index; blocks of fewer than 2 bytes are copied, a block longer than its destination is refused.
//
// Forward. Let T = w1 >= w2 >= ... >= wk be the Lyndon factorization of a block. Every rotation of every factor is sorted in omega-order
// (the order of the infinite repetitions rot^omega); output byte r is the byte in front of the rotation of rank r, cyclically inside its
// factor. Rotations tie only when they are the same rotation of two equal factors, and tied rotations have equal output bytes, so the
// output is unique: any correct construction is byte-identical to the reference's (which moves Lyndon word heads in a suffix array).
//   1. The suffix array of every block from the suffix sort of bwt_fwd.hip (bwt_suffix_arrays), scattered into ranks.
//   2. Position i starts a factor iff rank(i) < min(rank(0..i)): one global prefix-minimum scan over values made block-relative
//      (block b takes the range [total - base[b+1], total - base[b]), below every earlier block, so the global minimum in front of a
//      position of block b is the minimum inside block b), then a prefix sum gives factor ids and the factor start table.
//   3. Prefix doubling with group refinement on the rotations. A label is the slot where the rotation's group starts. Round 0 keys every
//      rotation by its first four bytes (wrapping inside its factor), round c (c = 4, 8, 16, ...) by (label, label of the rotation c
//      positions on inside its factor): that orders on the first 2c bytes. Only members of groups with more than one member take part:
//      their list (in slot order) is gathered into (label, key) pairs, sorted by the stable LSD radix sort of prims.hpp (one segment), and
//      the new groups are found by two max-scans. The sort stops when no group is left, or when the labels order the rotations on at
//      least 2M bytes, M the longest factor of the batch: by Fine and Wilf two different omega-words with periods <= M differ within
//      their first 2M - 1 bytes, so what is still grouped then is equal.
//   4. Emit: slot r of block b gets the byte cyclically in front of its rotation.
//
// Inverse. LF by a stable counting sort of the input (one 8-bit pass of the segmented radix sort: LF[i] = place of row i in the stable
// order of the bytes). The reference takes the cycles of LF in increasing order of their smallest row and writes each cycle backwards
// from the end of the block, starting with the smallest row. Data parallel:
//   1. pointer jumping along LF with a window that doubles every round: every row learns the smallest of the next W rows along LF
//      and how many steps on it lies; one 16-byte record per row (smallest row, steps, end of the window), one load per round. A round
//      that changes nothing means every cycle fits the window (see launch_bwts_inverse): the smallest row of the cycle and the distance
//      to it are then known, and the row behind the smallest one gives the cycle length;
//   2. an exclusive prefix sum of the cycle lengths, put at the smallest rows, gives every cycle's place (cycle lengths add up to the
//      block length, so the sum in front of block b is base[b]);
//   3. scatter: row i, k steps behind the smallest row h of its cycle, goes to n - 1 - (off[h] - base[b]) - k.
// n cycles of one row (all bytes equal) take one round; one cycle of n rows about log2(n).
#include "common.hpp"
#include "stages.hpp"
#include "bwt_common.hpp"

#include <algorithm>
#include "prims.hpp"

namespace knz {

namespace {

inline unsigned bwts_grid(size_t n)
{
    const size_t g = (n + 255) / 256;
    return (unsigned)std::max<size_t>(1, std::min<size_t>(g, 16384));
}

#define BWTS_FOR(i, n) for (u32 i = blockIdx.x * 256u + threadIdx.x; i < (n); i += gridDim.x * 256u)

// ---- forward ------------------------------------------------------------------------------------------------------------------------

// value of position p for the segmented prefix minimum: its suffix rank, made smaller than every value of the blocks before
__global__ __launch_bounds__(256) void k_bwts_rank_values(const u32* __restrict__ SA, const u32* __restrict__ base, int nBlocks, u32 total,
                                                          u32* __restrict__ val)
{
    BWTS_FOR(j, total) {
        const int b = find_block(base, nBlocks, j);
        val[SA[j]] = (total - base[b + 1]) + (j - base[b]);
    }
}

// factor start flags (1 at every block start and where the rank drops below every rank in front of it)
__global__ __launch_bounds__(256) void k_bwts_starts(const u32* __restrict__ val, const u32* __restrict__ pmin, const u32* __restrict__ base,
                                                     int nBlocks, u32 total, u32* __restrict__ flag)
{
    BWTS_FOR(p, total) {
        const int b = find_block(base, nBlocks, p);
        flag[p] = (p == base[b] || val[p] < pmin[p - 1]) ? 1u : 0u;
    }
}

// factor id of every position, start of every factor (fstart[nFactors] = total)
__global__ __launch_bounds__(256) void k_bwts_factors(const u32* __restrict__ flag, const u32* __restrict__ excl, u32 total, u32* __restrict__ fid,
                                                      u32* __restrict__ fstart)
{
    BWTS_FOR(p, total) {
        const u32 f = flag[p];
        fid[p] = excl[p] + f - 1u;
        if (f) fstart[excl[p]] = p;
        if (p == total - 1) fstart[excl[p] + f] = total;
    }
}

// initial state: one group per block (label = the block's first slot), identity slot order, every position unresolved;
// counters[0] = longest factor
__global__ __launch_bounds__(256) void k_bwts_init(const u32* __restrict__ base, int nBlocks, u32 total, const u32* __restrict__ fid,
                                                   const u32* __restrict__ fstart, u32* __restrict__ lab, u32* __restrict__ slotPos,
                                                   u32* __restrict__ list, u32* __restrict__ counters)
{
    u32 longest = 0;
    BWTS_FOR(p, total) {
        const int b = find_block(base, nBlocks, p);
        lab[p] = base[b];
        slotPos[p] = p;
        list[p] = p;
        if (fstart[fid[p]] == p) longest = max(longest, fstart[fid[p] + 1] - p);
    }
    longest = wave_max(longest);                                  // (every lane is back from the loop)
    if (lane_id() == 0 && longest) atomicMax(counters, longest);
}

// the rotation c positions on from position p, inside its factor
__device__ __forceinline__ u32 bwts_succ(u32 p, u32 s, u32 L, u32 c)
{
    return s + (u32)(((u64)(p - s) + c) % L);
}

struct BwtsText {
    const u8* const* src;
    const u32* base;
    int nBlocks;
};

// keys of a round: (label << lowBits) | low, low = the first four bytes of the rotation (c == 0) or the label c positions on
__global__ __launch_bounds__(256) void k_bwts_gather(BwtsText tx, const u32* __restrict__ list, u32 count, const u32* __restrict__ slotPos,
                                                     const u32* __restrict__ lab, const u32* __restrict__ fid, const u32* __restrict__ fstart,
                                                     u32 c, int lowBits, u64* __restrict__ keys, u32* __restrict__ vals)
{
    BWTS_FOR(u, count) {
        const u32 p = slotPos[list[u]];
        const u32 f = fid[p];
        const u32 s = fstart[f], L = fstart[f + 1] - s;
        u32 low;
        if (c == 0) {
            const int b = find_block(tx.base, tx.nBlocks, p);
            const u8* t = tx.src[b];
            const u32 bb = tx.base[b];
            low = 0;
            u32 q = p - s;
            for (int k = 0; k < 4; k++) {
                low = (low << 8) | (u32)t[s + q - bb];
                q = (q + 1 == L) ? 0u : q + 1;
            }
        } else {
            low = lab[bwts_succ(p, s, L, c)];
        }
        keys[u] = ((u64)lab[p] << lowBits) | (u64)low;
        vals[u] = p;
    }
}

// after the sort: where a new group (mark0) and where an old group (mark1) starts in the list
__global__ __launch_bounds__(256) void k_bwts_mark(const u64* __restrict__ keys, u32 count, int lowBits, u32* __restrict__ mark0, u32* __restrict__ mark1)
{
    BWTS_FOR(u, count) {
        const u64 k = keys[u];
        const u64 kp = u ? keys[u - 1] : ~k;
        mark0[u] = (u == 0 || k != kp) ? u : 0u;
        mark1[u] = (u == 0 || (k >> lowBits) != (kp >> lowBits)) ? u : 0u;
    }
}

// new slot order and labels; keep[u] = 1 where the member's new group has more than one member
__global__ __launch_bounds__(256) void k_bwts_apply(const u64* __restrict__ keys, const u32* __restrict__ vals, u32 count, int lowBits,
                                                    const u32* __restrict__ first0, const u32* __restrict__ first1, u32* __restrict__ slotPos,
                                                    u32* __restrict__ lab, u32* __restrict__ keep)
{
    BWTS_FOR(u, count) {
        const u64 k = keys[u];
        const u32 g = (u32)(k >> lowBits);
        const u32 p = vals[u];
        slotPos[g + (u - first1[u])] = p;
        lab[p] = g + (first0[u] - first1[u]);
        const bool alone = first0[u] == u && (u + 1 == count || keys[u + 1] != k);
        keep[u] = alone ? 0u : 1u;
    }
}

// the members still grouped, as slots, in slot order
__global__ __launch_bounds__(256) void k_bwts_compact(const u64* __restrict__ keys, u32 count, int lowBits, const u32* __restrict__ first1,
                                                      const u32* __restrict__ keep, const u32* __restrict__ at, u32* __restrict__ list)
{
    BWTS_FOR(u, count) {
        if (keep[u]) list[at[u]] = (u32)(keys[u] >> lowBits) + (u - first1[u]);
    }
}

__global__ __launch_bounds__(256) void k_bwts_emit(BwtsText tx, u8* const* dst, u32 total, const u32* __restrict__ slotPos,
                                                   const u32* __restrict__ fid, const u32* __restrict__ fstart)
{
    BWTS_FOR(j, total) {
        const int b = find_block(tx.base, tx.nBlocks, j);
        const u32 bb = tx.base[b];
        const u32 p = slotPos[j];
        const u32 f = fid[p];
        const u32 s = fstart[f];
        const u32 pred = (p == s) ? fstart[f + 1] - 1u : p - 1u;
        dst[b][j - bb] = tx.src[b][pred - bb];
    }
}

// blocks the sort did not take: n <= 1 are copied, n > cap refused; sorted blocks get ok and their length
__global__ void k_bwts_blocks(XfStage st)
{
    for (int b = blockIdx.x * 64 + threadIdx.x; b < st.nBlocks; b += gridDim.x * 64) {
        const u32 n = st.len[b];
        if (n > st.cap[b]) { st.ok[b] = 0; st.newLen[b] = 0; continue; }
        if (n == 1) st.dst[b][0] = st.src[b][0];
        st.ok[b] = 1;
        st.newLen[b] = n;
    }
}

struct BwtsFwdWs {
    u32 *val, *pmin, *flag, *excl, *fid, *fstart, *lab, *slotPos, *list, *t0, *t1, *t2, *t3, *valsA, *valsB, *counters;
    u64 *keysA, *keysB;
    void* scanTmp;
    void* rsMem;
};

size_t bwts_fwd_carve(u8* p, int nBlocks, size_t total, BwtsFwdWs* w)
{
    u8* q = p;
    auto take = [&](size_t sz) { u8* r = q; q += (sz + 255) & ~(size_t)255; return r; };
    const size_t n1 = total + 2;
    w->val = (u32*)take(4 * n1); w->pmin = (u32*)take(4 * n1); w->flag = (u32*)take(4 * n1); w->excl = (u32*)take(4 * n1);
    w->fid = (u32*)take(4 * n1); w->fstart = (u32*)take(4 * n1); w->lab = (u32*)take(4 * n1); w->slotPos = (u32*)take(4 * n1);
    w->list = (u32*)take(4 * n1); w->t0 = (u32*)take(4 * n1); w->t1 = (u32*)take(4 * n1); w->t2 = (u32*)take(4 * n1); w->t3 = (u32*)take(4 * n1);
    w->valsA = (u32*)take(4 * n1); w->valsB = (u32*)take(4 * n1);
    w->keysA = (u64*)take(8 * n1); w->keysB = (u64*)take(8 * n1);
    w->counters = (u32*)take(256);
    w->scanTmp = take(prims::scan_tmp_bytes(n1));
    w->rsMem = take(prims::rs_ws_bytes(n1, nBlocks + 1));
    return (size_t)(q - p);
}

// ---- inverse ------------------------------------------------------------------------------------------------------------------------

// dense bases of the blocks the inverse works on (2 <= n <= cap); ok / newLen of every block; counters[0] = total
__global__ void k_bwts_inv_bases(XfStage st, u32* __restrict__ base, u32* __restrict__ counters)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    u64 sum = 0;
    for (int b = 0; b < st.nBlocks; b++) {
        base[b] = (u32)sum;
        const u32 n = st.len[b];
        if (n > st.cap[b]) { st.ok[b] = 0; st.newLen[b] = 0; continue; }
        st.ok[b] = 1;
        st.newLen[b] = n;
        if (n == 1) st.dst[b][0] = st.src[b][0];
        if (n >= 2) sum += n;
    }
    base[st.nBlocks] = (u32)sum;
    counters[0] = sum >= 0xFFFFFFFFull ? 0xFFFFFFFFu : (u32)sum;
}

__global__ __launch_bounds__(256) void k_bwts_inv_load(BwtsText tx, u32 total, u32* __restrict__ keys, u32* __restrict__ vals)
{
    BWTS_FOR(i, total) {
        const int b = find_block(tx.base, tx.nBlocks, i);
        keys[i] = tx.src[b][i - tx.base[b]];
        vals[i] = i;
    }
}

// LF[i] = place of row i in the stable byte order
__global__ __launch_bounds__(256) void k_bwts_inv_lf(const u32* __restrict__ sortedRows, u32 total, u32* __restrict__ LF)
{
    BWTS_FOR(k, total) LF[sortedRows[k]] = k;
}

// Row state of the pointer jumping: x = smallest row of the window, y = steps from the row to the first occurrence of x in the window,
// z = the row the window ends in front of (w unused: one 16-byte record, one load per round)
// first window (two rows): the row and LF[row]
__global__ __launch_bounds__(256) void k_bwts_inv_jump0(const u32* __restrict__ LF, u32 total, uint4* __restrict__ S)
{
    BWTS_FOR(i, total) {
        const u32 l = LF[i];
        S[i] = make_uint4(l < i ? l : i, l < i ? 1u : 0u, LF[l], 0u);
    }
}

// one round: the window of W rows from i on and the one from its end on make one of 2W rows; a smaller minimum in the second half
// lies W + its offset there steps on. counters[1] != 0 when some minimum changed
__global__ __launch_bounds__(256) void k_bwts_inv_jump(const uint4* __restrict__ S, u32 total, u32 W, uint4* __restrict__ S2, u32* __restrict__ changed)
{
    bool ch = false;
    BWTS_FOR(i, total) {
        uint4 v = S[i];
        const uint4 a = S[v.z];
        if (a.x < v.x) { v.x = a.x; v.y = W + a.y; ch = true; }
        v.z = a.z;
        S2[i] = v;
    }
    const u64 any = __ballot(ch);                                 // (every lane is back from the loop)
    if (lane_id() == 0 && any) atomicOr(changed, 1u);
}

// cycle lengths at the smallest rows: the row behind the smallest one is length - 1 steps in front of it
__global__ __launch_bounds__(256) void k_bwts_inv_lengths(const uint4* __restrict__ S, const u32* __restrict__ LF, u32 total, u32* __restrict__ len)
{
    BWTS_FOR(i, total) len[i] = (S[i].x == i) ? S[LF[i]].y + 1u : 0u;
}

// row i, k steps behind the smallest row h of its cycle (k = length - offset, 0 at h), goes to n - 1 - (place of h's cycle) - k
__global__ __launch_bounds__(256) void k_bwts_inv_scatter(BwtsText tx, u8* const* dst, u32 total, const uint4* __restrict__ S, const u32* __restrict__ len,
                                                          const u32* __restrict__ off)
{
    BWTS_FOR(i, total) {
        const int b = find_block(tx.base, tx.nBlocks, i);
        const u32 bb = tx.base[b];
        const u32 n = tx.base[b + 1] - bb;
        const uint4 v = S[i];
        const u32 k = v.y ? len[v.x] - v.y : 0u;
        const u32 j = n - 1u - (off[v.x] - bb) - k;
        if (j < n) dst[b][j] = tx.src[b][i - bb];              // (always: the cycles of a block add up to n)
    }
}

struct BwtsInvWs {
    u32 *base, *counters, *keysA, *keysB, *valsA, *valsB, *LF;
    uint4* S[2];
    void* scanTmp;
    void* rsMem;
};

size_t bwts_inv_carve(u8* p, int nBlocks, size_t total, BwtsInvWs* w)
{
    u8* q = p;
    auto take = [&](size_t sz) { u8* r = q; q += (sz + 255) & ~(size_t)255; return r; };
    const size_t n1 = total + 2;
    w->base = (u32*)take(4ull * (nBlocks + 2)); w->counters = (u32*)take(256);
    w->keysA = (u32*)take(4 * n1); w->keysB = (u32*)take(4 * n1); w->valsA = (u32*)take(4 * n1); w->valsB = (u32*)take(4 * n1);
    w->LF = (u32*)take(4 * n1);
    for (int k = 0; k < 2; k++) w->S[k] = (uint4*)take(16 * n1);
    w->scanTmp = take(prims::scan_tmp_bytes(n1));
    w->rsMem = take(prims::rs_ws_bytes(n1, nBlocks + 1));
    return (size_t)(q - p);
}

}  // namespace

size_t bwts_forward_scratch_bytes(int nBlocks, u32 VS, size_t total)
{
    BwtsFwdWs w;
    return bwt_forward_scratch_bytes(nBlocks, VS, total) + bwts_fwd_carve(nullptr, nBlocks, total, &w) + 4096;
}

size_t bwts_inverse_scratch_bytes(int nBlocks, u32 VS, size_t total)
{
    (void)VS;
    BwtsInvWs w;
    return bwts_inv_carve(nullptr, nBlocks, total, &w) + 4096;
}

#define GRIDN(n) dim3(bwts_grid(n)), dim3(256), 0, s

// Returns 0 or a negative value (-2: scratch too small). Synchronises the stream (group counts are read back per round).
int launch_bwts_forward(hipStream_t s, const XfStage& st, void* scratch, size_t scratchBytes, u32* h_pinned)
{
    const size_t maxTotal = (size_t)st.nBlocks * st.maxLen;
    const size_t sortBytes = (bwt_forward_scratch_bytes(st.nBlocks, st.maxLen, maxTotal) + 255) & ~(size_t)255;
    BwtsFwdWs w;
    if (sortBytes + bwts_fwd_carve(nullptr, st.nBlocks, maxTotal, &w) > scratchBytes) return -2;
    bwts_fwd_carve(reinterpret_cast<u8*>(scratch) + sortBytes, st.nBlocks, maxTotal, &w);
    BwtSuffixArrays sa;
    if (int r = bwt_suffix_arrays(s, st, scratch, sortBytes, h_pinned, &sa)) return r;      // (its kernels time as k_bwt_f_*)
    if (sa.total > 0) {
        const u32 total = sa.total;
        BwtsText tx; tx.src = st.src; tx.base = sa.base; tx.nBlocks = st.nBlocks;
        { KScope ks_("k_bwts_f_factors");
          hipLaunchKernelGGL(k_bwts_rank_values, GRIDN(total), sa.SA, sa.base, st.nBlocks, total, w.val);
          prims::launch_scan<prims::SCAN_MIN_INCL>(s, w.val, w.pmin, total, nullptr, w.scanTmp);
          hipLaunchKernelGGL(k_bwts_starts, GRIDN(total), w.val, w.pmin, sa.base, st.nBlocks, total, w.flag);
          prims::launch_scan<prims::SCAN_SUM_EXCL>(s, w.flag, w.excl, total, nullptr, w.scanTmp);
          hipLaunchKernelGGL(k_bwts_factors, GRIDN(total), w.flag, w.excl, total, w.fid, w.fstart);
          hipMemsetAsync(w.counters, 0, 64, s);
          hipLaunchKernelGGL(k_bwts_init, GRIDN(total), sa.base, st.nBlocks, total, w.fid, w.fstart, w.lab, w.slotPos, w.list, w.counters); }
        if (hipMemcpyAsync(h_pinned, w.counters, 4, hipMemcpyDeviceToHost, s) != hipSuccess) return -1;
        if (hipStreamSynchronize(s) != hipSuccess) return -1;
        const u64 longest = h_pinned[0];
        int tb = 1;
        while ((1ull << tb) < (u64)total) tb++;                   // bits of a label (a slot)
        u32* seg2 = w.counters + 8;
        prims::RsWs rs = prims::rs_carve(w.rsMem, total, 2, seg2, 1);
        u32 count = total;
        u64 c = 0;                                                // the labels order the rotations on their first c bytes (0: not at all)
        for (;;) {
            const int lowBits = c == 0 ? 32 : tb;
            KScope ks_("k_bwts_f_round");
            hipLaunchKernelGGL(k_bwts_gather, GRIDN(count), tx, w.list, count, w.slotPos, w.lab, w.fid, w.fstart, (u32)c, lowBits, w.keysA, w.valsA);
            hipLaunchKernelGGL(prims::k_rs_one_segment, dim3(1), dim3(64), 0, s, seg2, count);
            prims::rs_launch_layout(s, rs);
            const int r = prims::rs_sort<u64, true>(s, rs, w.keysA, w.keysB, w.valsA, w.valsB, (size_t)count, 0, lowBits + tb);
            const u64* K = r ? w.keysB : w.keysA;
            const u32* V = r ? w.valsB : w.valsA;
            hipLaunchKernelGGL(k_bwts_mark, GRIDN(count), K, count, lowBits, w.t0, w.t1);
            prims::launch_scan<prims::SCAN_MAX_INCL>(s, w.t0, w.t0, count, nullptr, w.scanTmp);
            prims::launch_scan<prims::SCAN_MAX_INCL>(s, w.t1, w.t1, count, nullptr, w.scanTmp);
            hipLaunchKernelGGL(k_bwts_apply, GRIDN(count), K, V, count, lowBits, w.t0, w.t1, w.slotPos, w.lab, w.t2);
            prims::launch_scan<prims::SCAN_SUM_EXCL>(s, w.t2, w.t3, count, nullptr, w.scanTmp, w.counters + 1);
            hipLaunchKernelGGL(k_bwts_compact, GRIDN(count), K, count, lowBits, w.t1, w.t2, w.t3, w.list);
            if (hipMemcpyAsync(h_pinned, w.counters + 1, 4, hipMemcpyDeviceToHost, s) != hipSuccess) return -1;
            if (hipStreamSynchronize(s) != hipSuccess) return -1;
            count = h_pinned[0];
            c = c == 0 ? 4 : 2 * c;
            if (count == 0 || c >= 2 * longest) break;
        }
        { KScope ks_("k_bwts_f_emit"); hipLaunchKernelGGL(k_bwts_emit, GRIDN(total), tx, st.dst, total, w.slotPos, w.fid, w.fstart); }
    }
    hipLaunchKernelGGL(k_bwts_blocks, dim3((unsigned)((st.nBlocks + 63) / 64)), dim3(64), 0, s, st);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

// Returns 0 or a negative value (-2: scratch too small). Synchronises the stream (convergence flags are read back per round).
int launch_bwts_inverse(hipStream_t s, const XfStage& st, void* scratch, size_t scratchBytes, u32* h_pinned)
{
    const size_t maxTotal = (size_t)st.nBlocks * st.maxLen;
    BwtsInvWs w;
    if (bwts_inv_carve(nullptr, st.nBlocks, maxTotal, &w) > scratchBytes) return -2;
    bwts_inv_carve(reinterpret_cast<u8*>(scratch), st.nBlocks, maxTotal, &w);
    { KScope ks_("k_bwts_i_bases"); hipLaunchKernelGGL(k_bwts_inv_bases, dim3(1), dim3(64), 0, s, st, w.base, w.counters); }
    if (hipMemcpyAsync(h_pinned, w.counters, 4, hipMemcpyDeviceToHost, s) != hipSuccess) return -1;
    if (hipStreamSynchronize(s) != hipSuccess) return -1;
    const u32 total = h_pinned[0];
    if (total == 0) return hipGetLastError() == hipSuccess ? 0 : -1;
    if ((size_t)total > maxTotal) return -2;
    BwtsText tx; tx.src = st.src; tx.base = w.base; tx.nBlocks = st.nBlocks;
    { KScope ks_("k_bwts_i_lf");
      hipLaunchKernelGGL(k_bwts_inv_load, GRIDN(total), tx, total, w.keysA, w.valsA);
      prims::RsWs rs = prims::rs_carve(w.rsMem, total, st.nBlocks + 1, w.base, st.nBlocks);
      prims::rs_launch_layout(s, rs);
      const int r = prims::rs_sort<u32, true>(s, rs, w.keysA, w.keysB, w.valsA, w.valsB, (size_t)st.maxLen, 0, 8);
      hipLaunchKernelGGL(k_bwts_inv_lf, GRIDN(total), r ? w.valsB : w.valsA, total, w.LF); }
    // After the round that leaves the window at W rows, S[i].x = the smallest of the W rows from i on along LF, S[i].y = steps to it. A
    // round that changes no minimum means no cycle is longer than the window (else the row W steps in front of a longer cycle's smallest
    // row would have learnt it in that round), so every row knows its cycle's smallest row and how far on along LF it lies.
    int cur = 0;
    { KScope ks_("k_bwts_i_jump"); hipLaunchKernelGGL(k_bwts_inv_jump0, GRIDN(total), w.LF, total, w.S[0]); }
    u64 W = 2;
    for (;;) {
        if (W > (1ull << 32)) return -5;                          // cannot happen: a cycle has at most 2^30 rows
        KScope ks_("k_bwts_i_jump");
        hipMemsetAsync(w.counters + 1, 0, 4, s);
        hipLaunchKernelGGL(k_bwts_inv_jump, GRIDN(total), w.S[cur], total, (u32)W, w.S[cur ^ 1], w.counters + 1);
        cur ^= 1;
        W *= 2;
        if (hipMemcpyAsync(h_pinned, w.counters + 1, 4, hipMemcpyDeviceToHost, s) != hipSuccess) return -1;
        if (hipStreamSynchronize(s) != hipSuccess) return -1;
        if (h_pinned[0] == 0) break;
    }
    u32* len = w.keysA;                                           // (free since LF was built)
    u32* off = w.keysB;
    { KScope ks_("k_bwts_i_scatter");
      hipLaunchKernelGGL(k_bwts_inv_lengths, GRIDN(total), w.S[cur], w.LF, total, len);
      prims::launch_scan<prims::SCAN_SUM_EXCL>(s, len, off, total, nullptr, w.scanTmp);
      hipLaunchKernelGGL(k_bwts_inv_scatter, GRIDN(total), tx, st.dst, total, w.S[cur], len, off); }
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace knz
