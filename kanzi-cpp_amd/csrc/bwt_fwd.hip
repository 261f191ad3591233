// Forward Burrows-Wheeler transform (block codec) on gfx950: suffix sorting of all blocks of a batch at once.
//
// Reference being replaced (results are bit-identical; the suffix array of a block is unique, so any correct
// construction matches divsufsort):
//   transform/BWTBlockCodec.cpp:32-87 (header), transform/BWT.cpp:92-134, transform/DivSufSort.cpp:171-295
//   (computeBWT / constructBWT): "proper prefix sorts first", out[0] = in[n-1], then in[SA[r]-1] for ranks with
//   SA[r] != 0, 8 primary indexes rank(suffix k*ceil(n/8)) + 1 (BWT.hpp:40-61).
//
// GPU formulation: prefix doubling with group refinement (Larsson-Sadakane order refinement, made data parallel).
//   State in HBM: SA[slot] (global position ids), ISA[position] = a label of the position's group (a slot inside the group's range), and
//   one bit per slot, gbits, set where a group starts. A position is resolved when its group has one member.
//   Round 0 sorts every block's suffixes on their first 4 or 5 symbols with the segmented LSD radix sort of prims.hpp; its first pass reads
//   the text. Then:
//     * the small groups once on the next seven text bytes, in the kernel that places round 0 (k_bwt_f_r0_place_text),
//     * run groups (4 equal symbols) in one round by run length: the runs are sorted, the members follow their runs (k_bwt_f_run_*),
//       and because that round rebuilds every member from the text, the members stay out of round 0's sort: the run groups are found in
//       the text before the sort (FwdSort::run_scan), the first pass drops their members, the last pass leaves a gap per group where they
//       belong, one key fills its two ends and nobody reads its inside (TextSrcKept, LastPassSrc, k_bwt_f_r0_fill, R0_GAP_MARGIN; knob
//       bwt_run_in_sort: through the sort as before),
//   and the doubling rounds, h = 4, 8, 16, ..., refine what is left on the key ISA[p + h] (0 past the block end: "shorter sorts first"):
//     * small groups (2..256 members) need no list at all: a kernel sweeps the bit map in windows of 2048 slots, finds the groups that
//       start in its window and ranks every member by counting inside LDS (less / equal / equal-before),
//     * medium groups (257..8192) are (start, length) descriptors (found through staging slots, no atomics); one workgroup sorts a
//       group in LDS: majority-key split or a stable LSD radix sort (8-bit digits, ranking by ballot matching inside a wave),
//     * a group whose majority key is its OWN label (a periodic stretch whose period divides h) is finished in one round by pointer
//       jumping along its chains (med_chain_round, inside the workgroup that holds the group in LDS anyway),
//     * large groups go through one global radix sort of (descriptor index, key) pairs.
//   A round sorts on the labels as they stood when it began (a refined head read beside an unrefined one would order two suffixes that
//   are still equal): the keys of medium and large groups are gathered by kernels of their own before anything moves; the small groups
//   read theirs in the kernel that sorts them (k_bwt_f_small_fused, round 6), which the VERSIONED labels make safe (lab_old / lab_set below);
//   blocks above 256 MiB keep plain labels and gather the small groups' keys first as well (k_bwt_f_gather_small, k_bwt_f_sort_small).
#include "common.hpp"
#include "stages.hpp"
#include "bwt_common.hpp"

#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <cmath>
#include "prims.hpp"
#include <chrono>
#include <vector>

namespace knz {

constexpr u32 SM_TS = 1792;        // slots owned by one window
constexpr u32 SM_WIN = 2048;       // slots a window looks at (owned + halo)
constexpr u32 SM_G = 256;          // largest "small" group
// largest "medium" group (one workgroup, LDS resident). Round 6 measured 16,384 with a 1024 x 16 instantiation of k_bwt_f_sort_medium (150 KiB of
// LDS, one workgroup per CU): period-768 blocks 19.0 -> 9.8 ms, but real files 51.7 -> 52.6, the stand-in 26.6 -> 26.9 -- for groups of that
// size the global sort of (descriptor, key) pairs is no slower than one workgroup per CU. Stays 8,192.
constexpr u32 MED_CAP = 8192;
constexpr u32 MED_LO_CAP = 2048;   // medium groups up to here are sorted by workgroups of 256 threads x 8 members, larger ones by 512 x 16
constexpr u32 CHAIN_CAP = 8192;   // largest group the chain round and the periodic-stretch probe take
constexpr int GATHER_THREADS = 512;        // workgroup of k_bwt_f_gather_desc
constexpr u32 GATHER_ROWS = 16;            // members it holds per thread: a medium group whole
static_assert(MED_CAP <= GATHER_ROWS * GATHER_THREADS, "k_bwt_f_gather_desc judges a medium group from one batch of loads");
constexpr u32 LARGE_OS_MIN = 1000000;      // members from which the sort of the large groups uses the one-sweep radix passes
constexpr u32 NO_BIT = 0x7FFFFFFFu;

struct FwdView {
    const u32* base;     // [nBlocks + 1] slot / position base of every block (dense), base[nBlocks] = total
    int nBlocks;
    u32 total;
    u32* SA;             // [total]
    u32* ISA;            // [total] labels as 32-bit words (blocks above 256 MiB), or
    u64* ISA2;           // [total] VERSIONED labels (null: the plain words above): see lab_old / lab_set below
    u32 round;           // number of the doubling round under way (0: in front of the first one)
    u32* K;              // [total] keys of the round, by slot
    u32* gbits;          // group-start bit per slot (bit k of word w = slot 32 w + k); set for every slot >= total
    u32* gnew;           // group starts found in the current round; merged into gbits when the round is over (a window must
                         // not see the subgroups a neighbouring window has just made: their keys belong to the old order)
    u32* counters;       // [64] words, the slots of FwdCounter
    const u32* ovr;      // [total] by slot: run length R of the members of a group the run round left unresolved (valid where rtbits is set)
    const u32* rtbits;   // bit per slot: the slot belongs to such a group. Its members are c^R followed by different things, so the key that
                         // tells them apart is the label R positions on -- the doubling rounds look there (at max(R, h)) instead of h positions
                         // on, where for h < R they would find the same run again and learn nothing (null: no run round)
    uint2* medStage;     // medium groups found in the current round, one slot per 256 slots of SA (a medium group has more than 256
                         // members, so two of them never start in the same 256): written without atomics, compacted -- in slot order --
                         // into the next round's descriptor list by k_bwt_f_med_compact
    uint2* verdictNow;   // per staging slot: (key, verdict_word) of a medium group this round leaves whole (k_bwt_f_gather_desc's verdict,
                         // k_bwt_f_med_sleep); null: not recorded (knob bwt_no_group_sleep)
    const uint2* verdictWas;     // what the round before recorded (the two buffers take turns; an entry names its round)
};

// What a round knows of a medium group it left whole, by the group's staging slot: .x = the one key all members carried (the label of the
// group they all found, as gather_key gives it), .y = [round, 8 bits | status | members, 16 bits]. PLAIN: the key was looked up at the
// round's plain offset h and is no past-the-end sentinel -- what k_bwt_f_med_sleep may build on; WHOLE: left whole, nothing more said.
constexpr u32 VERDICT_WHOLE = 1, VERDICT_PLAIN = 2;
__host__ __device__ __forceinline__ u32 verdict_word(u32 round, u32 status, u32 members) { return (round << 24) | (status << 16) | members; }
static_assert(MED_CAP < (1u << 16), "verdict_word keeps a medium group's size in 16 bits");

// Slots of FwdView::counters. Slots 0-23 are zeroed in front of every doubling round and read back after it; the host reads its copy
// slot for slot (FwdSort::fetch).
enum FwdCounter : u32 {
    CNT_SMALL_LEFT = 0,          // != 0: small groups are left
    CNT_MED = 1,                 // medium descriptors (k_bwt_f_med_compact)
    CNT_LARGE = 2,               // large descriptors
    CNT_LARGE_MEMBERS = 3,       // members of large groups
    CNT_RUN = 4,                 // run groups (round 0)
    CNT_RUN_MEMBERS = 5,         // their members
    CNT_RUN_LONGEST = 6,         // longest run (run round)
    CNT_CHAINED = 7,             // groups that took the chain round (med_chain_round)
    CNT_RUNS = 8,                // runs of run-group bytes (run round)
    CNT_MED_LO = 9,              // medium descriptors of the lower size class, up to MED_LO_CAP members (k_bwt_f_med_compact)
    CNT_STAT_SMALL = 10,         // small members worked on (knob bwt_stats)
    CNT_STAT_SMALL_GROUPS = 11,  // small groups worked on (knob bwt_stats)
    CNT_STAT_MED = 12,           // in a doubling round: medium members worked on (knob bwt_stats)
    CNT_STAT_R0_SKIPPED = 12,    // in round 0: workgroups of k_bwt_f_r0_flags that lay inside a gap and loaded no key (knob bwt_stats)
    CNT_TIED = 13,               // small members still tied after the round (the windows' counts summed)
    CNT_PROBE_CAND = 14,         // after round 0, owned by the probe: candidates of k_bwt_f_probe (k_bwt_f_probe_scan)
    CNT_LINKED = 14,             // in a doubling round, owned by the link step: members linked (k_bwt_f_link_payoff)
    CNT_LINK_TIED = 15,          // link step: members of the linked windows still tied after the round
    CNT_STAT_MED_GROUPS = 16,    // medium groups worked on (knob bwt_stats, like the four below)
    CNT_STAT_UNSPLIT = 17,       // medium groups whose members all carry one key: the round cannot split them
    CNT_STAT_UNSPLIT_MEMBERS = 18,
    CNT_STAT_MAJ = 19,           // medium groups that take med_majority_write_back (a majority key and at most THREADS others)
    CNT_STAT_MAJ_MEMBERS = 20,
    CNT_STAT_ASLEEP = 21,        // medium groups k_bwt_f_med_sleep kept out of the gather (counted among the ones above as well)
    CNT_STAT_ASLEEP_MEMBERS = 22,
    CNT_RUN_TILES = 23,          // tiles of the run round's direct placement (device side only: k_bwt_f_run_tile_starts' scan)
    CNT_ROUND_SLOTS = 24,
    CNT_GAP_CLASSES = 25,        // run groups found before round 0's sort (k_bwt_f_run_scan_classes; behind the rounds' slots: round 0 zeroes those)
    CNT_GAP_MEMBERS = 26,        // their members: what stays out of the sort
    CNT_PROBE_SLOTS = 2,         // slots 0-1 (CNT_SMALL_LEFT, CNT_MED): what the probe zeroes, recounts and reads back
    CNT_LONGEST_BLOCK = 32,      // longest block the transform applies to (k_bwt_bases)
    CNT_NSYM = 33,               // round-0 key length the entropy asks for (k_bwt_f_choose_nsym)
};

// ---- labels --------------------------------------------------------------------------------------------------------------------------
// A round must sort on the labels as they stood when it began: a refined label read beside one that is still to be refined would order two
// suffixes that are equal so far (the old label of a group says nothing about where its members go). Rounds 1-5 therefore gathered all keys
// of a round (k_bwt_f_gather_*) before any kernel of it changed a label. With VERSIONED labels a kernel may read keys and write labels in the
// same launch: an entry of ISA2 holds, in one 64-bit word that is read and written whole,
//     bits 0-27 the label, bits 28-55 the label it replaced, bits 56-63 the round in which it was written,
// labels as slots relative to their block's first slot (blocks up to 2^28 bytes; larger ones use the plain words and separate key
// kernels). A reader of round r takes the replaced label when the entry carries r's number -- whatever kernel of the round wrote it, before
// or beside the reader -- and the label otherwise. A position changes its label at most once per round (it is a member of one group).
// Writers outside the rounds (round 0, text round, run round, probe: nobody reads beside them) write label = replaced label, number 0.
constexpr u32 LAB_BITS = 28;
constexpr u64 LAB_MASK = (1ull << LAB_BITS) - 1ull;

// label of position q as of the end of the previous round (global slot); bb = first slot of q's block
__device__ __forceinline__ u32 lab_old(const FwdView& v, u32 q, u32 bb)
{
    if (v.ISA2 == nullptr) return v.ISA[q];
    const u64 e = v.ISA2[q];
    const u32 rel = ((u32)(e >> 56) == v.round && v.round != 0) ? (u32)((e >> LAB_BITS) & LAB_MASK) : (u32)(e & LAB_MASK);
    return bb + rel;
}
// the latest label (for kernels that run where no label changes)
__device__ __forceinline__ u32 lab_cur(const FwdView& v, u32 q, u32 bb)
{
    if (v.ISA2 == nullptr) return v.ISA[q];
    return bb + (u32)(v.ISA2[q] & LAB_MASK);
}
// position p of the block that starts at slot bb goes from label `was` to label `lab` (global slots)
__device__ __forceinline__ void lab_set(const FwdView& v, u32 p, u32 bb, u32 lab, u32 was)
{
    if (v.ISA2 == nullptr) { v.ISA[p] = lab; return; }
#ifdef KNZ_EMU
    // `was` must be the label the position had when the round began (the placing kernels pass the group's first slot)
    if (v.round != 0 && lab_old(v, p, bb) != was) {
        fprintf(stderr, "lab_set: round %u position %u: was %u, label %u\n", v.round, p, was, lab_old(v, p, bb));
        abort();
    }
#endif
    const u64 nw = (u64)(lab - bb), ow = (v.round == 0) ? nw : (u64)(was - bb);
    v.ISA2[p] = nw | (ow << LAB_BITS) | ((u64)v.round << 56);
}

__device__ __forceinline__ u32 gather_key(const FwdView& v, u32 gp, u32 h, u32 blkBase, u32 blkEnd)
{
    const u32 q = gp + h;
    return (q < blkEnd) ? lab_old(v, q, blkBase) - blkBase + 1u : 0u;
}

// Is the slot in a group the run round, the probe or the link step left with a shared length of its own (FwdView::rtbits, ovr)?
__device__ __forceinline__ bool look_marked(const FwdView& v, u32 slot) { return v.rtbits && ((v.rtbits[slot >> 5] >> (slot & 31)) & 1u); }
// The offset a group (by its first slot) or a slot looks at in the round of offset h: h, or max(ovr, h) where the slot is marked. A group is
// marked whole, so its first slot answers for all members. (marked: where the caller holds the bit already, as the small-group windows do.)
__device__ __forceinline__ u32 look_offset(const FwdView& v, u32 slot, u32 h, bool marked)
{
    if (!marked) return h;
    const u32 r = v.ovr[slot];
    return r > h ? r : h;
}
__device__ __forceinline__ u32 look_offset(const FwdView& v, u32 slot, u32 h) { return look_offset(v, slot, h, look_marked(v, slot)); }

// A medium group d all of whose members found key0, looking off positions on, is left whole: staged for the next round's list as
// med_write_back would have, the verdict recorded for k_bwt_f_med_sleep, counted (stats: knob bwt_stats). By one thread.
__device__ __forceinline__ void med_leave_whole(const FwdView& v, uint2 d, u32 key0, u32 off, u32 h, bool stats)
{
    v.medStage[d.x >> 8] = d;
    if (v.verdictNow) v.verdictNow[d.x >> 8] = make_uint2(key0, verdict_word(v.round, (off == h && key0 != 0u) ? VERDICT_PLAIN : VERDICT_WHOLE, d.y));
    if (stats) { atomicAdd(&v.counters[CNT_STAT_UNSPLIT], 1u); atomicAdd(&v.counters[CNT_STAT_UNSPLIT_MEMBERS], d.y); }
}

__device__ __forceinline__ void classify_child(const FwdView& v, uint2* __restrict__ medNext, uint2* __restrict__ largeNext, u32 start, u32 size, u32& surv)
{
    if (size > MED_CAP) {
        const u32 at = atomicAdd(&v.counters[CNT_LARGE], 1u);
        largeNext[at] = make_uint2(start, size);
        atomicAdd(&v.counters[CNT_LARGE_MEMBERS], size);
    } else if (size > SM_G) {
        v.medStage[start >> 8] = make_uint2(start, size);
    } else if (size > 1) {
        surv = 1;
    }
}

// The same through the workgroup: the large / run groups a workgroup finds are counted in LDS first, ONE thread then reserves their
// places in the lists (one global atomic per list and workgroup instead of one per group), and the descriptors are written at
// base + local index. Medium groups -- hundreds of thousands after round 0 of a text, where atomics on ONE counter were two thirds
// of k_bwt_f_r0_place -- use no counter at all: they go to v.medStage (see FwdView).
struct ClassAgg { u32 cnt[3]; u32 elems[3]; u32 base[3]; };        // 0 medium, 1 large, 2 run groups

__device__ __forceinline__ void agg_init(ClassAgg& A) { if (threadIdx.x < 3) { A.cnt[threadIdx.x] = 0; A.elems[threadIdx.x] = 0; A.base[threadIdx.x] = 0; } }

// kind of the group (-1: small or resolved) and its index among the workgroup's groups of that kind
__device__ __forceinline__ int agg_note(ClassAgg& A, u32 size, bool run, u32& surv, u32& local)
{
    int kind;
    if (run) kind = 2;
    else if (size > MED_CAP) kind = 1;
    else if (size > SM_G) kind = 0;
    else { if (size > 1) surv = 1; return -1; }
    if (kind != 0) { local = atomicAdd(&A.cnt[kind], 1u); atomicAdd(&A.elems[kind], size); }
    return kind;
}

// one thread, between two barriers
__device__ __forceinline__ void agg_reserve(ClassAgg& A, const FwdView& v)
{
    if (A.cnt[1]) { A.base[1] = atomicAdd(&v.counters[CNT_LARGE], A.cnt[1]); atomicAdd(&v.counters[CNT_LARGE_MEMBERS], A.elems[1]); }
    if (A.cnt[2]) { A.base[2] = atomicAdd(&v.counters[CNT_RUN], A.cnt[2]); atomicAdd(&v.counters[CNT_RUN_MEMBERS], A.elems[2]); }
}

__device__ __forceinline__ void agg_write(const ClassAgg& A, const FwdView& v, int kind, u32 local, u32 start, u32 size, uint2* __restrict__ largeNext,
                                          uint2* __restrict__ runList)
{
    if (kind == 0) { v.medStage[start >> 8] = make_uint2(start, size); return; }        // (medium groups: no counter at all)
    uint2* dst = kind == 1 ? largeNext : runList;
    dst[A.base[kind] + local] = make_uint2(start, size);
}

// ------------------------------------------------------------------------------------------------
// round 0
// ------------------------------------------------------------------------------------------------
// base[b] = sum of active lengths of the blocks before b ; total in base[nBlocks]
// (suffixOnly: the suffix array for BWTS, bwts.hip: every block of at least 2 bytes that fits its destination is sorted)
__global__ void k_bwt_bases(BwtView v, u32* __restrict__ base, u8* __restrict__ ok, u32* __restrict__ maxLen, int suffixOnly)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    u32 sum = 0, mx = 0;
    for (int b = 0; b < v.nBlocks; b++) {
        base[b] = sum;
        u32 ps;
        const bool a = suffixOnly ? (v.len[b] >= 2 && v.len[b] <= v.cap[b]) : bwt_fwd_applies(v.len[b], v.cap[b], &ps);
        ok[b] = a ? 1 : 0;
        if (a) { sum += v.len[b]; mx = v.len[b] > mx ? v.len[b] : mx; }
    }
    base[v.nBlocks] = sum;
    *maxLen = mx;                       // longest block the transform applies to
}

// Round-0 key of a suffix: [P bytes of the suffix, zero past the block end | position inside the block in the low pbits bits].
// There is no block field (every block is a segment of the sort with its own digit bins) and no length field: the P - 1 suffixes
// that end inside their own key ("short" suffixes) are handed to the first pass IN FRONT of the others, shortest first, and the
// sort is stable -- so among equal padded keys they come first, shortest first, which is their place ("a proper prefix sorts
// first"); the flag kernel makes each of them a group of its own.
struct TextSrc {
    static constexpr bool STAGED = true, FILTER = false, SHIFTS = false;
    const u8* const* src;
    int P, pbits, shift;
    __device__ __forceinline__ u32 tab(int, u32) const { return 0u; }
    __device__ __forceinline__ bool keep(int, u32, u64, const u32*) const { return true; }
    __device__ __forceinline__ u32 out_shift(u64, u32, u32 at, const u32*) const { return at; }
    __device__ __forceinline__ void note_tile(int, u32, const u64*, u32, u32, const u32*) const {}
    __device__ __forceinline__ u32 pos_of(u32 n, u32 i) const
    {
        const u32 nShort = (u32)(P - 1) < n ? (u32)(P - 1) : n;
        return i < nShort ? n - 1 - i : i - nShort;
    }
    __device__ __forceinline__ u64 load(int sgm, u32, u32 n, u32 i) const
    {
        const u8* t = src[sgm];
        const u32 pos = pos_of(n, i);
        const u64 v = text8(t, pos, n);
        u64 kb = __builtin_bswap64(v) >> (64 - 8 * P);
        const u32 left = n - pos;
        if (left < (u32)P) kb &= ~0ull << (8 * ((u32)P - left));
        return (kb << pbits) | (u64)pos;
    }
    // The tile's stretch of the text in LDS (round 6; the pass took 1.57 ms against 0.97 for a pass over keys: a key was three dword loads
    // that overlap the neighbours'). Elements tile0 .. tile0 + RS_TILE - 1 are consecutive positions from pos0 on (the short suffixes in
    // front of the first tile keep the loads above): the dwords from the one that holds pos0 to the one behind pos0 + RS_TILE + 7, zero from
    // the block's end on, which is what text8 delivers there. A block whose text is not dword aligned is not staged.
    __device__ __forceinline__ bool stage(int sgm, u32 n, u32 tile0, u32* lds, int tid) const
    {
        const u8* t = src[sgm];
        if (reinterpret_cast<uintptr_t>(t) & 3) return false;
        const u32 nShort = (u32)(P - 1) < n ? (u32)(P - 1) : n;
        const u32 pos0 = (tile0 > nShort ? tile0 : nShort) - nShort;
        const u32 a0 = pos0 & ~3u;
        constexpr u32 NW = (prims::RS_TILE + 8u + 3u) / 4u + 2u;
        for (u32 w = (u32)tid; w < NW; w += (u32)prims::RS_THREADS) {
            const u32 q = a0 + 4u * w;
            u32 x = 0;
            if (q + 4u <= n) x = ldg<u32>(t + q);
            else for (u32 j = 0; j < 4u; j++) if (q + j < n) x |= (u32)ldg<u8>(t + q + j) << (8u * j);
            lds[w] = x;
        }
        return true;
    }
    __device__ __forceinline__ u64 load_staged(int sgm, u32 b0, u32 n, u32 i, const u32* lds, u32 tile0) const
    {
        const u32 nShort = (u32)(P - 1) < n ? (u32)(P - 1) : n;
        if (i < nShort) return load(sgm, b0, n, i);
        const u32 pos0 = (tile0 > nShort ? tile0 : nShort) - nShort;
        const u32 pos = i - nShort;
        const u32 o = pos - (pos0 & ~3u);
        const u32 w = o >> 2, sh = (o & 3u) * 8u;
        const u64 lo = (u64)lds[w] | ((u64)lds[w + 1] << 32);
        const u64 v = sh ? ((lo >> sh) | ((u64)lds[w + 2] << (64u - sh))) : lo;
        u64 kb = __builtin_bswap64(v) >> (64 - 8 * P);
        const u32 left = n - pos;
        if (left < (u32)P) kb &= ~0ull << (8 * ((u32)P - left));
        return (kb << pbits) | (u64)pos;
    }
    __device__ __forceinline__ u32 digit(u64 k) const { return (u32)(k >> shift) & 255u; }
    // (the first pass sorts on the last key byte)
    __device__ __forceinline__ u32 digit_at(int sgm, u32, u32 n, u32 i) const
    {
        const u32 q = pos_of(n, i) + (u32)(P - 1);
        return q < n ? (u32)ldg<u8>(src[sgm] + q) : 0u;
    }
};

// ---- round 0 without the run members ---------------------------------------------------------------------------------------------------
// A suffix that starts with P copies of a byte c, full length, is a RUN MEMBER when its block holds more than SM_G of them: round 0 makes
// one group of them (a run group) and the run round then rebuilds every one of them -- position, label and all -- from the text alone.
// So they stay out of the sort (FwdSort::run_scan decides, before the sort, from the runs of the text):
//   * the first pass drops them (TextSrcKept) and writes every block's other keys as a compact segment, which the middle passes sort;
//   * the last pass (LastPassSrc) writes to the slots the full sort would have used: the first output position of a first byte comes from
//     the full byte histogram, and a key with first byte c that is larger than c c .. c moves up by the members of c. What is in front of
//     the gap -- the smaller keys and the short suffixes, whose zero padding makes them at most equal -- is where stability puts it;
//   * the gap is filled with the class's key and the position of its first member (k_bwt_f_r0_fill), so that the flag and placing kernels
//     find one group per gap exactly where the run group was; the placing kernel writes SA and label for the gap's first slot only.
// Knob bwt_run_in_sort: the members go through the sort as before.
__host__ __device__ __forceinline__ u64 rep_key(u32 c, int P) { return (u64)c * (0x0101010101010101ull >> (64 - 8 * P)); }     // P copies of c

struct TextSrcKept : TextSrc {
    static constexpr bool FILTER = true;
    const u32* members;      // [block][256]: members of the byte's run group (0: it has none)
    __device__ __forceinline__ u32 tab(int sgm, u32 c) const { return members[(u32)sgm * 256u + c]; }
    __device__ __forceinline__ bool keep(int, u32 n, u64 k, const u32* tab) const
    {
        const u64 bytes = k >> pbits;
        const u32 c = (u32)bytes & 255u;
        if (bytes != rep_key(c, P)) return true;
        if ((u32)(k & ((1ull << pbits) - 1ull)) + (u32)P > n) return true;         // (a short suffix of zeros)
        return tab[c] == 0u;
    }
};

struct LastPassSrc : prims::DigitOfKey<u64> {
    static constexpr bool SHIFTS = true;
    const u32* members;      // as above
    u32* gapStart;           // [block][256]: first slot of the gap, preset to the end of the byte's slots less the members; the least unshifted
                             // position of a key that moves is where the gap starts
    int P, pbits;
    __device__ __forceinline__ bool above(u64 k) const { const u64 bytes = k >> pbits; return bytes > rep_key((u32)(bytes >> (8 * (P - 1))), P); }
    __device__ __forceinline__ u32 tab(int sgm, u32 d) const { return members[(u32)sgm * 256u + d]; }
    __device__ __forceinline__ u32 out_shift(u64 k, u32 d, u32 at, const u32* tab) const { return above(k) ? at + tab[d] : at; }
    // The tile's cnt keys of first byte d, whose first goes to at0: they come in the order of their other bytes, so the ones that move are
    // behind the ones that stay, and the first of them (found by bisection) is this tile's bid for the gap's start. Most tiles bid
    // nothing: no key that moves, or a bid that is not below what is known (read first: an atomic per tile and byte on the classes' few
    // words would queue up)
    __device__ __forceinline__ void note_tile(int sgm, u32 d, const u64* ks, u32 cnt, u32 at0, const u32* tab) const
    {
        if (tab[d] == 0u || cnt == 0u || !above(ks[cnt - 1u])) return;
        u32 lo = 0, hi = cnt - 1u;
        while (lo < hi) { const u32 mid = (lo + hi) >> 1; if (above(ks[mid])) hi = mid; else lo = mid + 1u; }
        u32* g = &gapStart[(u32)sgm * 256u + d];
        if (at0 + lo < ld_agent(g)) atomicMin(g, at0 + lo);
    }
};

// Byte histogram of every block (slices of a block by blockIdx.x, summed with atomics into byteHist[block][256], zeroed by the caller).
// Two things are read off it: the key length of round 0 (k_bwt_f_choose_nsym) and the digit counts of all round-0 passes
// (k_bwt_f_r0_counts; prims::k_rs_hist_all would build every key to count its bytes).
__global__ __launch_bounds__(256) void k_bwt_f_bytehist(BwtView bv, const u32* __restrict__ base, u32* __restrict__ byteHist)
{
    // four counter sets per wave (lane & 3 picks one; 257 words apart so that equal symbols of different sets fall into different banks):
    // lanes that show the same symbol in one step serialise on its counter, and text shows its few frequent symbols in most steps
    __shared__ u32 cnt[4][4][257];
    const int sgm = blockIdx.y;
    const u32 n = base[sgm + 1] - base[sgm];
    if (n == 0) return;
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int q = tid; q < 4 * 4 * 257; q += 256) (&cnt[0][0][0])[q] = 0;
    __syncthreads();
    const u8* t = bv.src[sgm];
    const u32 per = ((n + gridDim.x - 1) / gridDim.x + 15u) & ~15u;
    const u32 lo = blockIdx.x * per, hi = (lo + per < n) ? lo + per : n;
    // 16 bytes per lane and step (the block's text is 16-byte aligned or the slow path below takes it)
    const bool al = (reinterpret_cast<uintptr_t>(t) & 15) == 0;
    u32* mine = cnt[wave][lane & 3];
    for (u32 i0 = lo; i0 < hi; i0 += 16u * 256u) {                 // (uniform trip count: the row ballots want whole waves)
        const u32 i = i0 + 16u * (u32)tid;
        u32 wds[4] = { 0, 0, 0, 0 };
        const u32 m = (i >= hi) ? 0u : ((hi - i < 16u) ? hi - i : 16u);
        if (al && m == 16u) { wds[0] = ldg<u32>(t + i); wds[1] = ldg<u32>(t + i + 4); wds[2] = ldg<u32>(t + i + 8); wds[3] = ldg<u32>(t + i + 12); }
        else for (u32 j = 0; j < m; j++) wds[j >> 2] |= (u32)ldg<u8>(t + i + j) << (8 * (j & 3));
#pragma unroll
        for (u32 j = 0; j < 16; j++) {
            const bool valid = j < m;
            const u32 dg = (wds[j >> 2] >> (8 * (j & 3))) & 255u;
            const u32 d0 = uni(dg);
            const unsigned long long va = __ballot(valid);
            if (__ballot(valid && dg != d0) == 0) { if (lane == 0 && va) mine[d0] += (u32)__popcll(va); }
            else if (valid) atomicAdd(&mine[dg], 1u);
            KNZ_WAVE_ORDER();
        }
    }
    __syncthreads();
    u32 c = 0;
    for (int w = 0; w < 4; w++) for (int q = 0; q < 4; q++) c += cnt[w][q][tid];
    if (c) atomicAdd(&byteHist[(size_t)sgm * 256 + tid], c);
}

// Key length of round 0 from the order-0 entropy H of the blocks: four symbols tell suffixes apart when 4 H bits reach the
// log2(block length) bits a position has (the mixed stand-in: H = 6.8); text (H = 4.1), DNA (2.0) leave most suffixes in groups then,
// and a fifth symbol in the keys is cheaper than the doubling rounds those groups cost (measured on 212 MB of text at 8 MiB blocks:
// suffix sort 33.3 -> 29.6 ms; on the stand-in 27.1 -> 27.3). The host caps the answer by what fits the key beside the position.
// Round 6: H is the MEAN OF THE BLOCKS' entropies, weighted by their lengths, not the entropy of the batch's summed histogram -- a batch of
// different files (shared objects at 6-7 bits beside headers and scripts at 4.3-4.9) has a flat sum (6.1 for the real-file corpus) although
// most of its blocks are text-like: five symbols are worth 1.0 ms of 51.7 there. Batches of more than 64 blocks keep the summed histogram.
__global__ __launch_bounds__(256) void k_bwt_f_choose_nsym(const u32* __restrict__ byteHist, int nBlocks, const u32* __restrict__ longest, u32* __restrict__ out)
{
    __shared__ float part[256];
    __shared__ unsigned long long tot[256];
    const int tid = (int)threadIdx.x;
    float Hsum = 0.0f;                                   // (thread 0: sum of length x entropy over the blocks)
    unsigned long long lenSum = 0;
    const int nParts = nBlocks <= 64 ? nBlocks : 1;
    for (int q = 0; q < nParts; q++) {
        unsigned long long c = 0;
        if (nParts == 1) { for (int b = 0; b < nBlocks; b++) c += byteHist[(size_t)b * 256 + tid]; }
        else c = byteHist[(size_t)q * 256 + tid];
        tot[tid] = c;
        __syncthreads();
        unsigned long long all = 0;
        for (int i = 0; i < 256; i++) all += tot[i];
        part[tid] = (c && all) ? (float)((double)c / (double)all) * log2f((float)((double)all / (double)c)) : 0.0f;
        __syncthreads();
        if (tid == 0) {
            float H = 0.0f;
            for (int i = 0; i < 256; i++) H += part[i];
            Hsum += H * (float)all;
            lenSum += all;
        }
        __syncthreads();
    }
    if (tid == 0) {
        const float H = lenSum ? Hsum / (float)lenSum : 8.0f;
        const u32 n = longest[0] > 1 ? longest[0] : 2;
        out[0] = (4.0f * H < log2f((float)n)) ? 5u : 4u;
    }
}

// digit counts of the P round-0 passes of a block: the digit of pass k of the suffix at pos is the text byte at pos + o, o = P - 1 - k,
// or 0 behind the block's end, so its histogram is the block's byte histogram minus the block's first o bytes, plus o zeros
// (members: the run members that stay out of the sort, per block and byte, or null. Every digit of a member is its byte; the last pass keeps
// the full counts, which leaves the members' slots free)
__global__ __launch_bounds__(256) void k_bwt_f_r0_counts(BwtView bv, const u32* __restrict__ base, const u32* __restrict__ byteHist, int P, prims::RsLayout L,
                                                         const u32* __restrict__ members)
{
    const int sgm = blockIdx.x, tid = (int)threadIdx.x;
    const u32 n = base[sgm + 1] - base[sgm];
    const u32 c = n ? byteHist[(size_t)sgm * 256 + tid] : 0u;
    const u32 out = (members != nullptr && n) ? members[(size_t)sgm * 256 + tid] : 0u;
    const u8* t = bv.src[sgm];
    for (int k = 0; k < P; k++) {
        const u32 o = (u32)(P - 1 - k);
        const u32 oo = o < n ? o : n;
        u32 cut = 0;
        for (u32 j = 0; j < oo; j++) cut += ((u32)ldg<u8>(t + j) == (u32)tid) ? 1u : 0u;
        L.histAll[((size_t)k * L.nSeg + sgm) * 256 + tid] = c - cut + ((tid == 0) ? oo : 0u) - ((k + 1 < P) ? out : 0u);
    }
}

// prims::k_rs_digit_bases for the sort without the run members: the passes in front of the last one write compact segments (cbase), the
// last one the blocks' slots (base); the gap of every run group is preset to the end of its byte's slots (LastPassSrc::gapStart)
__global__ __launch_bounds__(256) void k_bwt_f_r0_bases(prims::RsLayout L, const u32* __restrict__ base, const u32* __restrict__ cbase, int P,
                                                        const u32* __restrict__ members, u32* __restrict__ gapStart)
{
    __shared__ u32 wsum[4];
    __shared__ u32 inclAll[256];
    const int sgm = blockIdx.x, ps = blockIdx.y;
    const int tid = (int)threadIdx.x;
    u32* h = L.histAll + ((size_t)ps * L.nSeg + sgm) * 256;
    const u32 c = h[tid];
    u32 tot;
    const u32 incl = prims::sc_block_incl<prims::SCAN_SUM_EXCL>(c, wsum, &tot);
    inclAll[tid] = incl;
    __syncthreads();
    const bool last = ps + 1 == P;
    const u32 b0 = last ? base[sgm] : cbase[sgm];
    h[tid] = b0 + (tid ? inclAll[tid - 1] : 0u);
    if (last) gapStart[(size_t)sgm * 256 + tid] = b0 + incl - members[(size_t)sgm * 256 + tid];
}

// The inside of a gap is left alone: only a gap's first slot is ever placed, every other slot of it starts no group, and what the flag
// and the placing kernel would learn from its keys is known from the gap's bounds (gapStart, members). k_bwt_f_r0_fill writes the
// class's key to the R0_GAP_MARGIN slots at either end of a gap (to all of a gap of up to two margins); a workgroup of k_bwt_f_r0_flags
// whose slots, and a window of k_bwt_f_r0_place_text whose view, lie strictly behind the first slot of one gap and in front of its end
// (r0_inside_gap) does its work without loading a key. What makes this safe: every slot a kernel reads without that test lies within
// the margin of a gap end, and is therefore filled -- a workgroup that fails the test starts at or in front of the gap's first slot, or
// ends behind the gap's last one, and reads no further than its 256 * R0F_ROWS slots (and the slot in front of them), or its SM_WIN.
// The two kernels are the only readers of round 0's sorted keys (FwdSort::keysFree2, scratch of the rounds afterwards).
constexpr u32 R0F_ROWS = 8;       // rows of 256 slots per workgroup of k_bwt_f_r0_flags
constexpr u32 R0_GAP_MARGIN = 2048;
static_assert(R0_GAP_MARGIN >= 256 * R0F_ROWS, "a workgroup of k_bwt_f_r0_flags that touches a gap's end must stay within the margin");
static_assert(R0_GAP_MARGIN >= SM_WIN, "a window of k_bwt_f_r0_place_text that touches a gap's end must stay within the margin");

// the n slots from a on lie strictly behind the first slot of the gap of (block b, byte c) and in front of its end
__device__ __forceinline__ bool r0_inside_gap(const u32* __restrict__ members, const u32* __restrict__ gapStart, int b, u32 c, u32 a, u32 n)
{
    const u32 m = members[(u32)b * 256u + c];
    if (m == 0u) return false;
    const u32 g0 = gapStart[(u32)b * 256u + c];
    return a > g0 && a - g0 < m && n <= m - (a - g0);
}

// the gaps filled: the class's key with the position of its first member in the slots at either end of the gap
__global__ __launch_bounds__(256) void k_bwt_f_r0_fill(u64* __restrict__ keys, const u32* __restrict__ members, const u32* __restrict__ gapStart,
                                                       const u32* __restrict__ firstPos, int P, int pbits)
{
    const u32 sgm = blockIdx.y, c = blockIdx.x;                          // (a workgroup per class: at most two margins to write)
    const u32 m = members[sgm * 256u + c];
    if (m == 0u) return;
    const u32 g0 = gapStart[sgm * 256u + c];
    const u64 key = (rep_key(c, P) << pbits) | (u64)firstPos[sgm * 256u + c];
    const bool whole = m <= 2u * R0_GAP_MARGIN;
    const u32 cnt = whole ? m : 2u * R0_GAP_MARGIN;
    for (u32 i = threadIdx.x; i < cnt; i += 256u) keys[g0 + ((whole || i < R0_GAP_MARGIN) ? i : m - 2u * R0_GAP_MARGIN + i)] = key;
}

// group-start flags of the sorted keys as a bit map (one ballot per wave): a slot starts a group when its key bytes differ from
// its left neighbour's, when it is the first slot of a block, or when it or its left neighbour is a short suffix.
// R0F_ROWS rows of 256 slots per workgroup, all loads of a thread in flight at once (one row per workgroup ran at 2.5 TB/s).
// members (null: no gaps): a workgroup inside a gap (one class per thread looks) writes its zero words and loads no key; nSkipped (null
// without the knob bwt_stats) counts those.
__global__ __launch_bounds__(256) void k_bwt_f_r0_flags(const u64* __restrict__ keys, const u32* __restrict__ base, int nBlocks, u32 total, int P, int pbits,
                                                        unsigned long long* __restrict__ gbits64, const u32* __restrict__ members, const u32* __restrict__ gapStart,
                                                        u32* __restrict__ nSkipped)
{
    __shared__ int sBlk;
    __shared__ u32 sInside;
    const u32 a0 = blockIdx.x * (256u * R0F_ROWS);
    if (threadIdx.x == 0) { sBlk = find_block(base, nBlocks, a0 < total ? a0 : (total ? total - 1 : 0)); sInside = 0; }
    __syncthreads();
    if (members != nullptr) {
        if (r0_inside_gap(members, gapStart, sBlk, threadIdx.x, a0, 256u * R0F_ROWS)) sInside = 1;
        __syncthreads();
        if (sInside) {
            if (threadIdx.x < 256u * R0F_ROWS / 64u) gbits64[(a0 >> 6) + threadIdx.x] = 0ull;
            if (nSkipped != nullptr && threadIdx.x == 0) atomicAdd(nSkipped, 1u);
            return;
        }
    }
    u64 kr[R0F_ROWS], kl[R0F_ROWS];
#pragma unroll
    for (u32 r = 0; r < R0F_ROWS; r++) {
        const u32 a = a0 + r * 256u + threadIdx.x;
        kr[r] = (a < total) ? keys[a] : 0ull;
        // the left neighbour's key comes from the lane next door (lane 0 of a wave loads it)
        kl[r] = ((threadIdx.x & 63) == 0 && a > 0 && a < total) ? keys[a - 1] : 0ull;
    }
    int b = sBlk;
    const u64 pm = (1ull << pbits) - 1ull;
#pragma unroll
    for (u32 r = 0; r < R0F_ROWS; r++) {
        const u32 a = a0 + r * 256u + threadIdx.x;
        if (a0 + r * 256u >= total) break;                  // (uniform)
        const u64 k = kr[r];
        const u32 klo = (u32)__shfl_up((int)(u32)k, 1u, 64), khi = (u32)__shfl_up((int)(u32)(k >> 32), 1u, 64);
        u64 kp = ((u64)khi << 32) | klo;
        if ((threadIdx.x & 63) == 0) kp = kl[r];
        bool f = true;
        if (a < total) {
            while (a >= base[b + 1]) b++;
            const u32 bb = base[b], n = base[b + 1] - bb;
            f = (a == bb) || ((k >> pbits) != (kp >> pbits)) || ((u32)(k & pm) + (u32)P > n) || ((u32)(kp & pm) + (u32)P > n);
        }
        const unsigned long long m = __ballot(f);
        if ((threadIdx.x & 63) == 0) gbits64[a >> 6] = m;
    }
}

// per window of wordsPerWin bit-map words: the last group start in it (0 when it has none: slot 0 always starts a group, so 0 is neutral
// for the running maximum) and, mirrored for a running minimum from the right, the first one (`total` when none)
__global__ __launch_bounds__(256) void k_bwt_f_r0_winsum(const u32* __restrict__ gbits, u32 total, u32 nWin, u32* __restrict__ winLast, u32* __restrict__ winFirstRev,
                                                         u32 wordsPerWin)
{
    const u32 w = blockIdx.x * 256 + threadIdx.x;
    if (w >= nWin) return;
    u32 last = 0, first = total;
    bool seen = false;
    for (u32 k = 0; k < wordsPerWin; k++) {
        const u32 x = gbits[w * wordsPerWin + k];
        if (x) {
            const u32 b0 = (w * wordsPerWin + k) * 32;
            if (!seen) { first = b0 + (u32)__ffs((int)x) - 1; seen = true; }
            last = b0 + 31 - (u32)__clz((int)x);
        }
    }
    winLast[w] = last < total ? last : (total ? total - 1 : 0);
    winFirstRev[nWin - 1 - w] = first < total ? first : total;
}

// ------------------------------------------------------------------------------------------------
// small groups: bit-map driven windows
// ------------------------------------------------------------------------------------------------
struct SmWindow {
    u32 bw[64];
    int prevSet[64];     // last set bit in the words before w (-1: none)
    u32 nextSet[64];     // first set bit in the words after w (NO_BIT: none)
};

// wave 0 of the workgroup loads the 64 bit-map words of the window and the two per-word summaries; returns false
// (to every thread) when no group that starts in the window is unresolved
__device__ __forceinline__ bool sm_load_window(const FwdView& v, u32 slot0, SmWindow& W, int* sAny)
{
    const int tid = (int)threadIdx.x;
    if (tid < 64) {
        const u32 w = v.gbits[(slot0 >> 5) + (u32)tid];
        W.bw[tid] = w;
        int last = w ? (tid * 32 + 31 - __clz((int)w)) : -1;
        u32 first = w ? (u32)(tid * 32 + __ffs((int)w) - 1) : NO_BIT;
        // exclusive prefix max / suffix min over the 64 words
        int pm = last;
        u32 sm = first;
        for (int o = 1; o < 64; o <<= 1) {
            const int t = __shfl_up(pm, o, 64);
            if (tid >= o) pm = t > pm ? t : pm;
            const u32 u = (u32)__shfl_down((int)sm, o, 64);
            if (tid + o < 64) sm = u < sm ? u : sm;
        }
        int pex = __shfl_up(pm, 1, 64);
        if (tid == 0) pex = -1;
        u32 sex = (u32)__shfl_down((int)sm, 1, 64);
        if (tid == 63) sex = NO_BIT;
        W.prevSet[tid] = pex;
        W.nextSet[tid] = sex;
        // anything to do? a zero bit among the owned slots, or right behind them (a group that starts at the last owned slot)
        const bool zero = (tid < (int)(SM_TS / 32)) ? (w != 0xFFFFFFFFu) : (tid == (int)(SM_TS / 32) ? ((w & 1u) == 0) : false);
        const unsigned long long anyz = __ballot(zero);
        if (tid == 0) *sAny = anyz != 0 ? 1 : 0;
    }
    __syncthreads();
    return *sAny != 0;
}

// group [s, e) of window element i; false when i is not a member of a small unresolved group owned by this window
__device__ __forceinline__ bool sm_group_of(const SmWindow& W, u32 i, u32& s, u32& e)
{
    const u32 w = i >> 5, bit = i & 31;
    const u32 lowmask = (bit == 31) ? 0xFFFFFFFFu : ((2u << bit) - 1u);
    const u32 word = W.bw[w];
    const u32 m = word & lowmask;
    int si = m ? (int)(w * 32 + 31 - __clz((int)m)) : W.prevSet[w];
    if (si < 0 || (u32)si >= SM_TS) return false;
    const u32 m2 = word & ~lowmask;
    const u32 ei = m2 ? (w * 32 + (u32)__ffs((int)m2) - 1) : W.nextSet[w];
    if (ei == NO_BIT) return false;
    const u32 len = ei - (u32)si;
    if (len < 2 || len > SM_G) return false;
    s = (u32)si; e = ei;
    return true;
}

// Round 0 and the text round in one sweep: SA, the labels and the descriptors of the groups that are not small. Windows of SM_TS owned
// slots that look SM_G slots further, as the small-group kernels do. The group of a slot starts at the last set bit at or before it:
// found in the window's bit-map words, else in the running maximum over the windows before it (winLastIncl); the length of a group
// (needed where it starts) ends at the next set bit. A slot is placed by the window that owns it -- except the members of a SMALL group
// (2..SM_G members), which are all placed by the window that owns the group's first slot: that window has their keys in LDS anyway,
// sorts them on the seven text bytes behind the round-0 symbols before anything is written, and writes position and label ONCE, with
// the label the text order gives. Most small groups of round 0 are resolved here and never enter a doubling round: a member pays one
// random read for seven symbols of depth where a doubling round at h = 4 buys four (a separate text round read SA back, and wrote SA
// and the labels of every member that moved a second time).
__global__ __launch_bounds__(256) void k_bwt_f_r0_place_text(BwtView bv, FwdView v, const u32* __restrict__ winLastIncl, const u32* __restrict__ winFirstInclRev, u32 nWin,
                                                             uint2* __restrict__ largeNext, const u64* __restrict__ keys, int nsym, int pbits, uint2* __restrict__ runList,
                                                             const u32* __restrict__ gapTab, const u32* __restrict__ gapMembers, const u32* __restrict__ gapStart)
{
    // gapTab (null: the run members went through the sort): [block][256], != 0xFFFFFFFF where the byte's run group is a gap that
    // k_bwt_f_r0_fill filled. Only its first slot is placed -- the run round writes position and label of every member. A window whose
    // whole view lies inside a gap (r0_inside_gap; gapMembers, gapStart) has nothing to place, list or count, and its keys are not there
    __shared__ SmWindow W;
    __shared__ int sBlk;
    __shared__ ClassAgg A;
    __shared__ u32 sSA[SM_WIN];
    __shared__ u64 sK[SM_WIN];
    __shared__ u32 sNew[64];
    __shared__ u32 sAfterLocal;           // first group start in the owned part of the NEXT window behind what this one looks at
    __shared__ u32 sInside;
    constexpr int E = (int)(SM_WIN / 256);
    constexpr u32 TSW = SM_TS / 32;       // words a window owns
    const int tid = (int)threadIdx.x;
    const u32 win = blockIdx.x;
    const u32 slot0 = win * SM_TS;
    if (gapTab != nullptr) {
        if (tid == 0) { sBlk = find_block(v.base, v.nBlocks, slot0 < v.total ? slot0 : v.total - 1); sInside = 0; }
        __syncthreads();
        if (r0_inside_gap(gapMembers, gapStart, sBlk, (u32)tid, slot0, SM_WIN)) sInside = 1;
        __syncthreads();
        if (sInside) return;
    } else if (tid == 0) sBlk = find_block(v.base, v.nBlocks, slot0 < v.total ? slot0 : v.total - 1);
    agg_init(A);
    if (tid < 64) {
        sNew[tid] = 0;
        const u32 w = v.gbits[(slot0 >> 5) + (u32)tid];
        W.bw[tid] = w;
        int pm = w ? (tid * 32 + 31 - __clz((int)w)) : -1;
        u32 sm = w ? (u32)(tid * 32 + __ffs((int)w) - 1) : NO_BIT;
        for (int o = 1; o < 64; o <<= 1) {
            const int t = __shfl_up(pm, (unsigned)o, 64);
            if (tid >= o) pm = t > pm ? t : pm;
            const u32 u = (u32)__shfl_down((int)sm, (unsigned)o, 64);
            if (tid + o < 64) sm = u < sm ? u : sm;
        }
        int pex = __shfl_up(pm, 1u, 64);
        if (tid == 0) pex = -1;
        u32 sex = (u32)__shfl_down((int)sm, 1u, 64);
        if (tid == 63) sex = NO_BIT;
        W.prevSet[tid] = pex;
        W.nextSet[tid] = sex;
    } else if (tid < 128) {
        // the rest of the next window's owned words (2 TSW - 64 of them): where a group that leaves this window's view ends, if it ends there
        const int k = tid - 64;
        const u32 w = (k < (int)(2 * TSW - 64)) ? v.gbits[(slot0 >> 5) + 64u + (u32)k] : 0u;
        const unsigned long long any = __ballot(w != 0);
        const int first = any ? __ffsll((long long)any) - 1 : 0;          // (this wave alone writes the word: lane 0 says "none")
        if (k == first) sAfterLocal = any ? SM_WIN + (u32)k * 32u + (u32)__ffs((int)w) - 1u : NO_BIT;
    }
    __syncthreads();
    const u32 before = win ? winLastIncl[win - 1] : 0u;
    u32 after = (sAfterLocal != NO_BIT) ? slot0 + sAfterLocal : ((win + 2 < nWin) ? winFirstInclRev[nWin - 3 - win] : v.total);
    if (after > v.total) after = v.total;
    const u64 pmask = (1ull << pbits) - 1ull;
    // ---- every slot in view: position, group, and -- for the members of small groups this window owns -- the text key
    u32 gp[E], gs[E], ge[E];
    u64 kk[E];
    bool inView[E], mine[E];              // mine: member of a small group whose first slot this window owns
    int blkOf[E];
#pragma unroll
    for (int k = 0; k < E; k++) {
        const u32 i = (u32)tid + 256u * (u32)k;
        const u32 a = slot0 + i;
        inView[k] = a < v.total;
        mine[k] = false; gp[k] = 0; kk[k] = 0; gs[k] = 0; ge[k] = 0; blkOf[k] = 0;
        if (!inView[k]) continue;
        int blk = sBlk;
        while (a >= v.base[blk + 1]) blk++;
        blkOf[k] = blk;
        kk[k] = keys[a];
        gp[k] = v.base[blk] + (u32)(kk[k] & pmask);
        mine[k] = sm_group_of(W, i, gs[k], ge[k]);
        if (mine[k]) {
            const u32 bb = v.base[blk], n = v.base[blk + 1] - bb;
            const u32 q = gp[k] - bb + (u32)nsym;
            const u8* t = bv.src[blk];
            const u64 x = text8(t, q, n);
            sSA[i] = gp[k];
            // (SEVEN text bytes and the member's place in its group below them: the key is unique inside the group, and one compare per
            // pair gives the stable rank, a second one against the key without the place the smaller keys alone -- see k_bwt_f_small_fused)
            sK[i] = (__builtin_bswap64(x) & ~0xFFull) | (u64)(i - gs[k]);
        }
    }
    __syncthreads();
    u32 surv = 0;
    int hKind[E];
    u32 hLocal[E], hSize[E];
#pragma unroll
    for (int k = 0; k < E; k++) {
        const u32 i = (u32)tid + 256u * (u32)k;
        const u32 a = slot0 + i;
        hKind[k] = -1; hLocal[k] = 0; hSize[k] = 0;
        if (!inView[k]) continue;
        if (mine[k]) {
            // a member of a small group of this window: its place and label come from the text order inside the group
            const u64 ki = sK[i], lo = ki & ~0xFFull;
            u32 less = 0, rank = 0;
            for (u32 j = gs[k]; j < ge[k]; j++) {
                const u64 kj = sK[j];
                rank += (kj < ki) ? 1u : 0u;
                less += (kj < lo) ? 1u : 0u;
            }
            const u32 eqBefore = rank - less;
            const u32 headIdx = gs[k] + less;
            v.SA[slot0 + headIdx + eqBefore] = gp[k];
            lab_set(v, gp[k], v.base[blkOf[k]], slot0 + headIdx, slot0 + headIdx);
            if (less != 0 && eqBefore == 0) atomicOr(&sNew[headIdx >> 5], 1u << (headIdx & 31));
            if (eqBefore != 0) surv = 1;
            continue;
        }
        if (i >= SM_TS) continue;                                  // in view only: the next window owns it
        // the group of the slot: starts at the last set bit at or before it
        const u32 w = i >> 5, bit = i & 31;
        const u32 lowmask = (bit == 31) ? 0xFFFFFFFFu : ((2u << bit) - 1u);
        const u32 word = W.bw[w];
        const u32 m = word & lowmask;
        const int si = m ? (int)(w * 32 + 31 - (u32)__clz((int)m)) : W.prevSet[w];
        const u32 hd = (si >= 0) ? slot0 + (u32)si : before;
        if (si < 0) {
            // the group began in front of this window. If it is a small one, the window in front places its members (this one included)
            const u32 m2 = word & ~lowmask;
            const u32 ei = m2 ? (w * 32 + (u32)__ffs((int)m2) - 1) : W.nextSet[w];
            const u32 endSlot = (ei != NO_BIT) ? slot0 + ei : after;
            if (endSlot - hd <= SM_G) continue;
        }
        if (gapTab != nullptr && hd != a) {
            // (the key bytes in registers decide for nearly every slot; the table is read for equal symbols only)
            const u64 bytes = kk[k] >> pbits;
            const u32 c = (u32)bytes & 255u;
            const int blk = blkOf[k];
            if (bytes == rep_key(c, nsym) && (u32)(kk[k] & pmask) + (u32)nsym <= v.base[blk + 1] - v.base[blk] && gapTab[(u32)blk * 256u + c] != 0xFFFFFFFFu) continue;
        }
        v.SA[a] = gp[k];
        lab_set(v, gp[k], v.base[blkOf[k]], hd, hd);
        if (hd == a) {
            const u32 m2 = word & ~lowmask;
            const u32 ei = m2 ? (w * 32 + (u32)__ffs((int)m2) - 1) : W.nextSet[w];
            u32 nxt = (ei != NO_BIT) ? slot0 + ei : after;
            if (nxt > v.total) nxt = v.total;
            const u32 size = nxt - a;
            if (size <= SM_G) continue;                            // (a singleton; small groups went the other way)
            bool runGroup = false;
            if (runList != nullptr) {
                const u64 bytes = kk[k] >> pbits;
                u64 rep = 0;
                for (int q = 0; q < nsym; q++) rep = (rep << 8) | (bytes & 0xFF);
                const int blk = blkOf[k];
                runGroup = ((u32)(kk[k] & pmask) + (u32)nsym <= v.base[blk + 1] - v.base[blk]) && bytes == rep;
            }
            hSize[k] = size;
            hKind[k] = agg_note(A, size, runGroup, surv, hLocal[k]);
        }
    }
    if (__ballot(surv != 0) != 0 && (tid & 63) == 0) v.counters[CNT_SMALL_LEFT] = 1;
    __syncthreads();
    if (tid == 0) agg_reserve(A, v);
    __syncthreads();
#pragma unroll
    for (int k = 0; k < E; k++)
        if (hKind[k] >= 0) agg_write(A, v, hKind[k], hLocal[k], slot0 + (u32)tid + 256u * (u32)k, hSize[k], largeNext, runList);
    if (tid < 64 && sNew[tid]) atomicOr(&v.gnew[(slot0 >> 5) + (u32)tid], sNew[tid]);
}

constexpr int SM_ROWS = (int)(SM_WIN / 256);       // window elements per thread: i = threadIdx.x + 256 k

// Fetch of one member of a small group: window element i (slot slot0 + i) of the group that starts at element s. b0 = block of the
// window's first slot, sRt = the window's words of rtbits. Gives the position gp, the block's first slot bb and the key of the round of
// offset h (gather_key at look_offset); counts the developer statistics (knob bwt_stats).
__device__ __forceinline__ u32 sm_fetch_key(const FwdView& v, u32 h, int b0, const u32* sRt, u32 slot0, u32 i, u32 s, int stats, u32& gp, u32& bb)
{
    const u32 slot = slot0 + i;
    int b = b0;
    while (slot >= v.base[b + 1]) b++;
    bb = v.base[b];
    const u32 off = look_offset(v, slot, h, (sRt[i >> 5] >> (i & 31)) & 1u);
    gp = v.SA[slot];
    const u32 key = gather_key(v, gp, off, bb, v.base[b + 1]);
    if (stats) { atomicAdd(&v.counters[CNT_STAT_SMALL], 1u); if (i == s) atomicAdd(&v.counters[CNT_STAT_SMALL_GROUPS], 1u); }
    return key;
}

// Rank and place of a window's small groups, positions in sSA and keys in sK (behind a barrier): every member act[k] of group
// [gs[k], ge[k]) counts the members with a smaller key and the equal ones in front of it, and goes to that place; a member that leaves the
// group's head gets the label of its subgroup's first slot (bb[k] = its block's first slot), the subgroup's first member sets the new
// group start. Members still tied are summed per wave (CNT_SMALL_LEFT) and per window (survTile, when not null).
// PACKED: a key in sK is (key << 8 | place in the group), unique inside the group, so that ONE compare per pair gives a member its stable
// rank (smaller keys + equal keys in front of it) and a second one against (key << 8) the smaller keys alone; the plain form needs
// "smaller", "equal" and "equal and in front" -- 9.4 vector instructions per pair against 4.
template <bool PACKED>
__device__ __forceinline__ void sm_rank_place(const FwdView& v, u32 slot0, const bool* act, const u32* gs, const u32* ge, const u32* bb,
                                              const u32* sSA, const u32* sK, u32* sNew, u32* sWs, u32* __restrict__ survTile)
{
    u32 surv = 0;
#pragma unroll
    for (int k = 0; k < SM_ROWS; k++) {
        if (!act[k]) continue;
        const u32 i = threadIdx.x + 256u * k;
        const u32 ki = sK[i];
        u32 less = 0, eqBefore = 0, tied = 0;
        if (PACKED) {
            const u32 lo = ki & ~0xFFu;
            u32 rank = 0;
            for (u32 j = gs[k]; j < ge[k]; j++) {
                const u32 kj = sK[j];
                rank += (kj < ki) ? 1u : 0u;
                less += (kj < lo) ? 1u : 0u;
            }
            eqBefore = rank - less;
            // (members that are still tied: in a subgroup of m equal keys m - 1 have an equal key in front of them, and exactly one of
            // those has exactly one)
            tied = (eqBefore != 0 ? 1u : 0u) + (eqBefore == 1 ? 1u : 0u);
        } else {
            u32 eq = 0;
            for (u32 j = gs[k]; j < ge[k]; j++) {
                const u32 kj = sK[j];
                less += (kj < ki) ? 1u : 0u;
                const u32 same = (kj == ki) ? 1u : 0u;
                eq += same;
                eqBefore += (j < i) ? same : 0u;
            }
            tied = (eq > 1) ? 1u : 0u;
        }
        const u32 gp = sSA[i];
        const u32 headIdx = gs[k] + less;
        v.SA[slot0 + headIdx + eqBefore] = gp;
        if (less != 0) {
            lab_set(v, gp, bb[k], slot0 + headIdx, slot0 + gs[k]);             // (a small group's label is its first slot)
            if (eqBefore == 0) atomicOr(&sNew[headIdx >> 5], 1u << (headIdx & 31));
        }
        surv += tied;
    }
    {
        // members that are still tied, per window (summed by a scan: the host decides by their number whether the next round looks for
        // links first; one counter for all windows would be an atomic per wave on one address)
        const u32 ws = wave_sum(surv);
        if ((threadIdx.x & 63) == 0) { sWs[threadIdx.x >> 6] = ws; if (ws) v.counters[CNT_SMALL_LEFT] = 1; }
    }
    __syncthreads();
    if (threadIdx.x == 0 && survTile) survTile[blockIdx.x] = sWs[0] + sWs[1] + sWs[2] + sWs[3];
    if (threadIdx.x < 64 && sNew[threadIdx.x]) atomicOr(&v.gnew[(slot0 >> 5) + threadIdx.x], sNew[threadIdx.x]);
}

__global__ __launch_bounds__(256) void k_bwt_f_gather_small(FwdView v, u32 h, int stats)
{
    __shared__ SmWindow W;
    __shared__ int sAny;
    __shared__ int sBlk;
    __shared__ u32 sRt[64];
    const u32 slot0 = blockIdx.x * SM_TS;
    if (threadIdx.x >= 64 && threadIdx.x < 128) sRt[threadIdx.x - 64] = v.rtbits ? v.rtbits[(slot0 >> 5) + threadIdx.x - 64] : 0u;
    if (!sm_load_window(v, slot0, W, &sAny)) return;
    if (threadIdx.x == 0) sBlk = find_block(v.base, v.nBlocks, slot0 < v.total ? slot0 : v.total - 1);
    __syncthreads();
    const int b0 = sBlk;
#pragma unroll
    for (int k = 0; k < SM_ROWS; k++) {
        const u32 i = threadIdx.x + 256u * k;
        u32 s, e, gp, bb;
        if (!sm_group_of(W, i, s, e)) continue;
        v.K[slot0 + i] = sm_fetch_key(v, h, b0, sRt, slot0, i, s, stats, gp, bb);
    }
}

// (plain labels only, keys from k_bwt_f_gather_small: versioned ones take k_bwt_f_small_fused)
__global__ __launch_bounds__(256) void k_bwt_f_sort_small(FwdView v, u32* __restrict__ survTile)
{
    __shared__ SmWindow W;
    __shared__ int sAny;
    __shared__ u32 sSA[SM_WIN];
    __shared__ u32 sK[SM_WIN];
    __shared__ u32 sNew[64];
    __shared__ u32 sWs[4];
    const u32 slot0 = blockIdx.x * SM_TS;
    if (!sm_load_window(v, slot0, W, &sAny)) { if (threadIdx.x == 0 && survTile) survTile[blockIdx.x] = 0; return; }
    if (threadIdx.x < 64) sNew[threadIdx.x] = 0;
    u32 gs[SM_ROWS], ge[SM_ROWS], bb[SM_ROWS];
    bool act[SM_ROWS];
#pragma unroll
    for (int k = 0; k < SM_ROWS; k++) {
        const u32 i = threadIdx.x + 256u * k;
        act[k] = sm_group_of(W, i, gs[k], ge[k]);
        bb[k] = 0;                                          // (plain labels need no block base)
        if (act[k]) { sSA[i] = v.SA[slot0 + i]; sK[i] = v.K[slot0 + i]; }
    }
    __syncthreads();
    sm_rank_place<false>(v, slot0, act, gs, ge, bb, sSA, sK, sNew, sWs, survTile);
}

// Keys and refinement of the small groups in ONE sweep (versioned labels, see lab_old): k_bwt_f_gather_small + k_bwt_f_sort_small without the
// key array in between -- a window's bit-map words, positions and keys are read once and stay in LDS (the two kernels read the bit map and
// SA twice and wrote and read K: 24 of the 40 KiB a dense window moved per round).
// PACKED (blocks of up to 8 MiB: a key -- a label inside the block + 1 -- has 24 bits): the keys are ranked in sm_rank_place's packed form; a
// member of a group of g compares with all g (round 6: groups of 33..256 members are a third of the small-group visits of the first rounds
// on real files).
template <bool PACKED>
__global__ __launch_bounds__(256) void k_bwt_f_small_fused(FwdView v, u32 h, u32* __restrict__ survTile, int stats)
{
    __shared__ SmWindow W;
    __shared__ int sAny;
    __shared__ int sBlk;
    __shared__ u32 sRt[64];
    __shared__ u32 sSA[SM_WIN];
    __shared__ u32 sK[SM_WIN];
    __shared__ u32 sNew[64];
    __shared__ u32 sWs[4];
    const u32 slot0 = blockIdx.x * SM_TS;
    if (threadIdx.x >= 64 && threadIdx.x < 128) sRt[threadIdx.x - 64] = v.rtbits ? v.rtbits[(slot0 >> 5) + threadIdx.x - 64] : 0u;
    if (!sm_load_window(v, slot0, W, &sAny)) { if (threadIdx.x == 0 && survTile) survTile[blockIdx.x] = 0; return; }
    if (threadIdx.x < 64) sNew[threadIdx.x] = 0;
    if (threadIdx.x == 64) sBlk = find_block(v.base, v.nBlocks, slot0 < v.total ? slot0 : v.total - 1);
    __syncthreads();
    const int b0 = sBlk;
    u32 gs[SM_ROWS], ge[SM_ROWS], bb[SM_ROWS];
    bool act[SM_ROWS];
#pragma unroll
    for (int k = 0; k < SM_ROWS; k++) {
        const u32 i = threadIdx.x + 256u * k;
        act[k] = sm_group_of(W, i, gs[k], ge[k]);
        bb[k] = 0;
        if (!act[k]) continue;
        u32 gp;
        const u32 key = sm_fetch_key(v, h, b0, sRt, slot0, i, gs[k], stats, gp, bb[k]);
        sSA[i] = gp;
        sK[i] = PACKED ? ((key << 8) | (i - gs[k])) : key;
    }
    __syncthreads();
    sm_rank_place<PACKED>(v, slot0, act, gs, ge, bb, sSA, sK, sNew, sWs, survTile);
}

// ------------------------------------------------------------------------------------------------
// small groups inside long repeats: the link step (round 5)
// ------------------------------------------------------------------------------------------------
// A repeat of length L is L tied groups {p + i, q + i, ...}, i = 0 .. L - 1, and prefix doubling visits each of them log2(L - i) times:
// real files (the same licence text in front of thousands of headers, string tables, duplicate objects) spend most of the suffix sort
// there. All those groups are ordered alike -- by what follows the repeat's end. A small group G is LINKED when the successors p + 1 of
// all its members lie in one group (which may hold other suffixes as well). Every member of a linked group is flagged at its own
// position in a bit map over the positions, so the groups of one repeat are runs of consecutive set bits, and a run's end -- the first
// position that is not flagged -- is c positions on, the same c for every member of G (they stay together all the way): the members of
// G share c symbols more than their depth says, and the group at the run's end is what tells them apart. The existing "look max(R, h)
// positions on" of the key kernels (FwdView::ovr, rtbits) does the rest: ovr = c + h for the members of G, and G is sorted in this
// round by the labels c + h positions on -- together with the group at the end of its run, instead of log2 c rounds later. Exact: a
// link means the successors are in ONE group, i.e. equal in at least their first symbol; c links in a row mean c equal symbols, and the
// group at the end has depth h. Only groups whose positions lie below posEnd take part (0: below the end of the first block -- the trial
// of the host policy covers that block only, and its bit map ends there: the window of the next block that rides along must neither
// flag nor look up anything).
// a trial looks at up to four whole blocks of the batch (a run never leaves its block, so the blocks' runs are complete)
struct LinkTrial { int n; int blk[4]; };

__device__ __forceinline__ bool link_tile(const FwdView& v, const LinkTrial& tr, u32 tileStep, u32& tile, u32& posLo, u32& posHi)
{
    if (tr.n == 0) { tile = blockIdx.x * tileStep; posLo = 0; posHi = v.total; return true; }
    const int b = tr.blk[blockIdx.y];
    posLo = v.base[b]; posHi = v.base[b + 1];
    tile = posLo / SM_TS + blockIdx.x;                        // (the window that holds the block's first slot, and the ones behind it)
    return tile * SM_TS < posHi;
}

__global__ __launch_bounds__(256) void k_bwt_f_link_small(FwdView v, u32* __restrict__ posflag, u32* __restrict__ linked, int stats, u32 tileStep,
                                                          u32* __restrict__ linkedTile, LinkTrial tr)
{
    __shared__ SmWindow W;
    __shared__ int sAny;
    __shared__ int sBlk;
    __shared__ u32 sP[SM_WIN];
    __shared__ u32 sK[SM_WIN];
    __shared__ u32 sLinked[64];
    __shared__ u32 sCnt[4];
    u32 tile, posLo, posHi;
    if (!link_tile(v, tr, tileStep, tile, posLo, posHi)) return;
    const u32 slot0 = tile * SM_TS;
    if (!sm_load_window(v, slot0, W, &sAny)) { if (threadIdx.x == 0) linkedTile[tile] = 0; return; }
    if (threadIdx.x < 64) sLinked[threadIdx.x] = 0;
    if (threadIdx.x == 64) sBlk = find_block(v.base, v.nBlocks, slot0 < v.total ? slot0 : v.total - 1);
    __syncthreads();
    const int b0 = sBlk;
    u32 gs[SM_WIN / 256], ge[SM_WIN / 256];
    bool act[SM_WIN / 256];
#pragma unroll
    for (int k = 0; k < (int)(SM_WIN / 256); k++) {
        const u32 i = threadIdx.x + 256u * k;
        act[k] = sm_group_of(W, i, gs[k], ge[k]);
        if (!act[k]) continue;
        const u32 slot = slot0 + i;
        int b = b0;
        while (slot >= v.base[b + 1]) b++;
        const u32 gp = v.SA[slot];
        sP[i] = gp;
        sK[i] = (gp + 1 < v.base[b + 1]) ? lab_old(v, gp + 1, v.base[b]) : 0xFFFFFFFFu;      // the label of the successor; none at the block's end
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < (int)(SM_WIN / 256); k++) {
        const u32 i = threadIdx.x + 256u * k;
        if (!act[k] || i != gs[k]) continue;
        const u32 lab = sK[i];
        bool ok = lab != 0xFFFFFFFFu && sP[i] >= posLo && sP[i] < posHi;         // (one group, one block: its first member speaks for all)
        for (u32 j = gs[k] + 1; j < ge[k] && ok; j++) ok = sK[j] == lab;
        if (ok) atomicOr(&sLinked[i >> 5], 1u << (i & 31));
    }
    __syncthreads();
    u32 mine = 0;
    // every member of a linked group is flagged at its own position: the group one position on may hold other suffixes as well (they do
    // not matter: what counts is that THESE members stay together), so a run is followed member by member, not group by group
#pragma unroll
    for (int k = 0; k < (int)(SM_WIN / 256); k++) {
        if (!act[k]) continue;
        if (!((sLinked[gs[k] >> 5] >> (gs[k] & 31)) & 1u)) continue;
        const u32 gp = sP[threadIdx.x + 256u * k];
        atomicOr(&posflag[gp >> 5], 1u << (gp & 31));
        mine++;
    }
    (void)stats;
    {
        const u32 ws = wave_sum(mine);
        if ((threadIdx.x & 63) == 0) sCnt[threadIdx.x >> 6] = ws;
    }
    __syncthreads();
    if (threadIdx.x == 0) linkedTile[tile] = sCnt[0] + sCnt[1] + sCnt[2] + sCnt[3];       // members in linked groups: what the step may pay for
    if (threadIdx.x < 64 && sLinked[threadIdx.x]) atomicOr(&linked[(slot0 >> 5) + threadIdx.x], sLinked[threadIdx.x]);
}

// what the link step bought: members it linked against members still tied after the round, over the windows it was applied to. A trial
// on sample blocks pays when it pays in EVERY one of them (a batch of different files: the first block of the real-file corpus is one
// shared object whose groups are whole repeats, the header files behind it are not -- applied to the whole batch the step cost 3.5 ms
// there and bought 1.7): a block that does not pay is reported as "everything still tied".
__global__ __launch_bounds__(256) void k_bwt_f_link_payoff(FwdView v, const u32* __restrict__ linkedTile, const u32* __restrict__ survTile, u32 nTiles, u32 tileStep,
                                                           u32* __restrict__ out, LinkTrial tr)
{
    __shared__ u32 sA[256], sB[256];
    u32 totA = 0, totB = 0;
    bool every = true;
    const int nPart = tr.n ? tr.n : 1;
    for (int q = 0; q < nPart; q++) {
        u32 t0 = 0, t1 = nTiles, step = tileStep;
        if (tr.n) { t0 = v.base[tr.blk[q]] / SM_TS; t1 = (v.base[tr.blk[q] + 1] + SM_TS - 1) / SM_TS; step = 1; if (t1 > nTiles) t1 = nTiles; }
        u32 a = 0, b = 0;
        for (u32 t = t0 + threadIdx.x * step; t < t1; t += 256u * step) { a += linkedTile[t]; b += survTile[t]; }
        sA[threadIdx.x] = a; sB[threadIdx.x] = b;
        __syncthreads();
        for (int o = 128; o > 0; o >>= 1) { if ((int)threadIdx.x < o) { sA[threadIdx.x] += sA[threadIdx.x + o]; sB[threadIdx.x] += sB[threadIdx.x + o]; } __syncthreads(); }
        totA += sA[0]; totB += sB[0];
        if (tr.n && !(sA[0] >= 1024u && sB[0] < sA[0] / 2)) every = false;
        __syncthreads();
    }
    if (threadIdx.x == 0) { out[0] = totA; out[1] = every ? totB : (totA > totB ? totA : totB); }
}

// first zero bit of every word of the link bit map, by word, in reversed order (an inclusive minimum scan over it gives, for every word,
// the first zero bit at or behind it)
__global__ __launch_bounds__(256) void k_bwt_f_link_zeros(const u32* __restrict__ posflag, u32 nW, u32* __restrict__ rev)
{
    const u32 w = blockIdx.x * 256 + threadIdx.x;
    if (w >= nW) return;
    const u32 x = ~posflag[w];
    rev[nW - 1 - w] = x ? 32u * w + (u32)__ffs((int)x) - 1u : 0xFFFFFFFFu;
}

__device__ __forceinline__ u32 link_next_zero(const u32* __restrict__ posflag, const u32* __restrict__ sufRev, u32 nW, u32 p)
{
    const u32 w = p >> 5;
    const u32 x = ~posflag[w] & (0xFFFFFFFFu << (p & 31));
    if (x) return 32u * w + (u32)__ffs((int)x) - 1u;
    return (w + 1 < nW) ? sufRev[nW - 2 - w] : 0xFFFFFFFFu;
}

__global__ __launch_bounds__(256) void k_bwt_f_link_apply(FwdView v, const u32* __restrict__ posflag, const u32* __restrict__ sufRev, u32 nW,
                                                          const u32* __restrict__ linked, u32 h, u32* __restrict__ ovr, u32* __restrict__ rtbits, u32 tileStep, LinkTrial tr)
{
    __shared__ SmWindow W;
    __shared__ int sAny;
    __shared__ u32 sLinked[64];
    __shared__ u32 sRt[64];
    __shared__ u32 sOff[SM_WIN];
    u32 tile, posLo, posHi;
    if (!link_tile(v, tr, tileStep, tile, posLo, posHi)) return;
    const u32 slot0 = tile * SM_TS;
    if (threadIdx.x >= 64 && threadIdx.x < 128) { sLinked[threadIdx.x - 64] = linked[(slot0 >> 5) + threadIdx.x - 64]; sRt[threadIdx.x - 64] = 0; }
    if (!sm_load_window(v, slot0, W, &sAny)) return;
    __syncthreads();
    u32 gs[SM_WIN / 256], ge[SM_WIN / 256];
    bool act[SM_WIN / 256];
#pragma unroll
    for (int k = 0; k < (int)(SM_WIN / 256); k++) {
        const u32 i = threadIdx.x + 256u * k;
        act[k] = sm_group_of(W, i, gs[k], ge[k]) && ((sLinked[gs[k] >> 5] >> (gs[k] & 31)) & 1u);
        if (act[k] && i == gs[k]) {
            const u32 gp = v.SA[slot0 + i];                                      // (any member: the run is as long for all of them)
            const u32 e = link_next_zero(posflag, sufRev, nW, gp);
            sOff[i] = (e != 0xFFFFFFFFu && e > gp) ? (e - gp) + h : 0u;
        }
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < (int)(SM_WIN / 256); k++) {
        if (!act[k]) continue;
        const u32 i = threadIdx.x + 256u * k;
        const u32 off = sOff[gs[k]];
        if (off == 0) continue;
        const u32 slot = slot0 + i;
        const bool had = (rtbits[slot >> 5] >> (slot & 31)) & 1u;
        const u32 old = had ? ovr[slot] : 0u;
        if (off > old) ovr[slot] = off;
        if (!had) atomicOr(&sRt[i >> 5], 1u << (i & 31));
    }
    __syncthreads();
    if (threadIdx.x < 64 && sRt[threadIdx.x]) atomicOr(&rtbits[(slot0 >> 5) + threadIdx.x], sRt[threadIdx.x]);
}

// ------------------------------------------------------------------------------------------------
// medium groups: one workgroup per descriptor
// ------------------------------------------------------------------------------------------------
// The descriptors arrive sorted by start slot: neighbours in the list are neighbouring groups, and in periodic data (the
// members of group v+1 are the members of group v moved by one position) their members look at neighbouring words of ISA.
// The 32 workgroups that run on one XCD (workgroup index mod 8 -- an observed placement, used for speed only) walk through one
// contiguous eighth of the list side by side, so that a line of ISA fetched for one group is found in that XCD's L2 by the
// 31 groups next to it, instead of being fetched from memory once per group.
// A group whose members all carry ONE key cannot be split by the round (every member looks at the same group `off` positions on: the inside
// of a periodic stretch, of a table, of records with a shared prefix, until the offset reaches past an end). The whole group is held in
// registers (up to GATHER_ROWS members per thread: MED_CAP of them per workgroup), so the kernel sees that before it has stored a key: it
// then stores none, stages the group for the next round's list as med_write_back would have, and makes this round's descriptor void
// (length 0, like a group k_bwt_f_probe took apart): no sorting workgroup looks at the group -- SA, labels (an entry the round did not
// write reads as "unchanged") and the bit map already say what it would write. `skip` == 0 (knob bwt_no_unsplit_skip): every group is
// stored and sorted.
// The keys of the group's first ROWS * GATHER_THREADS members (all of them when `judge`): all position loads, then all key loads, then the
// stores -- two memory latencies per batch instead of two per member. judge: true comes back, and nothing is stored, when no key differs
// from key0, the first member's. ROWS fits the group (the real files' medium groups have some 800 members, a stretch's thousands).
template <int ROWS>
__device__ __forceinline__ bool gather_rows(const FwdView& v, u32 gs, u32 n, u32 off, u32 bb, u32 be, bool judge, u32 key0, u32* sDiff)
{
    u32 gp[ROWS], key[ROWS];
#pragma unroll
    for (int k = 0; k < ROWS; k++) { const u32 i = (u32)k * GATHER_THREADS + threadIdx.x; gp[k] = (i < n) ? v.SA[gs + i] : bb; }
#pragma unroll
    for (int k = 0; k < ROWS; k++) { const u32 i = (u32)k * GATHER_THREADS + threadIdx.x; key[k] = (i < n) ? gather_key(v, gp[k], off, bb, be) : key0; }
    if (judge) {                                            // (uniform)
        bool diff = false;
#pragma unroll
        for (int k = 0; k < ROWS; k++) diff = diff || key[k] != key0;       // (a slot behind the group's end holds key0)
        if (__ballot(diff) != 0 && (threadIdx.x & 63) == 0) *sDiff = 1;
        __syncthreads();
        if (*sDiff == 0) return true;
    }
#pragma unroll
    for (int k = 0; k < ROWS; k++) { const u32 i = (u32)k * GATHER_THREADS + threadIdx.x; if (i < n) v.K[gs + i] = key[k]; }
    return false;
}

__global__ __launch_bounds__(GATHER_THREADS) void k_bwt_f_gather_desc(FwdView v, uint2* __restrict__ desc, u32 nDesc, u32 h, uint2* __restrict__ descInfo, int stats, int skip)
{
    __shared__ int sBlk;
    __shared__ u32 sDiff;
    const u32 xcd = blockIdx.x & 7, lanesPerXcd = gridDim.x >> 3, slot = blockIdx.x >> 3;      // the grid is a multiple of 8 workgroups
    const u32 per = (nDesc + 7) / 8;
    const u32 lo = xcd * per, hi = (lo + per < nDesc) ? lo + per : nDesc;
    for (u32 g = lo + slot; g < hi; g += lanesPerXcd) {
        const uint2 d = desc[g];
        if (d.y == 0) continue;                             // (uniform) void: taken apart by the probe, or asleep (k_bwt_f_med_sleep)
        if (threadIdx.x == 0) { sBlk = find_block(v.base, v.nBlocks, d.x); sDiff = 0; }
        __syncthreads();
        const u32 bb = v.base[sBlk], be = v.base[sBlk + 1];
        const u32 off = look_offset(v, d.x, h);             // (uniform for the group)
        // the first member's label and key, by every thread for itself (one address for the workgroup, in flight beside the loads below)
        const u32 gp0 = v.SA[d.x];
        const u32 lab = lab_old(v, gp0, bb), key0 = gather_key(v, gp0, off, bb, be);
        // a verdict needs the group whole; the label inside the group's range and more than SM_G members: what med_write_back's
        // "label unchanged, staged again" rests on (true of every group the rounds make; anything else is stored and sorted)
        const bool judge = skip && d.y > SM_G && d.y <= GATHER_ROWS * (u32)GATHER_THREADS && lab - d.x < d.y;
        bool unsplit = false;
        if (d.y <= 1 * GATHER_THREADS) unsplit = gather_rows<1>(v, d.x, d.y, off, bb, be, judge, key0, &sDiff);
        else if (d.y <= 2 * GATHER_THREADS) unsplit = gather_rows<2>(v, d.x, d.y, off, bb, be, judge, key0, &sDiff);
        else if (d.y <= 4 * GATHER_THREADS) unsplit = gather_rows<4>(v, d.x, d.y, off, bb, be, judge, key0, &sDiff);
        else if (d.y <= 8 * GATHER_THREADS) unsplit = gather_rows<8>(v, d.x, d.y, off, bb, be, judge, key0, &sDiff);
        else for (u32 i0 = 0; i0 < d.y; i0 += GATHER_ROWS * GATHER_THREADS)                       // (once for a medium group)
            unsplit = gather_rows<(int)GATHER_ROWS>(v, d.x + i0, d.y - i0, off, bb, be, judge, key0, &sDiff);
        // (block base, label the members carry): what the sorting kernel needs per group without a chain of dependent loads of its own
        if (threadIdx.x == 0) {
            descInfo[g] = make_uint2(bb, lab);
            if (stats) { atomicAdd(&v.counters[CNT_STAT_MED], d.y); atomicAdd(&v.counters[CNT_STAT_MED_GROUPS], 1u); }
            if (unsplit) { desc[g] = make_uint2(d.x, 0u); med_leave_whole(v, d, key0, off, h, stats); }       // (every thread has read desc[g] in front of the verdict's barrier)
        }
        __syncthreads();
    }
}

// Medium groups that sleep through a round: the verdict is known from the round before without a member being read. Write T(G) for the
// group all members of G found h positions on in the round of offset h ("all keys equal"). When, in that round, G' = T(G) was itself left
// whole on one key, G'' = T(G'), and G'' came out of the round whole, then in this round (offset 2h) every member m of G has m + h in G',
// so m + 2h in G'', and G'' still carries its label: all keys of G are equal again and T(G) is now G''. One thread per descriptor looks
// that up -- the list is in slot order and a label is a slot inside its group's range, so a binary search finds the group of a label --
// and then does for G what k_bwt_f_gather_desc does on such a verdict: stages it for the next round, voids this round's descriptor (the
// gather passes a void one by without a load), records the new target. The rule composes, so a group can sleep round after round; it
// holds for any period, for tables and for records with a shared prefix. Anything else is gathered as before: an offset that is not the
// plain h (run tie, link step), for G now or for G or G' then; a past-the-end key; a target that is small, large, split or relabelled (it
// has no record of the round before); a target that is G itself (no finite group is all-equal on itself: a guard only, the chain round's
// groups have a majority, not all, that looks at the group and are never recorded).
// The records read are the round before's, the ones written this round's (FwdView::verdictWas / verdictNow): no thread sees its target's
// new state. Another thread may void the descriptor a search reads: the start stays, and sizes come from the records.
__device__ __forceinline__ bool sleep_target(const FwdView& v, const uint2* __restrict__ desc, u32 nDesc, u32 lab, u32 bb, bool plain, u32& start, u32& key)
{
    u32 lo = 0, hi = nDesc;                                 // first descriptor that starts behind the label
    while (lo < hi) { const u32 mid = (lo + hi) >> 1; if (desc[mid].x <= lab) lo = mid + 1; else hi = mid; }
    if (lo == 0) return false;
    start = desc[lo - 1].x;
    const uint2 t = v.verdictWas[start >> 8];
    const u32 status = (t.y >> 16) & 3u;
    if ((t.y >> 24) != v.round - 1u || (plain ? status != VERDICT_PLAIN : status == 0u) || lab - start >= (t.y & 0xFFFFu)) return false;
    key = t.x;
    return lab_old(v, v.SA[start], bb) == lab;              // the group of that range does carry the label
}

__global__ __launch_bounds__(256) void k_bwt_f_med_sleep(FwdView v, uint2* __restrict__ desc, u32 nDesc, int stats)
{
    const u32 g = blockIdx.x * 256 + threadIdx.x;
    if (g >= nDesc) return;
    const uint2 d = desc[g];
    if (d.y <= SM_G || d.y > MED_CAP) return;
    const uint2 was = v.verdictWas[d.x >> 8];
    if (was.y != verdict_word(v.round - 1u, VERDICT_PLAIN, d.y)) return;
    if (look_marked(v, d.x)) return;                        // (an offset of its own, not the plain h)
    const u32 bb = v.base[find_block(v.base, v.nBlocks, d.x)];
    u32 s1, k1, s2, k2;
    if (!sleep_target(v, desc, nDesc, bb + was.x - 1u, bb, true, s1, k1) || s1 == d.x) return;
    if (!sleep_target(v, desc, nDesc, bb + k1 - 1u, bb, false, s2, k2) || s2 == d.x) return;
    v.verdictNow[d.x >> 8] = make_uint2(k1, verdict_word(v.round, VERDICT_PLAIN, d.y));
    v.medStage[d.x >> 8] = d;
    desc[g] = make_uint2(d.x, 0u);
    if (stats) {
        atomicAdd(&v.counters[CNT_STAT_MED], d.y); atomicAdd(&v.counters[CNT_STAT_MED_GROUPS], 1u);
        atomicAdd(&v.counters[CNT_STAT_UNSPLIT], 1u); atomicAdd(&v.counters[CNT_STAT_UNSPLIT_MEMBERS], d.y);
        atomicAdd(&v.counters[CNT_STAT_ASLEEP], 1u); atomicAdd(&v.counters[CNT_STAT_ASLEEP_MEMBERS], d.y);
    }
}

// threadIdx.x as a value the optimiser cannot trace to threadIdx.x: nothing computed from it is merged with, or hoisted to, code outside
// the function that asks for it (no instruction is emitted)
__device__ __forceinline__ int local_tid()
{
    int t = (int)threadIdx.x;
#if defined(__HIP_DEVICE_COMPILE__) && !defined(KNZ_EMU)
    asm volatile("" : "+v"(t));
#endif
    return t;
}

// LDS of one sorting workgroup of THREADS threads: up to ROWS elements per thread
template <int THREADS, int ROWS>
struct MedLds {
    static constexpr int WAVES = THREADS / 64;
    static constexpr u32 CAP = (u32)ROWS * THREADS;
    u32 oK[CAP];
    u32 oV[CAP];
    u32 cnt[WAVES * 256];
    u32 fb[CAP / 32];
    int pm[CAP / 32];
    u32 pn[CAP / 32];
    u32 wtot[WAVES];
    u32 wtot2[WAVES];
    u32 oldLab;                 // the label the group's members carry
    u32 blkBase;                // first slot of the group's block (labels are stored relative to it: lab_set)
};

template <int THREADS, int ROWS>
__device__ __forceinline__ u32 med_block_sum(MedLds<THREADS, ROWS>& L, u32 x)
{
    const u32 s = wave_sum(x);
    if ((threadIdx.x & 63) == 0) L.wtot[threadIdx.x >> 6] = s;
    __syncthreads();
    u32 tot = 0;
    for (int w = 0; w < THREADS / 64; w++) tot += L.wtot[w];
    __syncthreads();
    return tot;
}

// Stable LSD radix sort of the pairs (oK, oV)[0, n) in LDS, 8-bit digits. Wave w owns the R*64 consecutive elements from
// w*R*64 (R = rows of 64 per wave); the rank of an element among the elements of its wave with the same digit comes from
// ballot matching (the lanes of a row that agree on all 8 digit bits), rows in order; per-wave digit counters are then
// scanned in (digit, wave) order. Entered and left with the workgroup in step.
template <int THREADS, int ROWS>
__device__ __forceinline__ void med_radix_sort(MedLds<THREADS, ROWS>& L, u32 n, int npass)
{
    constexpr int WAVES = THREADS / 64;
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const unsigned long long ltMask = (lane == 0) ? 0ull : (~0ull >> (64 - lane));
    u32* cntw = L.cnt + wave * 256;
    const int R = (int)((n + THREADS - 1) / THREADS);
    const u32 waveBase = (u32)wave * (u32)R * 64u;
    for (int pass = 0; pass < npass; pass++) {
        const int shift = 8 * pass;
        for (int q = lane; q < 256; q += 64) cntw[q] = 0;
        u32 key[ROWS], val[ROWS], pre[ROWS];
#pragma unroll
        for (int r = 0; r < ROWS; r++) {
            key[r] = 0xFFFFFFFFu; val[r] = 0; pre[r] = 0;
            if (r < R) {
                const u32 idx = waveBase + (u32)r * 64u + (u32)lane;
                if (idx < n) { key[r] = L.oK[idx]; val[r] = L.oV[idx]; }
                const u32 dg = (key[r] >> shift) & 255u;
                const unsigned long long peers = prims::digit_peers_fast(true, dg);
                const u32 pop = (u32)__popcll(peers);
                const u32 rnk = (u32)__popcll(peers & ltMask);
                const int leader = __ffsll((long long)peers) - 1;
                u32 old = 0;
                if (lane == leader) { old = cntw[dg]; cntw[dg] = old + pop; }
                old = (u32)__shfl((int)old, leader, 64);
                pre[r] = old + rnk;
            }
        }
        __syncthreads();
        // exclusive scan of the counters in (digit, wave) order: a thread owns one digit and four consecutive waves
        {
            constexpr int TPD = THREADS / 256;
            const int dg = tid / TPD, w0 = (tid % TPD) * 4;
            const u32 c0 = L.cnt[(w0 + 0) * 256 + dg], c1 = L.cnt[(w0 + 1) * 256 + dg], c2 = L.cnt[(w0 + 2) * 256 + dg], c3 = L.cnt[(w0 + 3) * 256 + dg];
            const u32 sum = c0 + c1 + c2 + c3;
            const u32 incl = wave_incl_scan(sum);
            if (lane == 63) L.wtot[wave] = incl;
            __syncthreads();
            u32 wbase = 0;
            for (int w = 0; w < wave; w++) wbase += L.wtot[w];
            const u32 excl = wbase + incl - sum;
            L.cnt[(w0 + 0) * 256 + dg] = excl;
            L.cnt[(w0 + 1) * 256 + dg] = excl + c0;
            L.cnt[(w0 + 2) * 256 + dg] = excl + c0 + c1;
            L.cnt[(w0 + 3) * 256 + dg] = excl + c0 + c1 + c2;
        }
        __syncthreads();
#pragma unroll
        for (int r = 0; r < ROWS; r++) {
            if (r < R) {
                const u32 dg = (key[r] >> shift) & 255u;
                const u32 pos = cntw[dg] + pre[r];
                if (pos < n) {                         // the padding of the last row sorts behind everything: not stored
                    L.oK[pos] = key[r];
                    L.oV[pos] = val[r];
                }
            }
        }
        __syncthreads();
    }
    (void)WAVES;
}

// Write-back of a group sorted in LDS (oK = keys in order, oV = positions): subgroup boundaries, SA, labels, the round's bit map
// and the children's descriptors. Entered and left with the workgroup in step.
template <int THREADS, int ROWS>
__device__ __forceinline__ void med_write_back(MedLds<THREADS, ROWS>& L, const FwdView& v, u32 gs, u32 n, uint2* __restrict__ medNext, uint2* __restrict__ largeNext)
{
    constexpr u32 CAP = (u32)ROWS * THREADS;
    // (the thread's index, hidden from the optimiser: what it derives from it per row here -- word, bit, masks, slots -- is then computed
    // where it is used. Otherwise all of it is hoisted out of the caller's loop over the groups and lives in registers through every other
    // phase of that loop: k_bwt_f_medium_fused<512, 16> spilled 92 B per lane for it, and <256, 8> began to once the chain round ran there)
    const int tid = local_tid(), lane = tid & 63;
    // ---- subgroup boundaries of the sorted keys as a bit map in LDS + per-word summaries
    const int nWords = (int)((n + 31) >> 5);
    if (tid < (int)(CAP / 32)) {
        u32 bits = 0;
        if (tid < nWords) {
            const u32 i0 = (u32)tid * 32u;
            u32 prev = (i0 == 0) ? 0u : L.oK[i0 - 1];
            for (u32 k = 0; k < 32; k++) {
                const u32 i = i0 + k;
                if (i >= n) break;
                const u32 cur = L.oK[i];
                if (i == 0 || cur != prev) bits |= 1u << k;
                prev = cur;
            }
        }
        L.fb[tid] = bits;
        L.pm[tid] = bits ? (tid * 32 + 31 - __clz((int)bits)) : -1;
        L.pn[tid] = bits ? (u32)(tid * 32 + __ffs((int)bits) - 1) : n;
    }
    __syncthreads();
    // inclusive prefix max of pm / suffix min of pn over the words, by the first wave (WPL consecutive words per lane)
    if (tid < 64) {
        constexpr int WPL = (int)(CAP / 32) / 64;
        int run = -1;
        for (int k = 0; k < WPL; k++) { const int x = L.pm[tid * WPL + k]; run = x > run ? x : run; }
        int incl = run;
        for (int o = 1; o < 64; o <<= 1) { const int t = __shfl_up(incl, (unsigned)o, 64); if (tid >= o) incl = t > incl ? t : incl; }
        int carry = __shfl_up(incl, 1u, 64);
        if (tid == 0) carry = -1;
        for (int k = 0; k < WPL; k++) { const int x = L.pm[tid * WPL + k]; carry = x > carry ? x : carry; L.pm[tid * WPL + k] = carry; }
        u32 runn = n;
        for (int k = WPL - 1; k >= 0; k--) { const u32 x = L.pn[tid * WPL + k]; runn = x < runn ? x : runn; }
        u32 incn = runn;
        for (int o = 1; o < 64; o <<= 1) { const u32 t = (u32)__shfl_down((int)incn, (unsigned)o, 64); if (tid + o < 64) incn = t < incn ? t : incn; }
        u32 carn = (u32)__shfl_down((int)incn, 1u, 64);
        if (tid == 63) carn = n;
        for (int k = WPL - 1; k >= 0; k--) { const u32 x = L.pn[tid * WPL + k]; carn = x < carn ? x : carn; L.pn[tid * WPL + k] = carn; }
    }
    __syncthreads();
    // pm[w] = last boundary at or before the end of word w, pn[w] = first boundary at or after the start of word w
    u32 surv = 0;
    const u32 oldLab = L.oldLab;
    __shared__ ClassAgg A;
    agg_init(A);
    __syncthreads();
    int hKind[ROWS];
    u32 hLocal[ROWS], hSize[ROWS];
#pragma unroll
    for (int r = 0; r < ROWS; r++) hKind[r] = -1;
    int row = 0;
    for (u32 i = (u32)tid; i < n; i += THREADS, row++) {
        const u32 w = i >> 5, bit = i & 31;
        const u32 lowmask = (bit == 31) ? 0xFFFFFFFFu : ((2u << bit) - 1u);
        const u32 word = L.fb[w];
        const u32 mm = word & lowmask;
        const u32 hd = mm ? (w * 32 + 31 - (u32)__clz((int)mm)) : (u32)L.pm[w - 1];      // word 0 always has bit 0
        const u32 gp = L.oV[i];
        v.SA[gs + i] = gp;
        const u32 m2 = word & ~lowmask;
        const u32 e = m2 ? (w * 32 + (u32)__ffs((int)m2) - 1) : ((w + 1 < (u32)(CAP / 32)) ? L.pn[w + 1] : n);     // end of my subgroup
        // The label of a group only has to be a slot inside the group's range (ranges are disjoint, so labels stay unique and
        // ordered). Small children take their first slot, as every kernel that works on small groups expects; a larger child
        // keeps the parent's label when that slot lies inside its range, else it takes its middle slot -- which the part that
        // holds the majority in the rounds to come will still contain, so that its thousands of members are not relabelled
        // (a scattered 4-byte store each) round after round just because a few members left in front of them.
        const u32 size = e - hd;
        const u32 rel = oldLab - gs;
        const u32 lab = (size <= SM_G) ? gs + hd : ((rel >= hd && rel < e) ? oldLab : gs + hd + (size >> 1));
        if (lab != oldLab) lab_set(v, gp, L.blkBase, lab, oldLab);
        if (hd == i) {
#pragma unroll
            for (int r = 0; r < ROWS; r++) if (r == row) { hSize[r] = size; hKind[r] = agg_note(A, size, false, surv, hLocal[r]); }
        }
    }
    if (__ballot(surv != 0) != 0 && lane == 0) v.counters[CNT_SMALL_LEFT] = 1;
    __syncthreads();
    if (tid == 0) agg_reserve(A, v);
    __syncthreads();
#pragma unroll
    for (int r = 0; r < ROWS; r++)
        if (hKind[r] >= 0) agg_write(A, v, hKind[r], hLocal[r], gs + (u32)tid + (u32)r * THREADS, hSize[r], largeNext, (uint2*)nullptr);
    // new group starts into the round's bit map (bit 0 of the group is set already)
    if (tid < nWords && L.fb[tid]) {
        const u32 off = gs + (u32)tid * 32u;
        const u32 sh = off & 31;
        atomicOr(&v.gnew[off >> 5], L.fb[tid] << sh);
        if (sh && (L.fb[tid] >> (32 - sh))) atomicOr(&v.gnew[(off >> 5) + 1], L.fb[tid] >> (32 - sh));
    }
}

// Write-back of a group whose majority key m is held by c members, with the nOth <= THREADS others sorted in oK / oV [0, nOth) and the
// majority's members behind them in their old (position) order: the result is [others < m][majority][others > m], `less` others in front.
template <int THREADS, int ROWS>
__device__ __forceinline__ void med_majority_write_back(MedLds<THREADS, ROWS>& L, const FwdView& v, u32 gs, u32 n, u32 nOth, u32 c, u32 less, u32 m)
{
    const int tid = (int)threadIdx.x;
    const u32 oldLab = L.oldLab;
    (void)n; (void)m;
    // ---- the majority: c members from slot gs + less on. It keeps the group's label when that slot is inside its range (see med_write_back)
    const u32 mStart = gs + less;
    const u32 rel = oldLab - gs;
    const u32 mLab = (c <= SM_G) ? mStart : ((rel >= less && rel < less + c) ? oldLab : mStart + (c >> 1));
    for (u32 i = (u32)tid; i < c; i += THREADS) {
        const u32 gp = L.oV[nOth + i];
        v.SA[mStart + i] = gp;
        if (mLab != oldLab) lab_set(v, gp, L.blkBase, mLab, oldLab);
    }
    u32 surv = 0;
    if (tid == 0) {
        if (less != 0) atomicOr(&v.gnew[mStart >> 5], 1u << (mStart & 31));
        if (c > SM_G) v.medStage[mStart >> 8] = make_uint2(mStart, c);      // (c <= n <= MED_CAP)
        else if (c > 1) surv = 1;
    }
    // ---- the others: one thread each
    if ((u32)tid < nOth) {
        const u32 t = (u32)tid;
        const u32 key = L.oK[t];
        u32 hd = t, e = t + 1;
        while (hd > 0 && L.oK[hd - 1] == key) hd--;
        while (e < nOth && L.oK[e] == key) e++;
        const u32 size = e - hd;
        const u32 shift = (t < less) ? 0u : c;                          // (equal keys are on one side of the majority)
        const u32 slot = gs + t + shift, hdSlot = gs + hd + shift;
        const u32 relO = rel - shift;                                   // the parent's label in the others' own index space (wraps when it is not there)
        const u32 lab = (size <= SM_G) ? hdSlot : ((oldLab >= hdSlot && oldLab < hdSlot + size) ? oldLab : hdSlot + (size >> 1));
        (void)relO;
        const u32 gp = L.oV[t];
        v.SA[slot] = gp;
        if (lab != oldLab) lab_set(v, gp, L.blkBase, lab, oldLab);
        if (t == hd) {
            if (hdSlot != gs) atomicOr(&v.gnew[hdSlot >> 5], 1u << (hdSlot & 31));
            if (size > SM_G) v.medStage[hdSlot >> 8] = make_uint2(hdSlot, size);
            else if (size > 1) surv = 1;
        }
    }
    if (__ballot(surv != 0) != 0 && (tid & 63) == 0) v.counters[CNT_SMALL_LEFT] = 1;
}

// The chain round. A group whose majority key is the group's OWN label: for most members p the suffix p + h is a member too, i.e. the
// members form chains p, p + h, p + 2h, ... inside the group (a periodic stretch whose period divides h) that end in a member e whose key is
// another label. With c(p) = steps from p to the end e(p) of its chain, two members compare like this: all of them start with the group's
// h symbols B, so suffix p = B^(c+1) followed by what the key of e(p) stands for. The one with the shorter chain meets its foreign
// key while the other still shows B (label = the group's own): it is the smaller one when that key is below the own label,
// the larger one when above; equal chain lengths leave the two foreign keys to decide. One sort on
//     hi = key(e) < own ? c : 2 cmax + 1 - c (cmax = the longest chain),   lo = rank of key(e) among the chain ends
// therefore does what log2(longest chain) doubling rounds would do; ties share (c + 1) h symbols and the depth of the end's label
// (at least 2h altogether) and go on as ordinary groups. The members are in position order (every sort of the pipeline is stable),
// so p + h is found by binary search in the group itself and c, e come from pointer jumping in LDS.
// It runs on a group that is in LDS already: oK / oV [0, n) = keys and positions in position order, m = the group's own label as a key,
// link = the offset the keys were gathered at (look_offset: h, or what the group is known to share beyond it). It needs no LDS beyond
// the group's own, because what it adds is never live together with what it replaces:
//   - a member's link and chain length are one word, (successor's index | steps << 16), and take the place of its position in oV once every
//     binary search has read the positions (the links wait in registers for that); the final re-gather reads the positions from SA, which
//     nothing has written yet;
//   - a member whose key is m has its successor in the group, so the chain ends are at most the others, n - c <= n / 2 <= CAP / 2 of them.
//     Their (key, index) pairs are sorted in the lower halves of oK / oV -- the keys pass through oV's upper half, since oK is read until
//     every member knows on which side of m its end's key lies -- and the ends' ranks, one word per member index, fill the two upper halves.
// A thread keeps one word per member throughout: end's index | chain length << 16 | (end's key below m) << 31, then the sort key, then the
// position. Returns false, with oK / oV untouched, when the ends would not fit half the capacity (members with key m whose successor is not
// in the group: that would be a group out of position order); the caller then refines the group the ordinary way. Returns true with
// the group sorted in oK / oV (positions) for med_write_back. Entered and left with the workgroup in step.
template <int THREADS, int ROWS>
__device__ __forceinline__ bool med_chain_round(MedLds<THREADS, ROWS>& L, const FwdView& v, u32 gs, u32 n, u32 m, u32 link, int npass)
{
    constexpr u32 CAP = (u32)ROWS * THREADS, HALF = CAP / 2;
    static_assert(CAP <= 0x2000u, "index and chain length of a member: 13 bits each");
    __shared__ u32 sEnds, sAt, sCmax, sMoved[2];
    const int tid = (int)threadIdx.x, lane = tid & 63;
    const unsigned long long ltMask = (lane == 0) ? 0ull : (~0ull >> (64 - lane));
    if (tid == 0) { sEnds = 0; sAt = 0; sCmax = 0; }
    __syncthreads();
    u32 w[ROWS];
    // ---- chain links: the member `link` further on (first index with position >= target)
    {
        u32 nE = 0;
#pragma unroll
        for (int r = 0; r < ROWS; r++) {
            const u32 i = (u32)tid + (u32)r * THREADS;
            w[r] = i;
            if (i < n) {
                bool found = false;
                if (L.oK[i] == m) {
                    const u32 target = L.oV[i] + link;
                    u32 lo = i + 1, hi = n;
                    if (lo < n && L.oV[lo] == target) hi = lo;     // (inside a stretch whose period is the link the next member is the one: no search)
                    while (lo < hi) { const u32 mid = (lo + hi) >> 1; if (L.oV[mid] < target) lo = mid + 1; else hi = mid; }
                    if (lo < n && L.oV[lo] == target) { w[r] = lo | (1u << 16); found = true; }
                }
                nE += found ? 0u : 1u;
            }
        }
        nE = wave_sum(nE);
        if (lane == 0 && nE) atomicAdd(&sEnds, nE);
    }
    __syncthreads();
    const u32 nEnds = sEnds;
    if (nEnds > HALF) return false;                        // (uniform; the next call's reset of sEnds lies behind the caller's barriers)
#pragma unroll
    for (int r = 0; r < ROWS; r++) { const u32 i = (u32)tid + (u32)r * THREADS; if (i < n) L.oV[i] = w[r]; }
    __syncthreads();
    // ---- pointer jumping: chain end and chain length of every member (until no link moves any more)
    for (u32 span = 1, it = 0; span < n; span <<= 1, it ^= 1) {
        bool moved = false;
#pragma unroll
        for (int r = 0; r < ROWS; r++) {
            const u32 i = (u32)tid + (u32)r * THREADS;
            if (i < n) {
                // (two hops a pass: the reach triples, and a pass is two barriers of all waves)
                const u32 wi = L.oV[i], j = wi & 0xFFFFu, wj = L.oV[j], k = wj & 0xFFFFu, wk = L.oV[k];
                w[r] = (wk & 0xFFFFu) | (((wi >> 16) + (wj >> 16) + (wk >> 16)) << 16);
                moved = moved || ((wk & 0xFFFFu) != k);
            }
        }
        if (tid == 0) sMoved[it] = 0;                              // (two flags in turn: the other one may still be read by a slow thread)
        __syncthreads();
        if (moved) sMoved[it] = 1;
#pragma unroll
        for (int r = 0; r < ROWS; r++) { const u32 i = (u32)tid + (u32)r * THREADS; if (i < n) L.oV[i] = w[r]; }
        __syncthreads();
        if (!sMoved[it]) break;
    }
    // (w = what oV holds for the thread's members, and nobody reads oV any more)
    // ---- the side of every member's end; the chain ends compacted (any order): indexes to oV [0, nEnds), keys to oV [HALF, HALF + nEnds)
    {
        u32 cm = 0;
#pragma unroll
        for (int r = 0; r < ROWS; r++) {
            const u32 i = (u32)tid + (u32)r * THREADS;
            const bool in = i < n;
            const u32 cc = w[r] >> 16;
            const u32 tail = in ? L.oK[w[r] & 0xFFFFu] : m;
            if (in && tail < m) w[r] |= 0x80000000u;
            cm = (in && cc > cm) ? cc : cm;
            const bool isEnd = in && cc == 0;
            const unsigned long long bal = __ballot(isEnd);
            u32 base0 = 0;
            if (lane == 0 && bal) base0 = atomicAdd(&sAt, (u32)__popcll(bal));
            base0 = (u32)__shfl((int)base0, 0, 64);
            if (isEnd) { const u32 at = base0 + (u32)__popcll(bal & ltMask); L.oV[at] = i; L.oV[HALF + at] = tail; }
        }
        cm = wave_max(cm);
        if (lane == 0 && cm) atomicMax(&sCmax, cm);
    }
    __syncthreads();
    for (u32 j = (u32)tid; j < nEnds; j += THREADS) L.oK[j] = L.oV[HALF + j];
    __syncthreads();
    // (the members' words wait in the upper halves while the ends are sorted, by index like the ranks that replace them, so that the
    // sort's registers do not come on top of them)
#pragma unroll
    for (int r = 0; r < ROWS; r++) { const u32 i = (u32)tid + (u32)r * THREADS; if (r < ROWS / 2) L.oK[HALF + i] = w[r]; else L.oV[i] = w[r]; }      // (i < HALF in the first half of the rows)
    // ---- the ends sorted by key
    if (nEnds <= (u32)THREADS) {
        u32 kk = 0, vv = 0, at = 0;
        if ((u32)tid < nEnds) {
            kk = L.oK[tid]; vv = L.oV[tid];
            for (u32 j = 0; j < nEnds; j++) { const u32 kj = L.oK[j]; at += (kj < kk || (kj == kk && j < (u32)tid)) ? 1u : 0u; }
        }
        __syncthreads();
        if ((u32)tid < nEnds) { L.oK[at] = kk; L.oV[at] = vv; }
        __syncthreads();
    } else {
        med_radix_sort<THREADS, ROWS>(L, nEnds, npass);
    }
#pragma unroll
    for (int r = 0; r < ROWS; r++) { const u32 i = (u32)tid + (u32)r * THREADS; w[r] = (r < ROWS / 2) ? L.oK[HALF + i] : L.oV[i]; }
    __syncthreads();
    // rank of an end's key = first index with that key, kept by the end's index: [0, HALF) in oK's upper half, [HALF, CAP) in oV's
    for (u32 j = (u32)tid; j < nEnds; j += THREADS) {
        const u32 key = L.oK[j];
        u32 lo = 0, hi = j;
        while (lo < hi) { const u32 mid = (lo + hi) >> 1; if (L.oK[mid] < key) lo = mid + 1; else hi = mid; }
        const u32 e = L.oV[j];
        if (e < HALF) L.oK[HALF + e] = lo; else L.oV[e] = lo;
    }
    __syncthreads();
    // ---- one sort of all members on (chain length or its mirror, rank of the end's key), as wide as the longest chain and the ends ask for
    const u32 cmax = sCmax;
    const u32 trBits = bitlen_u32(nEnds ? nEnds - 1 : 0), hiBits = bitlen_u32(2u * cmax + 1u);
#pragma unroll
    for (int r = 0; r < ROWS; r++) {
        const u32 i = (u32)tid + (u32)r * THREADS;
        if (i < n) {
            const u32 e = w[r] & 0xFFFFu, cc = (w[r] >> 16) & 0x7FFFu;
            const u32 hiKey = (w[r] >> 31) ? cc : (2u * cmax + 1u - cc);
            w[r] = (hiKey << trBits) | (e < HALF ? L.oK[HALF + e] : L.oV[e]);
        }
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < ROWS; r++) { const u32 i = (u32)tid + (u32)r * THREADS; if (i < n) { L.oK[i] = w[r]; L.oV[i] = i; } }
    __syncthreads();
    med_radix_sort<THREADS, ROWS>(L, n, (int)((hiBits + trBits + 7) / 8));
#pragma unroll
    for (int r = 0; r < ROWS; r++) { const u32 i = (u32)tid + (u32)r * THREADS; if (i < n) w[r] = v.SA[gs + L.oV[i]]; }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < ROWS; r++) { const u32 i = (u32)tid + (u32)r * THREADS; if (i < n) L.oV[i] = w[r]; }
    __syncthreads();
    return true;
}

// The refinement of one group whose keys and positions are in LDS (oK / oV [0, n), position order; the workgroup in step behind the
// stores): chain round, majority split or radix sort, write-back. info = (block base, the members' label), off = the offset the keys
// were gathered at. A group whose majority looks at the group itself takes the chain round, in place (med_chain_round).
// Left with the workgroup in step.
template <int THREADS, int ROWS, bool STATS>
__device__ __forceinline__ void med_sort_group(MedLds<THREADS, ROWS>& L, const FwdView& v, u32 gs, u32 n, uint2 info, int npass, u32 off,
                                               uint2* __restrict__ medNext, uint2* __restrict__ largeNext)
{
    constexpr int WAVES = THREADS / 64;
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const unsigned long long ltMask = (lane == 0) ? 0ull : (~0ull >> (64 - lane));
    if (tid == 0) { L.oldLab = info.y; L.blkBase = info.x; }
    // majority candidate: the key two of three probes agree on, else the middle one
    const u32 ka = L.oK[n >> 2], kb = L.oK[n >> 1], kc = L.oK[(n >> 2) * 3];
    const u32 m = (ka == kc) ? ka : kb;
    u32 c = 0;
    for (u32 i = (u32)tid; i < n; i += THREADS) c += (L.oK[i] == m) ? 1u : 0u;
    c = med_block_sum(L, c);
    bool chained = false;
    if (c < n && 2 * c >= n && n <= CHAIN_CAP && m == info.y - info.x + 1u) {
        // the majority looks at the group itself (a periodic stretch whose period divides h): the chain round finishes it in one round
        chained = med_chain_round<THREADS, ROWS>(L, v, gs, n, m, off, npass);
        if (chained && tid == 0) atomicAdd(&v.counters[CNT_CHAINED], 1u);
    }
    if (STATS && tid == 0 && c == n) { atomicAdd(&v.counters[CNT_STAT_UNSPLIT], 1u); atomicAdd(&v.counters[CNT_STAT_UNSPLIT_MEMBERS], n); }
    if (c < n && !chained) {
        if (2 * c >= n) {
            // ---- stable split: [others (nOth)][members with key m (c)]
            const int R = (int)((n + THREADS - 1) / THREADS);
            const u32 waveBase = (u32)wave * (u32)R * 64u;
            u32 key[ROWS], val[ROWS], pos[ROWS];
            u32 runO = 0, runE = 0;
#pragma unroll
            for (int r = 0; r < ROWS; r++) {
                key[r] = m; val[r] = 0; pos[r] = 0xFFFFFFFFu;
                if (r < R) {
                    const u32 idx = waveBase + (u32)r * 64u + (u32)lane;
                    const bool valid = idx < n;
                    if (valid) { key[r] = L.oK[idx]; val[r] = L.oV[idx]; }
                    const bool oth = valid && key[r] != m, same = valid && key[r] == m;
                    const unsigned long long bo = __ballot(oth), be = __ballot(same);
                    if (oth) pos[r] = runO + (u32)__popcll(bo & ltMask);
                    if (same) pos[r] = 0x80000000u | (runE + (u32)__popcll(be & ltMask));
                    runO += (u32)__popcll(bo);
                    runE += (u32)__popcll(be);
                }
            }
            if (lane == 0) { L.wtot[wave] = runO; L.wtot2[wave] = runE; }
            __syncthreads();
            u32 baseO = 0, baseE = 0, nOth = 0;
            for (int w = 0; w < WAVES; w++) { if (w < wave) { baseO += L.wtot[w]; baseE += L.wtot2[w]; } nOth += L.wtot[w]; }
#pragma unroll
            for (int r = 0; r < ROWS; r++) {
                if (r < R && pos[r] != 0xFFFFFFFFu) {
                    const u32 at = (pos[r] & 0x80000000u) ? (nOth + baseE + (pos[r] & 0x7FFFFFFFu)) : (baseO + pos[r]);
                    L.oK[at] = key[r];
                    L.oV[at] = val[r];
                }
            }
            __syncthreads();
            if (nOth <= (u32)THREADS) {
                // few others: rank by counting (stable: smaller keys, then equal keys that come earlier)
                u32 kk = 0, vv = 0, at = 0;
                if ((u32)tid < nOth) {
                    kk = L.oK[tid]; vv = L.oV[tid];
                    for (u32 j = 0; j < nOth; j++) { const u32 kj = L.oK[j]; at += (kj < kk || (kj == kk && j < (u32)tid)) ? 1u : 0u; }
                }
                __syncthreads();
                if ((u32)tid < nOth) { L.oK[at] = kk; L.oV[at] = vv; }
                __syncthreads();
                // A group that keeps its majority and loses a handful of members (round after round, for a periodic stretch): the
                // majority is written where it goes straight from the split order and keeps its label, each of the few others finds the
                // members it stays with by looking left and right among the sorted others -- no rearranging of the whole group, no bit map
                // over it, no scans (med_write_back does all that for the general case)
                u32 lessQ = 0;
                if ((u32)tid < nOth) lessQ = (L.oK[tid] < m) ? 1u : 0u;
                lessQ = med_block_sum(L, lessQ);
                if (tid == 0) { L.oldLab = info.y; L.blkBase = info.x; if (STATS) { atomicAdd(&v.counters[CNT_STAT_MAJ], 1u); atomicAdd(&v.counters[CNT_STAT_MAJ_MEMBERS], n); } }
                __syncthreads();
                med_majority_write_back<THREADS, ROWS>(L, v, gs, n, nOth, c, lessQ, m);
                __syncthreads();
                return;
            } else {
                med_radix_sort<THREADS, ROWS>(L, nOth, npass);
            }
            u32 less = 0;
            for (u32 i = (u32)tid; i < nOth; i += THREADS) less += (L.oK[i] < m) ? 1u : 0u;
            less = med_block_sum(L, less);
            // ---- [others < m][key m][others > m]
#pragma unroll
            for (int k = 0; k < ROWS; k++) {
                const u32 i = (u32)tid + (u32)k * THREADS;
                if (i < n) { key[k] = L.oK[i]; val[k] = L.oV[i]; }
            }
            __syncthreads();
#pragma unroll
            for (int k = 0; k < ROWS; k++) {
                const u32 i = (u32)tid + (u32)k * THREADS;
                if (i < n) {
                    const u32 at = (i < less) ? i : (i < nOth ? i + c : less + (i - nOth));
                    L.oK[at] = key[k];
                    L.oV[at] = val[k];
                }
            }
            __syncthreads();
        } else {
            med_radix_sort<THREADS, ROWS>(L, n, npass);
        }
    }
    med_write_back<THREADS, ROWS>(L, v, gs, n, medNext, largeNext);
    __syncthreads();
}

// One workgroup refines one group of 257..ROWS*THREADS members (descriptors of other sizes are left to the other
// instantiations of the kernel): keys and positions into LDS, sort, subgroup boundaries, SA / ISA / bit map / children.
// A group in which one key holds the majority (periodic stretches and runs: every member but the ones near the end of the
// stretch looks at the same group h further on) is first split, stably, into "that key" and "the others"; only the
// others are sorted.
// (Round 6 measured the keys fetched inside this kernel, versioned labels as in k_bwt_f_small_fused: gather + sort of the medium groups
// 9.1 -> 11.0 ms on the real files, 5.5 -> 6.9 on the stand-in -- a sorting workgroup waits for its own three dependent loads, the gather kernel
// keeps eight groups per CU in flight and walks the list XCD by XCD. The keys stay a kernel of their own.)
// The chain round runs here on plain labels as well: the round's keys sit in K before any label moves, med_chain_round works on the group's
// own LDS and re-reads positions only from the group's own range of SA, which no other workgroup writes.
// (STATS: the instantiation the knob bwt_stats launches; it counts the groups that come out unsplit and the ones of the majority path.)
template <int THREADS, int ROWS, bool STATS>
__global__ __launch_bounds__(THREADS, (THREADS >= 1024 ? 4 : THREADS / 128)) void k_bwt_f_sort_medium(FwdView v, const uint2* __restrict__ desc, u32 nDesc, u32 h, int npass, u32 minLen,
                                                               uint2* __restrict__ medNext, uint2* __restrict__ largeNext, const uint2* __restrict__ descInfo)
{
    constexpr u32 CAP = (u32)ROWS * THREADS;
    __shared__ MedLds<THREADS, ROWS> L;
    const int tid = (int)threadIdx.x;

    for (u32 g = blockIdx.x; g < nDesc; g += gridDim.x) {
        const uint2 d = desc[g];
        const u32 gs = d.x, n = d.y;
        if (n <= minLen || n > CAP) continue;               // uniform for the workgroup
        const uint2 info = descInfo[g];                     // (block base, the members' label)
        {
            // all loads of the group in flight before the first one is used
            u32 k[ROWS], p[ROWS];
#pragma unroll
            for (int r = 0; r < ROWS; r++) { const u32 i = (u32)tid + (u32)r * THREADS; k[r] = 0; p[r] = 0; if (i < n) { k[r] = v.K[gs + i]; p[r] = v.SA[gs + i]; } }
#pragma unroll
            for (int r = 0; r < ROWS; r++) { const u32 i = (u32)tid + (u32)r * THREADS; if (i < n) { L.oK[i] = k[r]; L.oV[i] = p[r]; } }
        }
        __syncthreads();
        med_sort_group<THREADS, ROWS, STATS>(L, v, gs, n, info, npass, look_offset(v, gs, h), medNext, largeNext);     // (the offset k_bwt_f_gather_desc gathered at)
    }
}

// Versioned labels: fetch, judge and sort a medium group in one workgroup. The launch gets the descriptors of ONE size class (classIdx:
// their indexes in the round's list, in slot order -- k_bwt_f_med_compact), so no workgroup is dealt a group of the other shape; the eight
// XCDs walk contiguous eighths of the class side by side, as k_bwt_f_gather_desc does with the list. The members' positions and keys
// (gather_key: lab_old answers with the label a position had when the round began, whatever the round has written since) stay in
// registers until the verdict: all keys equal -> the group is staged again and its verdict recorded, as k_bwt_f_gather_desc does, and
// nothing else is written; else they go to LDS and through med_sort_group. No key passes through K and nothing through descInfo.
// skip == 0 (knob bwt_no_unsplit_skip): every group is sorted.
template <int THREADS, int ROWS, bool STATS>
__global__ __launch_bounds__(THREADS, 4) void k_bwt_f_medium_fused(FwdView v, const uint2* __restrict__ desc, const u32* __restrict__ classIdx, u32 nClass, u32 h, int npass,
                                                               int skip, uint2* __restrict__ medNext, uint2* __restrict__ largeNext)
{
    constexpr u32 CAP = (u32)ROWS * THREADS;
    __shared__ MedLds<THREADS, ROWS> L;
    __shared__ u32 sDiff;
    const int tid = (int)threadIdx.x;
    const u32 xcd = blockIdx.x & 7, lanesPerXcd = gridDim.x >> 3, slot = blockIdx.x >> 3;      // the grid is a multiple of 8 workgroups
    const u32 per = (nClass + 7) / 8;
    const u32 lo = xcd * per, hi = (lo + per < nClass) ? lo + per : nClass;
    if (tid == 0) sDiff = 0;
    __syncthreads();
    for (u32 g = lo + slot; g < hi; g += lanesPerXcd) {
        const uint2 d = desc[classIdx[g]];
        const u32 gs = d.x, n = d.y;
        if (n <= SM_G || n > CAP) continue;                 // (uniform) void: taken apart by the probe, or asleep (k_bwt_f_med_sleep)
        const int blk = find_block(v.base, v.nBlocks, gs);  // (uniform)
        const u32 bb = v.base[blk], be = v.base[blk + 1];
        const u32 off = look_offset(v, gs, h);              // (uniform for the group)
        // the first member's label and key, by every thread for itself (one address for the workgroup, in flight beside the loads below)
        const u32 gp0 = v.SA[gs];
        const u32 lab = lab_old(v, gp0, bb), key0 = gather_key(v, gp0, off, bb, be);
        const bool judge = skip && lab - gs < n;           // (the label inside the group's range: see k_bwt_f_gather_desc)
        u32 gp[ROWS], key[ROWS];
#pragma unroll
        for (int r = 0; r < ROWS; r++) { const u32 i = (u32)tid + (u32)r * THREADS; gp[r] = (i < n) ? v.SA[gs + i] : bb; }
#pragma unroll
        for (int r = 0; r < ROWS; r++) { const u32 i = (u32)tid + (u32)r * THREADS; key[r] = (i < n) ? gather_key(v, gp[r], off, bb, be) : key0; }
        bool unsplit = false;
        if (judge) {                                        // (uniform; sDiff is 0 here)
            bool diff = false;
#pragma unroll
            for (int r = 0; r < ROWS; r++) diff = diff || key[r] != key0;       // (a slot behind the group's end holds key0)
            if (__ballot(diff) != 0 && (tid & 63) == 0) sDiff = 1;
            __syncthreads();
            unsplit = sDiff == 0;
        }
        if (tid == 0) {
            if (STATS) { atomicAdd(&v.counters[CNT_STAT_MED], n); atomicAdd(&v.counters[CNT_STAT_MED_GROUPS], 1u); }
            if (unsplit) med_leave_whole(v, d, key0, off, h, STATS);
        }
        if (unsplit) { __syncthreads(); continue; }         // (uniform; sDiff stays 0, and every thread has read it before the next group's verdict)
#pragma unroll
        for (int r = 0; r < ROWS; r++) { const u32 i = (u32)tid + (u32)r * THREADS; if (i < n) { L.oK[i] = key[r]; L.oV[i] = gp[r]; } }
        __syncthreads();
        if (tid == 0) sDiff = 0;                            // (every thread has read it; the barriers of the sort lie in front of the next group's verdict)
        med_sort_group<THREADS, ROWS, STATS>(L, v, gs, n, make_uint2(bb, lab), npass, off, medNext, largeNext);
    }
}

constexpr u32 PROBE_PMAX = 2048;
// Periodic stretches of ANY period, found by looking at the text (once, in front of the first doubling round). The members of a medium group are
// in position order; when most neighbours are the same distance P apart the group is mostly made of chains p, p + P, p + 2P, ...
// through stretches of period P, and doubling would refine it log2(stretch / h) times, peeling off only the members near the ends of
// the stretches each time, before the chain round can see the group look at itself (which it only does once P divides h). Here every
// member is compared with ONE member's text over the P symbols behind the ones the group shares: members that differ leave, ordered by
// where they differ and how (an ordinary refinement: a member that falls below the pattern earlier is smaller, one that rises above it
// earlier is larger, same place and byte stay together); the members that equal the pattern stay one group that is now KNOWN to share P
// symbols, which is recorded like a run length (FwdView::ovr / rtbits): its keys are gathered P positions on, where most members find
// the group itself, and the chain round finishes it in the first doubling round whatever P is (a block of text(2000) + 550 copies of a
// random 700-byte unit: 16 doubling rounds without this, 1 with it).
// candidates: medium groups with three equal distances around their middle member, a distance that is no power of two
// (a period that is a power of two is left to the doubling rounds: the chain round takes the group as soon as h reaches it, and the rounds up
// to there are cheap -- the majority of the members looks at one and the same group and is split off unsorted; measured on the stand-in's
// period-256 stretches the text comparison costs 3.4 ms and saves 1.7. Any other period never meets h.)
__global__ __launch_bounds__(256) void k_bwt_f_probe_scan(FwdView v, const uint2* __restrict__ desc, u32 depth, const u32* __restrict__ rtbits, u32* __restrict__ cand)
{
    const u32 nDesc = v.counters[CNT_MED];
    for (u32 g = blockIdx.x * 256 + threadIdx.x; g < nDesc; g += gridDim.x * 256) {
        const uint2 d = desc[g];
        const u32 gs = d.x, n = d.y;
        if (n <= SM_G || n > CHAIN_CAP) continue;
        if (rtbits != nullptr && ((rtbits[gs >> 5] >> (gs & 31)) & 1u)) continue;         // (groups of the run round know their offset already)
        const u32 a0 = v.SA[gs + (n >> 1) - 2], a1 = v.SA[gs + (n >> 1) - 1], a2 = v.SA[gs + (n >> 1)], a3 = v.SA[gs + (n >> 1) + 1];
        const u32 pd = a2 - a1;
        if ((a1 - a0 == pd) && (a3 - a2 == pd) && (pd > depth) && (pd <= 2048u) && ((pd & (pd - 1)) != 0)) cand[atomicAdd(&v.counters[CNT_PROBE_CAND], 1u)] = g;
    }
}

__global__ __launch_bounds__(512, 4) void k_bwt_f_probe(BwtView bv, FwdView v, uint2* __restrict__ desc, const u32* __restrict__ cand, u32 nCand, u32 depth, uint2* __restrict__ medNext,
                                                        uint2* __restrict__ largeNext, u32* __restrict__ ovr, u32* __restrict__ rtbits)
{
    constexpr int THREADS = 512, ROWS = 16;
    constexpr u32 CAP = (u32)ROWS * THREADS;
    __shared__ MedLds<THREADS, ROWS> L;
    __shared__ u32 patw[PROBE_PMAX / 4];
    u8* pat = reinterpret_cast<u8*>(patw);
    __shared__ u32 sInfo[4];                 // block base, block end, label of the group, -
    const int tid = (int)threadIdx.x;
    for (u32 cg = blockIdx.x; cg < nCand; cg += gridDim.x) {
        const u32 g = cand[cg];
        const uint2 d = desc[g];
        const u32 gs = d.x, n = d.y;
        bool take = n > SM_G && n <= CAP;
        __syncthreads();                                     // (LDS of the group before)
        if (take) {
            for (u32 i = (u32)tid; i < n; i += THREADS) L.oV[i] = v.SA[gs + i];
            if (tid == 0) {
                const int b = find_block(v.base, v.nBlocks, gs);
                sInfo[0] = v.base[b]; sInfo[1] = v.base[b + 1]; sInfo[3] = (u32)b;
            }
        }
        __syncthreads();
        u32 P = 0, pr = 0;
        if (take) {
            pr = L.oV[n >> 1];
            P = pr - L.oV[(n >> 1) - 1];
            take = P > depth && P <= PROBE_PMAX && pr + P <= sInfo[1];
        }
        if (take) {
            u32 c = 0;
            for (u32 i = (u32)tid; i + 1 < n; i += THREADS) c += (L.oV[i + 1] - L.oV[i] == P) ? 1u : 0u;
            c = med_block_sum(L, c);
            take = 2 * c >= n;
        }
        if (!take) continue;                                  // (uniform) the group goes on as it is
        const u32 bb = sInfo[0], be = sInfo[1];
        const u8* t = bv.src[sInfo[3]];
        for (u32 j = (u32)tid; j < P; j += THREADS) pat[j] = ldg<u8>(t + (pr - bb + j));
        if (tid == 0) sInfo[2] = lab_cur(v, pr, sInfo[0]);
        __syncthreads();
        // ---- every member against the pattern: where and how it differs
        constexpr u32 MID = 1u << 21;
        u32 nEq = 0, nBelow = 0;
        for (u32 i = (u32)tid; i < n; i += THREADS) {
            const u32 q0 = L.oV[i] - bb;
            u32 l = depth;
            // sixteen bytes at a time while they agree: the member's from five aligned dwords (all loads issued together), the pattern's
            // as dwords from LDS (`depth` and the steps are multiples of four)
            if ((depth & 3u) == 0) {
                const u32* pw = patw;
                while (l + 16 <= P && q0 + l + 20 <= be - bb) {
                    const uintptr_t ad = reinterpret_cast<uintptr_t>(t + q0 + l);
                    const u8* w = reinterpret_cast<const u8*>(ad & ~(uintptr_t)3);
                    const u32 sh = (u32)(ad & 3) * 8;
                    const u32 w0 = ldg<u32>(w), w1 = ldg<u32>(w + 4), w2 = ldg<u32>(w + 8), w3 = ldg<u32>(w + 12), w4 = ldg<u32>(w + 16);
                    const u32 x0 = sh ? ((w0 >> sh) | (w1 << (32 - sh))) : w0, x1 = sh ? ((w1 >> sh) | (w2 << (32 - sh))) : w1;
                    const u32 x2 = sh ? ((w2 >> sh) | (w3 << (32 - sh))) : w2, x3 = sh ? ((w3 >> sh) | (w4 << (32 - sh))) : w3;
                    const u32 d0 = x0 ^ pw[l >> 2], d1 = x1 ^ pw[(l >> 2) + 1], d2 = x2 ^ pw[(l >> 2) + 2], d3 = x3 ^ pw[(l >> 2) + 3];
                    if ((d0 | d1 | d2 | d3) != 0) break;
                    l += 16;
                }
            }
            u32 code = MID;
            while (l < P) {
                if (q0 + l >= be - bb) { code = l * 512u; break; }                        // the suffix ends here: a proper prefix sorts first
                const u32 x = ldg<u8>(t + q0 + l), y = pat[l];
                if (x != y) { code = (x < y) ? (l * 512u + x + 1u) : (MID + 1u + (P - l) * 512u + x + 1u); break; }
                l++;
            }
            L.oK[i] = code;
            nEq += (code == MID) ? 1u : 0u;
            nBelow += (code < MID) ? 1u : 0u;
        }
        nEq = med_block_sum(L, nEq);
        nBelow = med_block_sum(L, nBelow);
        if (2 * nEq < n) continue;                            // the pattern was not the stretches' (or there are none): nothing was written
        // the parts of the group are staged for the next round's list (med_write_back); this round's descriptor is void
        if (tid == 0) { L.oldLab = sInfo[2]; L.blkBase = sInfo[0]; desc[g].y = 0; }
        med_radix_sort<THREADS, ROWS>(L, n, 3);
        med_write_back<THREADS, ROWS>(L, v, gs, n, medNext, largeNext);
        // what every member is now known to share with the members it stays together with: the ones that equal the pattern P symbols
        // (slots [gs + nBelow, + nEq)), a member that left at symbol l with the ones that left there with the same byte l + 1
        for (u32 i = (u32)tid; i < n; i += THREADS) {
            const u32 code = L.oK[i];
            const u32 lshare = (code == MID) ? P : ((code < MID) ? (code >> 9) : (P - ((code - MID - 1u) >> 9))) + 1u;
            ovr[gs + i] = lshare;
            atomicOr(&rtbits[(gs + i) >> 5], 1u << ((gs + i) & 31));
        }
    }
}

// ------------------------------------------------------------------------------------------------
// large groups: one global sort of (descriptor index, key) pairs
// ------------------------------------------------------------------------------------------------
// loff[i] = sum of the lengths of the descriptors before i; loff[n] = total
// (+ lbase[i] = first slot of the block descriptor i lies in: the placing kernels store labels relative to it, lab_set)
__global__ __launch_bounds__(1024) void k_bwt_f_large_prefix(const uint2* __restrict__ desc, u32 nDesc, u32* __restrict__ loff, const u32* __restrict__ base, int nBlocks,
                                                             u32* __restrict__ lbase)
{
    __shared__ u32 part[1024];
    const u32 per = (nDesc + 1023) / 1024;
    const u32 lo = threadIdx.x * per, hi = (lo + per < nDesc) ? lo + per : nDesc;
    u32 sum = 0;
    for (u32 i = lo; i < hi; i++) { sum += desc[i].y; lbase[i] = base[find_block(base, nBlocks, desc[i].x)]; }
    part[threadIdx.x] = sum;
    __syncthreads();
    if (threadIdx.x == 0) { u32 run = 0; for (int t = 0; t < 1024; t++) { const u32 x = part[t]; part[t] = run; run += x; } loff[nDesc] = run; }
    __syncthreads();
    u32 run = part[threadIdx.x];
    for (u32 i = lo; i < hi; i++) { loff[i] = run; run += desc[i].y; }
}

// KEY = u32 when descriptor index and key fit 32 bits together (two thirds of the sort's traffic), else u64
template <class KEY>
__global__ __launch_bounds__(256) void k_bwt_f_large_keys(FwdView v, const uint2* __restrict__ desc, u32 nDesc, const u32* __restrict__ loff,
                                                          u32 L, u32 h, int kbits, KEY* __restrict__ keys, u32* __restrict__ vals)
{
    const u32 j = blockIdx.x * 256 + threadIdx.x;
    if (j >= L) return;
    u32 lo = 0, hi = nDesc;
    while (hi - lo > 1) { const u32 mid = (lo + hi) >> 1; if (loff[mid] <= j) lo = mid; else hi = mid; }
    const uint2 d = desc[lo];
    const u32 slot = d.x + (j - loff[lo]);
    const int b = find_block(v.base, v.nBlocks, d.x);
    const u32 gp = v.SA[slot];
    const u32 key = gather_key(v, gp, look_offset(v, d.x, h), v.base[b], v.base[b + 1]);
    keys[j] = (KEY)(((u64)lo << kbits) | (u64)key);
    vals[j] = gp;
}

template <class KEY>
__global__ __launch_bounds__(256) void k_bwt_f_large_flags(const KEY* __restrict__ keys, u32 L, u32* __restrict__ headIdx, u32* __restrict__ nextIdxRev)
{
    const u32 j = blockIdx.x * 256 + threadIdx.x;
    if (j >= L) return;
    const bool f = (j == 0) || (keys[j] != keys[j - 1]);
    headIdx[j] = f ? j : 0u;
    nextIdxRev[L - 1 - j] = f ? j : L;
}

template <class KEY>
__global__ __launch_bounds__(256) void k_bwt_f_large_place(FwdView v, const uint2* __restrict__ desc, const u32* __restrict__ loff, u32 L, int kbits,
                                                           const KEY* __restrict__ keys, const u32* __restrict__ vals, const u32* __restrict__ head,
                                                           const u32* __restrict__ nextRev, uint2* __restrict__ medNext, uint2* __restrict__ largeNext,
                                                           const u32* __restrict__ lbase)
{
    const u32 j = blockIdx.x * 256 + threadIdx.x;
    u32 surv = 0;
    u32 mySlot = 0;
    bool setBit = false;
    __shared__ ClassAgg A;
    agg_init(A);
    __syncthreads();
    int hKind = -1;
    u32 hLocal = 0, hSize = 0;
    if (j < L) {
        const u32 di = (u32)(keys[j] >> kbits);
        const u32 gs = desc[di].x, off = loff[di];
        const u32 gp = vals[j];
        const u32 nh = head[j];
        v.SA[gs + (j - off)] = gp;
        // (a large group's label is its first slot: round 0 and this kernel are the only ones that make large groups)
        if (nh != off) lab_set(v, gp, lbase[di], gs + (nh - off), gs);
        mySlot = gs + (j - off);
        if (nh == j) {
            const u32 nxt = (j + 1 < L) ? nextRev[L - 2 - j] : L;
            setBit = (j != off);
            hSize = nxt - j;
            hKind = agg_note(A, hSize, false, surv, hLocal);
        }
    }
    if (__ballot(surv != 0) != 0 && (threadIdx.x & 63) == 0) v.counters[CNT_SMALL_LEFT] = 1;
    __syncthreads();
    if (threadIdx.x == 0) agg_reserve(A, v);
    __syncthreads();
    if (hKind >= 0) agg_write(A, v, hKind, hLocal, mySlot, hSize, largeNext, (uint2*)nullptr);
    // new group starts: the lanes of a wave mostly hold consecutive slots (one group), so their bits are put together with a
    // ballot and leave as at most three word-wide ORs per wave; lanes that are out of line (a group border inside the wave) OR
    // their own bit
    const int lane = (int)(threadIdx.x & 63);
    const u32 s0 = (u32)__shfl((int)mySlot, 0, 64);
    const bool inLine = (j < L) && (mySlot == s0 + (u32)lane);
    const unsigned long long mask = __ballot(setBit && inLine);
    if (setBit && !inLine) atomicOr(&v.gnew[mySlot >> 5], 1u << (mySlot & 31));
    if (mask != 0 && lane == 0) {
        const u32 w0 = s0 >> 5, sh = s0 & 31;
        const u32 p0 = (u32)(mask << sh);
        const u32 p1 = sh ? (u32)(mask >> (32 - sh)) : (u32)(mask >> 32);
        const u32 p2 = sh ? (u32)(mask >> (64 - sh)) : 0u;
        if (p0) atomicOr(&v.gnew[w0], p0);
        if (p1) atomicOr(&v.gnew[w0 + 1], p1);
        if (p2) atomicOr(&v.gnew[w0 + 2], p2);
    }
}

// ------------------------------------------------------------------------------------------------
// runs of one byte: finished in one round by their length
// ------------------------------------------------------------------------------------------------
// Members of a run group all start with nsym copies of a byte c. With R = length of the run of c that starts at the position, a =
// the byte behind the run (or the block end, which sorts first), two members compare like (R, a): the one whose run ends first
// is smaller when its a is below c, larger when above; equal (R, a) leave the suffixes behind the runs to decide. So ONE sort on
//   hi = (a < c) ? R : 2^(kbits+1) - 1 - R,   lo = ISA[p + R] (rank of the suffix behind the run, 0 at the block end)
// replaces the log2(R / nsym) doubling rounds such a group would otherwise take; members that still tie share R + nsym symbols.

// run-end flags in position order: bit set where the next byte differs or the block ends (and for everything past the end);
// a thread makes the flag byte of 8 positions, a workgroup the 2048 positions of one window
__global__ __launch_bounds__(256) void k_bwt_f_run_ends(BwtView bv, FwdView v, u8* __restrict__ ebits8)
{
    __shared__ int sBlk;
    const u32 pos0 = blockIdx.x * SM_WIN;
    if (threadIdx.x == 0) sBlk = find_block(v.base, v.nBlocks, pos0 < v.total ? pos0 : v.total - 1);
    __syncthreads();
    const u32 g0 = pos0 + 8u * threadIdx.x;
    u32 flags = 0xFF;
    if (g0 < v.total) {
        int b = sBlk;
        while (g0 >= v.base[b + 1]) b++;
        u32 bb = v.base[b], be = v.base[b + 1];
        const u8* t = bv.src[b];
        u32 cur = t[g0 - bb];
        flags = 0;
#pragma unroll
        for (u32 k = 0; k < 8; k++) {
            const u32 gp = g0 + k;
            if (gp >= v.total) { flags |= 1u << k; continue; }
            if (gp + 1 >= be) {                               // last byte of a block: the run ends here
                flags |= 1u << k;
                if (gp + 1 < v.total) { b++; while (v.base[b + 1] <= gp + 1) b++; bb = be; be = v.base[b + 1]; t = bv.src[b]; cur = t[0]; }   // (blocks the BWT skips are empty here)
                continue;
            }
            const u32 nxt = t[gp + 1 - bb];
            flags |= (cur != nxt ? 1u : 0u) << k;
            cur = nxt;
        }
    }
    ebits8[g0 >> 3] = (u8)flags;
}

// R[gp] = distance to the end of the run that holds gp (1 = the run ends here); one workgroup per window of 2048 positions
// SCAN (FwdSort::run_scan, before round 0's sort, when nobody knows yet which bytes have run groups): every run of at least nsym bytes is
// a candidate start, and its members are counted for its (block, byte): L - nsym + 1 into members[], its position into firstPos[] (the
// least one stays). Per workgroup through LDS where the window lies in one block: a zero-filled stretch is thousands of windows that
// would otherwise all add to one word.
template <bool SCAN>
__global__ __launch_bounds__(256) void k_bwt_f_run_len(BwtView bv, FwdView v, const u32* __restrict__ ebits, const u32* __restrict__ winFirstInclRev, u32 nWin,
                                                       u32* __restrict__ R, const u32* __restrict__ classTab, u32 nsym, unsigned long long* __restrict__ startBits64,
                                                       u32* __restrict__ startCount, u32* __restrict__ members, u32* __restrict__ firstPos)
{
    __shared__ u32 bw[64];
    __shared__ u32 nextSet[64];
    __shared__ int sBlk;
    __shared__ u32 sMem[SCAN ? 256 : 1], sFirst[SCAN ? 256 : 1];
    const int tid = (int)threadIdx.x;
    const u32 win = blockIdx.x, pos0 = win * SM_WIN;
    if (SCAN) { sMem[tid] = 0u; sFirst[tid] = 0xFFFFFFFFu; }
    if (tid == 64) sBlk = find_block(v.base, v.nBlocks, pos0 < v.total ? pos0 : v.total - 1);
    if (tid < 64) {
        const u32 w = ebits[(pos0 >> 5) + (u32)tid];
        bw[tid] = w;
        u32 sm = w ? (u32)(tid * 32 + __ffs((int)w) - 1) : NO_BIT;
        for (int o = 1; o < 64; o <<= 1) {
            const u32 u = (u32)__shfl_down((int)sm, (unsigned)o, 64);
            if (tid + o < 64) sm = u < sm ? u : sm;
        }
        u32 sex = (u32)__shfl_down((int)sm, 1u, 64);
        if (tid == 63) sex = NO_BIT;
        nextSet[tid] = sex;
    }
    __syncthreads();
    const u32 after = (win + 1 < nWin) ? winFirstInclRev[nWin - 2 - win] : v.total - 1;
    const u32 prevWord = pos0 ? ebits[(pos0 >> 5) - 1] : 0xFFFFFFFFu;      // (the run-end bit of the position in front of the window)
    const bool oneBlock = SCAN && pos0 + SM_WIN <= v.base[sBlk + 1];       // (uniform)
    u32 rmax = 0;
#pragma unroll
    for (int k = 0; k < (int)(SM_WIN / 256); k++) {
        const u32 i = (u32)tid + 256u * (u32)k;
        const u32 gp = pos0 + i;
        bool start = false;
        if (gp < v.total) {
            const u32 w = i >> 5, bit = i & 31;
            const u32 m = bw[w] & (0xFFFFFFFFu << bit);              // this position or later
            const u32 ei = m ? (w * 32 + (u32)__ffs((int)m) - 1) : nextSet[w];
            const u32 e = (ei != NO_BIT) ? pos0 + ei : after;
            const u32 r = e - gp + 1;
            R[gp] = r;
            rmax = r > rmax ? r : rmax;
            // a run starts here when a run ends right in front (block ends are run ends); it takes part in the run-length round when it
            // is at least nsym long and its byte has a run group
            const bool endBefore = (i == 0) ? ((prevWord >> 31) & 1u) != 0 : ((bw[(i - 1) >> 5] >> ((i - 1) & 31)) & 1u) != 0;
            if (endBefore && r >= nsym) {
                int b = sBlk;
                while (gp >= v.base[b + 1]) b++;
                const u32 c = (u32)bv.src[b][gp - v.base[b]];
                if (SCAN) {
                    start = true;
                    if (oneBlock) { atomicAdd(&sMem[c], r - nsym + 1u); atomicMin(&sFirst[c], gp - v.base[b]); }
                    else { atomicAdd(&members[(u32)b * 256u + c], r - nsym + 1u); atomicMin(&firstPos[(u32)b * 256u + c], gp - v.base[b]); }
                } else start = classTab[(u32)b * 256u + c] != 0xFFFFFFFFu;
            }
        }
        const unsigned long long m64 = __ballot(start);
        if ((tid & 63) == 0) {
            startBits64[(pos0 + 256u * (u32)k + (u32)(tid & ~63)) >> 6] = m64;
            if (!SCAN) {                                             // (k_bwt_f_run_starts counts what it leaves of the candidates)
                startCount[((pos0 + 256u * (u32)k + (u32)(tid & ~63)) >> 5)] = (u32)__popc((u32)m64);
                startCount[((pos0 + 256u * (u32)k + (u32)(tid & ~63)) >> 5) + 1] = (u32)__popc((u32)(m64 >> 32));
            }
        }
    }
    if (SCAN) {
        __syncthreads();
        if (oneBlock && sMem[tid]) { atomicAdd(&members[(u32)sBlk * 256u + (u32)tid], sMem[tid]); atomicMin(&firstPos[(u32)sBlk * 256u + (u32)tid], sFirst[tid]); }
    }
    rmax = wave_max(rmax);
    // longest run: sizes the key of the run-length sort (read first: one atomic per wave on one address would serialise the launch)
    if ((tid & 63) == 0 && rmax > __atomic_load_n(&v.counters[CNT_RUN_LONGEST], __ATOMIC_RELAXED)) atomicMax(&v.counters[CNT_RUN_LONGEST], rmax);
}

// The run groups known before the sort (FwdSort::run_scan): a (block, byte) with more than SM_G members is a run group -- the group
// round 0 would make of them. classTab marks them (any value but 0xFFFFFFFF; k_bwt_f_run_classes puts the descriptor indexes there once
// round 0 has listed the groups), members[] keeps their counts and drops the others, cbase[] = the blocks' bases without the members in
// front of them: the compact segments of the sort. One workgroup.
__global__ __launch_bounds__(256) void k_bwt_f_run_scan_classes(u32* __restrict__ members, u32* __restrict__ classTab, const u32* __restrict__ base, u32* __restrict__ cbase,
                                                                int nBlocks, u32* __restrict__ counters)
{
    __shared__ u32 sSum;
    const int tid = (int)threadIdx.x;
    u32 out = 0, mine = 0;                                           // (thread 0: members in the blocks so far)
    for (int b = 0; b < nBlocks; b++) {
        const u32 m = members[(u32)b * 256u + (u32)tid];
        const bool q = m > SM_G;
        classTab[(u32)b * 256u + (u32)tid] = q ? 0u : 0xFFFFFFFFu;
        if (!q) members[(u32)b * 256u + (u32)tid] = 0u;
        if (tid == 0) sSum = 0;
        __syncthreads();
        if (q) { atomicAdd(&sSum, m); mine++; }
        __syncthreads();
        if (tid == 0) { cbase[b] = base[b] - out; out += sSum; }
        __syncthreads();
    }
    if (tid == 0) { cbase[nBlocks] = base[nBlocks] - out; counters[CNT_GAP_MEMBERS] = out; }
    if (mine) atomicAdd(&counters[CNT_GAP_CLASSES], mine);
}

// the candidate run starts of k_bwt_f_run_len<true> cut down to the runs of run-group bytes, and counted per word
__global__ __launch_bounds__(256) void k_bwt_f_run_starts(BwtView bv, FwdView v, u32* __restrict__ bits, u32 nWords, const u32* __restrict__ classTab, u32* __restrict__ startCount)
{
    const u32 w = blockIdx.x * 256 + threadIdx.x;
    if (w >= nWords) return;
    u32 x = bits[w], out = 0;
    if (x) {
        int b = find_block(v.base, v.nBlocks, 32u * w);               // (a candidate is a position: 32 w < total)
        while (x) {
            const u32 k = (u32)__ffs((int)x) - 1u, gp = 32u * w + k;
            while (gp >= v.base[b + 1]) b++;
            if (classTab[(u32)b * 256u + (u32)bv.src[b][gp - v.base[b]]] != 0xFFFFFFFFu) out |= 1u << k;
            x &= x - 1u;
        }
        bits[w] = out;
    }
    startCount[w] = (u32)__popc(out);
}

// the run groups as ordinary groups (when the run-length round cannot take them)
__global__ __launch_bounds__(256) void k_bwt_f_run_fallback(FwdView v, const uint2* __restrict__ runList, u32 nRun, uint2* __restrict__ medNext, uint2* __restrict__ largeNext)
{
    const u32 g = blockIdx.x * 256 + threadIdx.x;
    u32 surv = 0;
    if (g < nRun) classify_child(v, medNext, largeNext, runList[g].x, runList[g].y, surv);
}

// ---- the run-length round without a sort of (key, position) pairs over 48 bits ----------------------------------------------
// A member's key (run length R, what follows the run) is a property of its RUN except for R itself: a run of length L of a
// run-group byte has the members R = nsym .. L, and all of them share the direction bit and the rank T of the suffix behind the
// run. So the runs (a few per cent of the members in number) are sorted on (class, direction, T) first; the members are then
// generated run by run in that order and sorted, stably, on (class, hi(R)) alone -- three passes over 8-byte elements for 24 key
// bits, where the pair sort took six passes over 12-byte elements: the order of equal (class, hi) is the order of the runs, i.e.
// T. What k_bwt_f_large_flags / _place want -- the full key and the position per slot -- is rebuilt from the run table.
// That is the order of work of a batch with a run longer than RUN_DIRECT_LMAX and of the knob bwt_run_sort. Every other batch sorts the
// runs the same way and then writes each member's record straight to its slot, which three counts over the runs give ("the members placed
// directly" below: k_bwt_f_run_seg_marks .. k_bwt_f_run_emit in place of k_bwt_f_run_members, the member sort and k_bwt_f_run_expand).

// class of a run-group byte: classTab[block * 256 + byte] = index of the group's descriptor
__global__ __launch_bounds__(256) void k_bwt_f_run_classes(BwtView bv, FwdView v, const uint2* __restrict__ runList, u32 nRun, u32* __restrict__ classTab)
{
    const u32 d = blockIdx.x * 256 + threadIdx.x;
    if (d >= nRun) return;
    const u32 gp = v.SA[runList[d].x];
    const int b = find_block(v.base, v.nBlocks, gp);
    classTab[(u32)b * 256u + (u32)bv.src[b][gp - v.base[b]]] = d;
}

__global__ __launch_bounds__(256) void k_bwt_f_run_compact(const u32* __restrict__ bits, const u32* __restrict__ wprefix, u32 nWords, u32* __restrict__ runPos)
{
    const u32 w = blockIdx.x * 256 + threadIdx.x;
    if (w >= nWords) return;
    u32 word = bits[w];
    u32 at = wprefix[w];
    while (word) {
        const u32 k = (u32)__ffs((int)word) - 1;
        runPos[at++] = 32u * w + k;
        word &= word - 1;
    }
}

// run k: end, length, and the sort key [class | above? | T | k]
__global__ __launch_bounds__(256) void k_bwt_f_run_table(BwtView bv, FwdView v, const u32* __restrict__ runPos, u32 nRuns, const u32* __restrict__ R,
                                                         const u32* __restrict__ classTab, int kbits, int idxBits, u64* __restrict__ runKeys,
                                                         u32* __restrict__ runE, u32* __restrict__ runL, const uint2* __restrict__ gapList, u32 nsym)
{
    const u32 k = blockIdx.x * 256 + threadIdx.x;
    if (k >= nRuns) return;
    const u32 p = runPos[k];
    const int b = find_block(v.base, v.nBlocks, p);
    const u32 bb = v.base[b], be = v.base[b + 1];
    const u8* t = bv.src[b];
    const u32 c = t[p - bb], L = R[p], e = p + L;
    const bool below = (e >= be) || (t[e - bb] < c);                 // the block end sorts in front of every byte
    u64 T = 0ull;
    if (e < be) {
        // gapList (the run list, when the members stayed out of round 0's sort): a member of a run group has no label yet. Behind a run
        // that can only be the first position of another run, and its label is its group's first slot
        u32 d = 0xFFFFFFFFu;
        if (gapList != nullptr && R[e] >= nsym) d = classTab[(u32)b * 256u + (u32)t[e - bb]];
        T = (u64)((d != 0xFFFFFFFFu ? gapList[d].x : lab_cur(v, e, bb)) - bb + 1u);
    }
    const u64 cls = classTab[(u32)b * 256u + c];
    runKeys[k] = ((((cls << 1) | (below ? 0ull : 1ull)) << kbits | T) << idxBits) | (u64)k;
    runE[k] = e;
    runL[k] = L;
}

// the runs in sorted order: end, (class, direction, T), number of members
__global__ __launch_bounds__(256) void k_bwt_f_run_sorted(const u64* __restrict__ runKeys, u32 nRuns, int idxBits, const u32* __restrict__ runE,
                                                          const u32* __restrict__ runL, u32 nsym, u32* __restrict__ sE, u64* __restrict__ sKey, u32* __restrict__ cnt)
{
    const u32 k = blockIdx.x * 256 + threadIdx.x;
    if (k >= nRuns) return;
    const u64 key = runKeys[k];
    const u32 idx = (u32)(key & ((1ull << idxBits) - 1ull));
    sE[k] = runE[idx];
    sKey[k] = key >> idxBits;
    cnt[k] = runL[idx] - nsym + 1u;
}

// member j (members of run 0 first, then of run 1, ...): [class | hi(R) | run index]; a workgroup makes 2048 consecutive members
__global__ __launch_bounds__(256) void k_bwt_f_run_members(const u32* __restrict__ moff, u32 nRuns, u32 M, const u64* __restrict__ sKey, int kbits, int hbits,
                                                           u32 nsym, u64* __restrict__ mkeys)
{
    __shared__ u32 sOff[2048 + 1];
    __shared__ u32 sFirst;
    const u32 j0 = blockIdx.x * 2048u;
    if (j0 >= M) return;
    if (threadIdx.x == 0) {
        u32 lo = 0, hi = nRuns;                                      // last run with moff <= j0
        while (hi - lo > 1) { const u32 mid = (lo + hi) >> 1; if (moff[mid] <= j0) lo = mid; else hi = mid; }
        sFirst = lo;
    }
    __syncthreads();
    const u32 k0 = sFirst;
    // every run has at least one member: the members of this tile belong to at most 2048 runs
    for (u32 i = threadIdx.x; i <= 2048u; i += 256) sOff[i] = (k0 + i < nRuns) ? moff[k0 + i] : 0xFFFFFFFFu;
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 8; q++) {
        const u32 j = j0 + (u32)q * 256u + threadIdx.x;
        if (j >= M) continue;
        u32 lo = 0, hi = 2048;
        while (hi - lo > 1) { const u32 mid = (lo + hi) >> 1; if (sOff[mid] <= j) lo = mid; else hi = mid; }
        if (sOff[hi] <= j) lo = hi;
        const u32 k = k0 + lo;
        const u64 key = sKey[k];
        const u64 cls = key >> (kbits + 1);
        const bool above = (key >> kbits) & 1ull;
        const u64 Rr = (u64)nsym + (u64)(j - sOff[lo]);
        const u64 hiK = above ? ((1ull << hbits) - 1ull - Rr) : Rr;
        mkeys[j] = (((cls << hbits) | hiK) << 32) | (u64)k;
    }
}

// sorted members -> the (key, position) pairs k_bwt_f_large_flags / k_bwt_f_large_place work on: key = [class | hi | T]
__global__ __launch_bounds__(256) void k_bwt_f_run_expand(const u64* __restrict__ mkeys, u32 M, const u64* __restrict__ sKey, const u32* __restrict__ sE,
                                                          int kbits, int hbits, u64* __restrict__ keys, u32* __restrict__ vals, u32* __restrict__ Rout)
{
    const u32 j = blockIdx.x * 256 + threadIdx.x;
    if (j >= M) return;
    const u64 mk = mkeys[j];
    const u32 k = (u32)mk;
    const u64 ch = mk >> 32;                                         // class | hi
    const u64 hiK = ch & ((1ull << hbits) - 1ull);
    const u64 rk = sKey[k];
    const bool above = (rk >> kbits) & 1ull;
    const u64 T = rk & ((1ull << kbits) - 1ull);
    const u32 Rr = (u32)(above ? ((1ull << hbits) - 1ull - hiK) : hiK);
    keys[j] = (ch << kbits) | T;
    vals[j] = sE[k] - Rr;
    Rout[j] = Rr;
}

// ---- the members placed directly (no sort of the members at all) ---------------------------------------------------------------
// The member sort above only transposes a ragged matrix. The sorted runs fall into segments of equal (class, direction); the sorted
// members of a segment are its columns R, ascending for "below" and descending for "above", and column R holds the runs with L >= R
// in run order. So the slot of member (run k, R) is
//   (members in front of the segment: moff of its first run) + (members of the columns in front of R) + #{earlier runs of the segment with L >= R},
// three counts over the runs. A segment is cut into tiles of RUN_TILE consecutive runs (most segments are one partly filled tile; one
// per block -- byte 0 of the stand-in -- has tens of thousands of runs), a tile into rows of 64 runs, one wave each:
//   k_bwt_f_run_seg_marks, max scans     first run of the segment of every run, and of its stretch of equal keys
//   k_bwt_f_run_tie_marks, max scan      per run: the longest earlier run of its stretch (which of its members start a tie)
//   k_bwt_f_run_tile_marks, sum scan,
//   k_bwt_f_run_tile_starts              the tiles [tileStart[t], tileStart[t + 1]) in run order, their number in CNT_RUN_TILES
//   k_bwt_f_run_tile_counts              tiles of segments of several tiles: colTab[tile][R] = #{runs of the tile with L >= R}
//   k_bwt_f_run_tile_scan                per such segment and column: colTab[tile][R] = column offset of R + runs of the tiles in front
//   k_bwt_f_run_emit                     per tile: the same counts per row in LDS, RUN_CH columns at a time; a wave then walks the columns
//                                        of its row, ranks the runs that are still alive with a ballot and writes their members:
//                                        SA and R (ovr) to the member's slot, its tie flag as a byte
//   k_bwt_f_run_tie_bits                 the tie flags as the bit map k_bwt_f_run_place reads
// No record per member is written: what the member sort's kernels pass on as key, position and R per member is a function of the run
// tables. k_bwt_f_run_place<true> then writes the labels and lists the ties.
// Every loop is bounded by a count known when the kernel starts (runs of the tile, RUN_DIRECT_LMAX columns, tiles of the batch); nothing
// waits for another workgroup. The host launches one workgroup per tile there CAN be (segments + runs / RUN_TILE), the ones past
// CNT_RUN_TILES leave at once: no read-back. Runs longer than RUN_DIRECT_LMAX (a block of one byte: one run, one member per position)
// send the batch through the member sort above: the tables are sized by that bound, and a column costs a wave one step however few of
// its runs reach it. So does a batch with so many runs that a run's index and a length do not fit one word of k_bwt_f_run_tie_marks'
// scan (idxBits + RUN_LBITS > 32: more than 4 M runs).
constexpr u32 RUN_TILE = 1024;                       // runs per tile (16 rows of 64)
constexpr u32 RUN_ROWS = RUN_TILE / 64;
constexpr u32 RUN_DIRECT_LMAX = 1023;                // longest run the direct path takes (RUN_LBITS bits: k_bwt_f_run_tie_marks)
constexpr u32 RUN_COLS = RUN_DIRECT_LMAX + 1;        // columns of a tile's row in colTab (column R at index R)
constexpr u32 RUN_CH = 256;                          // columns k_bwt_f_run_emit counts at a time
static_assert(RUN_COLS == 4 * 256 && RUN_CH == 256 && RUN_ROWS % 4 == 0, "the kernels below map columns and rows to 256 threads");
// slots of colTab: a tile of RUN_TILE runs holds exactly one multiple of RUN_TILE, the last, shorter tile of a segment of several
// tiles follows a full one of its segment
static inline size_t run_tile_slots(size_t maxRuns) { return 2 * (maxRuns / RUN_TILE + 2); }

struct RunTile { u32 k0, k1, a, slot; bool first, last, multi; };
__device__ __forceinline__ RunTile run_tile(const u32* __restrict__ tileStart, const u32* __restrict__ segStart, u32 nRuns, u32 t)
{
    RunTile r;
    r.k0 = tileStart[t]; r.k1 = tileStart[t + 1]; r.a = segStart[r.k0];
    r.first = r.k0 == r.a;
    r.last = r.k1 >= nRuns || segStart[r.k1] == r.k1;
    r.multi = !(r.first && r.last);
    r.slot = (r.k1 - r.k0 == RUN_TILE) ? 2u * ((r.k0 + RUN_TILE - 1) / RUN_TILE) : (r.k0 >= RUN_TILE ? 2u * ((r.k0 - 1) / RUN_TILE) + 1u : 1u);
    return r;
}

// (strMark: the same for the stretches of equal (class, direction, T) inside the segments, see k_bwt_f_run_tie_marks)
__global__ __launch_bounds__(256) void k_bwt_f_run_seg_marks(const u64* __restrict__ sKey, u32 nRuns, int kbits, u32* __restrict__ segMark, u32* __restrict__ strMark)
{
    const u32 k = blockIdx.x * 256 + threadIdx.x;
    if (k >= nRuns) return;
    const u64 key = sKey[k], prev = k > 0 ? sKey[k - 1] : 0ull;
    segMark[k] = (k > 0 && (key >> kbits) == (prev >> kbits)) ? 0u : k;     // (a running maximum makes it the segment's first run)
    strMark[k] = (k > 0 && key == prev) ? 0u : k;
}

// Ties among the members placed directly, from the runs alone. Two members of a column (class, direction, R) tie when their runs follow
// the same text, i.e. lie in one STRETCH of equal sKey; such runs are adjacent. The member in front of (run k, R) in its column is the
// nearest earlier run of the segment with L >= R, and that run lies in k's stretch exactly when some earlier run of the stretch has
// L >= R. So (k, R) starts a tie exactly when R > P[k], P[k] = the largest L among the runs of k's stretch in front of k (0 for the
// stretch's first run) -- the bit k_bwt_f_run_flags takes from keys[j] != keys[j - 1]. tie[k] = (first run of k's stretch) << RUN_LBITS | L
// under a running maximum is (the same) << RUN_LBITS | max L of the stretch up to k, since the first runs do not decrease;
// k_bwt_f_run_emit reads P[k] from tie[k - 1].
constexpr int RUN_LBITS = 10;
static_assert(RUN_DIRECT_LMAX < (1u << RUN_LBITS), "a run length of the direct path fits the low bits of tie[]");
__global__ __launch_bounds__(256) void k_bwt_f_run_tie_marks(u32* __restrict__ tie, const u32* __restrict__ rcnt, u32 nRuns, u32 nsym)
{
    const u32 k = blockIdx.x * 256 + threadIdx.x;
    if (k >= nRuns) return;
    const u32 L = rcnt[k] + nsym - 1u;
    tie[k] = (tie[k] << RUN_LBITS) | (L < (1u << RUN_LBITS) ? L : (1u << RUN_LBITS) - 1u);
}

// The tie flags k_bwt_f_run_emit wrote, one byte per member, as the members' bit map (a word per thread); every bit from M up to the end
// of the last window is set (the end of the last tie), as k_bwt_f_run_flags leaves them. (The first build had k_bwt_f_run_emit OR the
// bits of every step into the map, up to three words by one lane: 1.14 ms for the kernel where the records took 0.63 -- a single-lane
// atomic is one memory-side request, and a step holds only the runs of a row that reach the column; profiles/r12_run_tables.txt.)
__global__ __launch_bounds__(256) void k_bwt_f_run_tie_bits(const u8* __restrict__ flags, u32 M, u32 nWords, u32* __restrict__ mbits)
{
    const u32 w = blockIdx.x * 256 + threadIdx.x;
    if (w >= nWords) return;
    const u32 j0 = 32u * w;
    u32 bits = 0;
    if (j0 + 32u <= M) {
        const u32x4 a = ldg<u32x4>(flags + j0), b = ldg<u32x4>(flags + j0 + 16);
        const u32 x[8] = { a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w };
#pragma unroll
        for (u32 i = 0; i < 8; i++) bits |= ((x[i] * 0x00204081u) >> 21 & 0xFu) << (4 * i);      // (bytes of 0 / 1: bit 0 of byte q to bit q)
    } else {
        for (u32 i = 0; i < 32; i++) bits |= ((j0 + i >= M || flags[j0 + i] != 0) ? 1u : 0u) << i;
    }
    mbits[w] = bits;
}

// bit i of `mask` ORed into bit pos + i of a bit map, as at most three word-wide atomics
__device__ __forceinline__ void or_mask64(u32* __restrict__ dst, u32 pos, unsigned long long mask)
{
    const u32 w0 = pos >> 5, sh = pos & 31;
    const u32 p0 = (u32)(mask << sh);
    const u32 p1 = sh ? (u32)(mask >> (32 - sh)) : (u32)(mask >> 32);
    const u32 p2 = sh ? (u32)(mask >> (64 - sh)) : 0u;
    if (p0) atomicOr(&dst[w0], p0);
    if (p1) atomicOr(&dst[w0 + 1], p1);
    if (p2) atomicOr(&dst[w0 + 2], p2);
}

__global__ __launch_bounds__(256) void k_bwt_f_run_tile_marks(const u32* __restrict__ segStart, u32 nRuns, u32* __restrict__ tileMark)
{
    const u32 k = blockIdx.x * 256 + threadIdx.x;
    if (k >= nRuns) return;
    tileMark[k] = ((k - segStart[k]) % RUN_TILE == 0) ? 1u : 0u;
}

__global__ __launch_bounds__(256) void k_bwt_f_run_tile_starts(const u32* __restrict__ segStart, const u32* __restrict__ tileIdx, u32 nRuns, u32* __restrict__ tileStart)
{
    const u32 k = blockIdx.x * 256 + threadIdx.x;
    if (k >= nRuns) return;
    const bool mark = (k - segStart[k]) % RUN_TILE == 0;
    const u32 t = tileIdx[k];
    if (mark) tileStart[t] = k;
    if (k + 1 == nRuns) tileStart[t + (mark ? 1u : 0u)] = nRuns;         // (the end of the last tile)
}

// tiles of segments of several tiles: colTab[slot][R] = #{runs of the tile with L >= R}
__global__ __launch_bounds__(256) void k_bwt_f_run_tile_counts(const u32* __restrict__ tileStart, const u32* __restrict__ segStart, const u32* __restrict__ rcnt, u32 nRuns,
                                                               const u32* __restrict__ nTilesDev, u32 nsym, u32* __restrict__ colTab)
{
    __shared__ u32 hist[RUN_COLS];
    __shared__ u32 wsum[4];
    const u32 t = blockIdx.x, tid = threadIdx.x;
    if (t >= *nTilesDev) return;
    const RunTile T = run_tile(tileStart, segStart, nRuns, t);
    if (!T.multi) return;
    for (u32 i = tid; i < RUN_COLS; i += 256) hist[i] = 0;
    __syncthreads();
    for (u32 k = T.k0 + tid; k < T.k1; k += 256) { const u32 L = rcnt[k] + nsym - 1u; atomicAdd(&hist[L < RUN_DIRECT_LMAX ? L : RUN_DIRECT_LMAX], 1u); }
    __syncthreads();
    u32 x[4], acc = 0;
#pragma unroll
    for (u32 i = 0; i < 4; i++) { x[i] = hist[4 * tid + i]; acc += x[i]; }
    u32 tot;
    const u32 incl = prims::sc_block_incl<prims::SCAN_SUM_EXCL>(acc, wsum, &tot);
    u32 ge = tot - (incl - acc);                                         // runs with L >= 4 tid
    u32* row = colTab + (size_t)T.slot * RUN_COLS;
#pragma unroll
    for (u32 i = 0; i < 4; i++) { row[4 * tid + i] = ge; ge -= x[i]; }
}

// the first tile of a segment of several tiles, for all of them: colTab[slot][R] = (members of the segment's columns in front of R) +
// (runs with L >= R of the segment's tiles in front of this one)
__global__ __launch_bounds__(256) void k_bwt_f_run_tile_scan(const u32* __restrict__ tileStart, const u32* __restrict__ segStart, const u64* __restrict__ sKey, u32 nRuns,
                                                             const u32* __restrict__ nTilesDev, u32 nsym, int kbits, u32* __restrict__ colTab)
{
    __shared__ u32 wsum[4];
    const u32 t0 = blockIdx.x, tid = threadIdx.x, nT = *nTilesDev;
    if (t0 >= nT) return;
    const RunTile T0 = run_tile(tileStart, segStart, nRuns, t0);
    if (!T0.multi || !T0.first) return;
    const bool above = ((sKey[T0.a] >> kbits) & 1ull) != 0;
    u32 A[4] = { 0, 0, 0, 0 };                                           // column R = tid + 256 c: runs of the segment with L >= R
    for (u32 t = t0; t < nT; t++) {
        const RunTile T = run_tile(tileStart, segStart, nRuns, t);
        const u32* row = colTab + (size_t)T.slot * RUN_COLS;
#pragma unroll
        for (u32 c = 0; c < 4; c++) A[c] += row[tid + 256 * c];
        if (T.last) break;
    }
    u32 P[4], carry = 0;                                                 // members of the columns up to R
#pragma unroll
    for (u32 c = 0; c < 4; c++) {
        if (tid + 256 * c < nsym) A[c] = 0;                              // (no such column)
        u32 tot;
        P[c] = carry + prims::sc_block_incl<prims::SCAN_SUM_EXCL>(A[c], wsum, &tot);
        carry += tot;
    }
    u32 run[4];
#pragma unroll
    for (u32 c = 0; c < 4; c++) run[c] = above ? carry - P[c] : P[c] - A[c];
    for (u32 t = t0; t < nT; t++) {
        const RunTile T = run_tile(tileStart, segStart, nRuns, t);
        u32* row = colTab + (size_t)T.slot * RUN_COLS;
#pragma unroll
        for (u32 c = 0; c < 4; c++) { const u32 x = row[tid + 256 * c]; row[tid + 256 * c] = run[c]; run[c] += x; }
        if (T.last) break;
    }
}

// one workgroup per tile, a wave per row of 64 runs. Member j of class di (the tile's: a tile lies in one segment) has the slot
// desc[di].x + (j - loff[di]): SA and ovr (R, what the doubling rounds need to look behind the run) are written there, and the member's
// tie flag (R > P, see k_bwt_f_run_tie_marks) is written as a byte, flags[j], which k_bwt_f_run_tie_bits packs into the members' bit map.
__global__ __launch_bounds__(256) void k_bwt_f_run_emit(const u32* __restrict__ tileStart, const u32* __restrict__ segStart, const u32* __restrict__ rcnt,
                                                        const u32* __restrict__ moff, const u64* __restrict__ sKey, const u32* __restrict__ sE, u32 nRuns, u32 M,
                                                        const u32* __restrict__ nTilesDev, const u32* __restrict__ colTab, u32 nsym, int kbits,
                                                        const uint2* __restrict__ desc, const u32* __restrict__ loff, const u32* __restrict__ tie,
                                                        u32* __restrict__ SA, u32* __restrict__ ovr, u8* __restrict__ flags)
{
    __shared__ u32 cnt[RUN_ROWS][RUN_CH];                                // runs of the row with L >= c0 + r, then the same of the rows in front
    __shared__ u32 colBase[RUN_CH];                                      // where column c0 + r of this tile starts in the segment
    __shared__ u32 wsum[4];
    __shared__ u32 sLmax;
    const u32 t = blockIdx.x, tid = threadIdx.x;
    if (t >= *nTilesDev) return;
    const int lane = lane_id();
    const u32 wave = tid >> 6;
    const RunTile T = run_tile(tileStart, segStart, nRuns, t);
    const u32 nRows = (T.k1 - T.k0 + 63) / 64;
    const u32 tileMembers = (T.k1 < nRuns ? moff[T.k1] : M) - moff[T.k0];     // (the segment's, when the tile is all of it)
    const u64 key0 = sKey[T.k0];
    const bool above = ((key0 >> kbits) & 1ull) != 0;
    const u32 di = (u32)(key0 >> (kbits + 1));
    const u32 segBase = moff[T.a];
    const u32 slotBase = desc[di].x - loff[di];                          // slot of member j: slotBase + j (mod 2^32)
    // my runs: wave w has the rows w, w + 4, ...
    u32 Lr[RUN_ROWS / 4], rowMax[RUN_ROWS / 4], e[RUN_ROWS / 4], Pr[RUN_ROWS / 4];
    u32 lmax = 0;
    if (tid == 0) sLmax = 0;
#pragma unroll
    for (u32 q = 0; q < RUN_ROWS / 4; q++) {
        const u32 k = T.k0 + (wave + 4 * q) * 64 + (u32)lane;
        Lr[q] = 0; e[q] = 0; Pr[q] = 0;
        if (k < T.k1) {
            Lr[q] = rcnt[k] + nsym - 1u;
            if (Lr[q] > RUN_DIRECT_LMAX) Lr[q] = RUN_DIRECT_LMAX;        // (the host sends no such batch here)
            e[q] = sE[k];
            if ((tie[k] >> RUN_LBITS) != k) Pr[q] = tie[k - 1] & ((1u << RUN_LBITS) - 1u);     // (not the first run of its stretch: k > 0)
        }
        rowMax[q] = wave_max(Lr[q]);
        lmax = rowMax[q] > lmax ? rowMax[q] : lmax;
    }
    __syncthreads();
    if (lane == 0) atomicMax(&sLmax, lmax);
    __syncthreads();
    const u32 Lmax = sLmax;
    u32 carry = 0;                                                       // members of the columns below c0 (a segment of one tile)
    for (u32 c0 = nsym; c0 <= Lmax; c0 += RUN_CH) {
        for (u32 i = tid; i < nRows * RUN_CH; i += 256) (&cnt[0][0])[i] = 0;
        __syncthreads();
#pragma unroll
        for (u32 q = 0; q < RUN_ROWS / 4; q++)
            if (Lr[q] >= c0) atomicAdd(&cnt[wave + 4 * q][Lr[q] - c0 < RUN_CH ? Lr[q] - c0 : RUN_CH - 1], 1u);
        __syncthreads();
        // per row: counts of L -> counts of L >= column
#pragma unroll
        for (u32 q = 0; q < RUN_ROWS / 4; q++) {
            const u32 row = wave + 4 * q;
            if (row >= nRows) break;
            u32 x[4], acc = 0;
#pragma unroll
            for (u32 i = 0; i < 4; i++) { x[i] = cnt[row][4 * lane + i]; acc += x[i]; }
            const u32 incl = wave_incl_scan(acc);
            const u32 tot = (u32)__shfl((int)incl, 63, 64);
            u32 ge = tot - (incl - acc);
#pragma unroll
            for (u32 i = 0; i < 4; i++) { cnt[row][4 * lane + i] = ge; ge -= x[i]; }
        }
        __syncthreads();
        // per column: the rows in front, and the column's place in the segment
        u32 colRuns = 0;
        for (u32 row = 0; row < nRows; row++) { const u32 x = cnt[row][tid]; cnt[row][tid] = colRuns; colRuns += x; }
        if (T.multi) {
            colBase[tid] = (c0 + tid < RUN_COLS) ? colTab[(size_t)T.slot * RUN_COLS + c0 + tid] : 0u;
        } else {
            u32 tot;
            const u32 P = carry + prims::sc_block_incl<prims::SCAN_SUM_EXCL>(colRuns, wsum, &tot);
            colBase[tid] = above ? tileMembers - P : P - colRuns;
            carry += tot;
        }
        __syncthreads();
#pragma unroll
        for (u32 q = 0; q < RUN_ROWS / 4; q++) {
            const u32 row = wave + 4 * q;
            if (row >= nRows) break;
            const u32 Rend = rowMax[q] < c0 + RUN_CH - 1 ? rowMax[q] : c0 + RUN_CH - 1;
            for (u32 R = c0; R <= Rend; R++) {
                const bool alive = Lr[q] >= R;
                const unsigned long long m = __ballot(alive);
                const u32 j = segBase + colBase[R - c0] + cnt[row][R - c0] + (u32)__popcll(m & __lanemask_lt());
                if (alive && j < M) {
                    const u32 mySlot = slotBase + j;
                    SA[mySlot] = e[q] - R;
                    ovr[mySlot] = R;
                    flags[j] = R > Pr[q] ? 1 : 0;
                }
            }
        }
        __syncthreads();
    }
}

// ---- the run round's last step without index arrays: where a tie starts among the sorted members is ONE BIT per member (a ballot per
// wave), the windows of 2048 members find their heads and sizes the way round 0 does (k_bwt_f_r0_winsum + two scans over the windows),
// and the placing kernel reads keys, positions and 64 words of bits -- where k_bwt_f_large_flags wrote two index arrays of the members'
// size and two device-wide scans ran over them.
// k_bwt_f_run_flags makes the bits of the member-sort path (a run longer than RUN_DIRECT_LMAX, the knob bwt_run_sort) from the members'
// sorted keys. The direct path has no keys: its bits come from the run tables (k_bwt_f_run_tie_marks, k_bwt_f_run_emit,
// k_bwt_f_run_tie_bits), and k_bwt_f_run_place<true> reads no record either.
__global__ __launch_bounds__(256) void k_bwt_f_run_flags(const u64* __restrict__ keys, u32 M, unsigned long long* __restrict__ bits64)
{
    const u32 j = blockIdx.x * 256 + threadIdx.x;
    const u64 k = (j < M) ? keys[j] : 0ull;
    u32 klo = (u32)__shfl_up((int)(u32)k, 1u, 64), khi = (u32)__shfl_up((int)(u32)(k >> 32), 1u, 64);
    u64 kp = ((u64)khi << 32) | klo;
    if ((threadIdx.x & 63) == 0 && j > 0 && j < M) kp = keys[j - 1];
    const bool f = (j >= M) || (j == 0) || (k != kp);                  // (every bit from M on is set: the end of the last tie)
    const unsigned long long m = __ballot(f);
    if ((threadIdx.x & 63) == 0) bits64[j >> 6] = m;
}

// DIRECT: the members were placed by k_bwt_f_run_emit -- SA and ovr are written, the bits are the ties; what is left is the labels and the
// descriptors. There are no member records then (keys, vals, memberR are null): the position is read from SA, and the class of a member
// is found in loff (nDesc + 1 entries), once per workgroup by bisection and from there by stepping.
template <bool DIRECT>
__global__ __launch_bounds__(256) void k_bwt_f_run_place(FwdView v, const uint2* __restrict__ desc, const u32* __restrict__ loff, u32 nDesc, u32 M, int kbits,
                                                         const u64* __restrict__ keys, const u32* __restrict__ vals, const u32* __restrict__ bits,
                                                         const u32* __restrict__ winLastIncl, const u32* __restrict__ winFirstInclRev, u32 nWin,
                                                         uint2* __restrict__ largeNext, const u32* __restrict__ memberR, u32* __restrict__ ovr,
                                                         u32* __restrict__ rtbits, const u32* __restrict__ lbase, int allLabels)
{
    // one member per thread (the kernel is a scatter of labels: occupancy is what hides its latency); the 64 words of the member's window of
    // 2048 are looked at by every one of the window's eight workgroups
    __shared__ SmWindow W;
    __shared__ ClassAgg A;
    __shared__ u32 sDi;
    const int tid = (int)threadIdx.x;
    const u32 jb = blockIdx.x * 256u;
    const u32 win = jb / SM_WIN, j0 = win * SM_WIN;
    agg_init(A);
    if (DIRECT && tid == 64) {
        u32 lo = 0, hi = nDesc;                                          // last class with loff <= jb (jb < M = loff[nDesc])
        while (hi - lo > 1) { const u32 mid = (lo + hi) >> 1; if (loff[mid] <= jb) lo = mid; else hi = mid; }
        sDi = lo;
    }
    if (tid < 64) {
        const u32 w = bits[(j0 >> 5) + (u32)tid];
        W.bw[tid] = w;
        int pm = w ? (tid * 32 + 31 - __clz((int)w)) : -1;
        u32 sm = w ? (u32)(tid * 32 + __ffs((int)w) - 1) : NO_BIT;
        for (int o = 1; o < 64; o <<= 1) {
            const int t = __shfl_up(pm, (unsigned)o, 64);
            if (tid >= o) pm = t > pm ? t : pm;
            const u32 u = (u32)__shfl_down((int)sm, (unsigned)o, 64);
            if (tid + o < 64) sm = u < sm ? u : sm;
        }
        int pex = __shfl_up(pm, 1u, 64);
        if (tid == 0) pex = -1;
        u32 sex = (u32)__shfl_down((int)sm, 1u, 64);
        if (tid == 63) sex = NO_BIT;
        W.prevSet[tid] = pex;
        W.nextSet[tid] = sex;
    }
    __syncthreads();
    const u32 j = jb + (u32)tid;
    u32 surv = 0, mySlot = 0, hLocal = 0, hSize = 0;
    int hKind = -1;
    bool setBit = false;
    if (j < M) {
        const u32 i = j - j0;
        const u32 w = i >> 5, bit = i & 31;
        const u32 lowmask = (bit == 31) ? 0xFFFFFFFFu : ((2u << bit) - 1u);
        const u32 word = W.bw[w];
        const u32 m = word & lowmask;
        const int si = m ? (int)(w * 32 + 31 - (u32)__clz((int)m)) : W.prevSet[w];
        const u32 nh = (si >= 0) ? j0 + (u32)si : (win ? winLastIncl[win - 1] : 0u);       // first member of my tie
        u32 di;
        if (DIRECT) { di = sDi; while (di + 1 < nDesc && j >= loff[di + 1]) di++; }
        else di = (u32)(keys[j] >> kbits);
        const u32 gs = desc[di].x, off = loff[di];
        mySlot = gs + (j - off);
        const u32 gp = DIRECT ? v.SA[mySlot] : vals[j];
        if (!DIRECT) v.SA[mySlot] = gp;
        // (the first tie of a group keeps the group's label, which round 0 wrote -- unless the members stayed out of its sort: allLabels)
        if (nh != off || allLabels) lab_set(v, gp, lbase[di], gs + (nh - off), gs);
        if (!DIRECT) ovr[mySlot] = memberR[j];                               // what the doubling rounds need to look behind the run
        if (nh == j) {
            const u32 m2 = word & ~lowmask;
            const u32 ei = m2 ? (w * 32 + (u32)__ffs((int)m2) - 1) : W.nextSet[w];
            u32 nxt = (ei != NO_BIT) ? j0 + ei : ((win + 1 < nWin) ? winFirstInclRev[nWin - 2 - win] : M);
            if (nxt > M) nxt = M;
            setBit = (j != off);
            hSize = nxt - j;
            hKind = agg_note(A, hSize, false, surv, hLocal);
        }
    }
    if (__ballot(surv != 0) != 0 && (tid & 63) == 0) v.counters[CNT_SMALL_LEFT] = 1;
    __syncthreads();
    if (tid == 0) agg_reserve(A, v);
    __syncthreads();
    if (hKind >= 0) agg_write(A, v, hKind, hLocal, mySlot, hSize, largeNext, (uint2*)nullptr);
    // bits: the lanes of a wave mostly hold consecutive slots (one group), so their bits leave as at most three word-wide ORs per wave
    const int lane = tid & 63;
    const bool live = j < M;
    const u32 s0 = (u32)__shfl((int)mySlot, 0, 64);
    const bool inLine = live && (mySlot == s0 + (u32)lane);
    const unsigned long long hm = __ballot(setBit && inLine), rm = __ballot(inLine);
    if (live && !inLine) {
        if (setBit) atomicOr(&v.gnew[mySlot >> 5], 1u << (mySlot & 31));
        atomicOr(&rtbits[mySlot >> 5], 1u << (mySlot & 31));
    }
    if (lane == 0) {
        if (hm) or_mask64(v.gnew, s0, hm);
        if (rm) or_mask64(rtbits, s0, rm);
    }
}

// end of a round: the group starts found in it become visible
__global__ __launch_bounds__(256) void k_bwt_f_merge_bits(u32* __restrict__ gbits, u32* __restrict__ gnew, u32 nWords)
{
    const u32 w = blockIdx.x * 256 + threadIdx.x;
    if (w >= nWords) return;
    const u32 x = gnew[w];
    if (x) { gbits[w] |= x; gnew[w] = 0; }
}

// ------------------------------------------------------------------------------------------------
// final: BWT bytes + header (BWTBlockCodec.cpp:58-86)
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_bwt_f_emit(BwtView v, const u32* __restrict__ base, const u8* __restrict__ ok, const u32* __restrict__ SA,
                                                    FwdView fv, u32* __restrict__ newLen)
{
    const int b = blockIdx.y;
    if (!ok[b]) return;
    const u32 n = v.len[b];
    u32 pIndexSize = 0;
    bwt_fwd_applies(n, v.cap[b], &pIndexSize);
    const int chunks = bwt_chunks(n);
    const u32 hdr = 1 + (u32)chunks * pIndexSize;
    const u8* s = v.src[b];
    u8* d = v.dst[b];
    const u32 bb = base[b];
    const u32 r0 = lab_cur(fv, bb, bb) - bb;               // rank of suffix 0
    // output byte q (hdr + 1 <= q < hdr + n) is the symbol in front of the suffix of rank r' = q - hdr - 1, ranks from r0 on moved
    // up by one (suffix 0 has nothing in front of it); a thread gathers the four bytes of one aligned dword of the output
    const u32 qLo = hdr + 1, qHi = hdr + n;
    const bool al = (reinterpret_cast<uintptr_t>(d) & 3) == 0;
    for (u32 w = (qLo >> 2) + blockIdx.x * 256 + threadIdx.x; 4 * w < qHi; w += gridDim.x * 256) {
        u32 word = 0, have = 0;
#pragma unroll
        for (u32 k = 0; k < 4; k++) {
            const u32 q = 4 * w + k;
            if (q >= qLo && q < qHi) {
                const u32 rr = q - qLo;
                const u32 r = rr + (rr >= r0 ? 1u : 0u);
                const u32 p = SA[bb + r] - bb;
                word |= (u32)s[p - 1] << (8 * k);
                have |= 1u << k;
            }
        }
        if (have == 0xF && al) reinterpret_cast<u32*>(d)[w] = word;
        else for (u32 k = 0; k < 4; k++) if ((have >> k) & 1) d[4 * w + k] = (u8)(word >> (8 * k));
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        d[hdr] = s[n - 1];
        const u32 st = n / (u32)chunks;
        const u32 step = ((u32)chunks * st == n) ? st : st + 1;
        const u32 logNbChunks = (u32)ilog2_u32((u32)chunks);
        d[0] = (u8)((logNbChunks << 2) | (pIndexSize - 1));
        u32 idx = 1;
        for (int k = 0; k < chunks; k++) {
            const u32 prim = lab_cur(fv, bb + (u32)k * step, bb) - bb;   // primaryIndex - 1
            for (int sh = (int)(pIndexSize - 1) * 8; sh >= 0; sh -= 8) d[idx++] = (u8)(prim >> sh);
        }
        newLen[b] = hdr + n;
    }
}

// ------------------------------------------------------------------------------------------------
// medium groups of the round that ends: the staging slots in order -> flags, (scan), descriptor list; the slots are cleared for the next round.
// The flags are two arrays behind each other, one per size class (up to MED_LO_CAP members, above), and ONE scan runs over both: a slot's
// place among its class is its prefix (less the lower class's count, for the upper one), its place in the list the sum of the two. The
// list is in slot order; idxLo / idxHi name, in slot order again, the list's descriptors of either class (k_bwt_f_medium_fused).
__global__ __launch_bounds__(256) void k_bwt_f_med_flags(const uint2* __restrict__ stage, u32 nSlots, u32* __restrict__ flags)
{
    const u32 i = blockIdx.x * 256 + threadIdx.x;
    if (i >= nSlots) return;
    const u32 n = stage[i].y;
    flags[i] = (n != 0 && n <= MED_LO_CAP) ? 1u : 0u;
    flags[nSlots + i] = (n > MED_LO_CAP) ? 1u : 0u;
}

// (at, atLo, atHi: what the list and the two indexes hold already -- the groups the probe appends to the first round's list)
__global__ __launch_bounds__(256) void k_bwt_f_med_compact(uint2* __restrict__ stage, u32 nSlots, const u32* __restrict__ prefix, uint2* __restrict__ medNext,
                                                           u32 at, u32* __restrict__ idxLo, u32 atLo, u32* __restrict__ idxHi, u32 atHi, u32* __restrict__ nLoOut)
{
    const u32 i = blockIdx.x * 256 + threadIdx.x;
    if (i >= nSlots) return;
    const u32 nLo = prefix[nSlots];                         // (the upper class's flags start there)
    if (i == 0) *nLoOut = nLo;
    const uint2 d = stage[i];
    if (d.y == 0) return;
    const u32 pLo = prefix[i], pHi = prefix[nSlots + i] - nLo, g = at + pLo + pHi;
    medNext[g] = d; stage[i] = make_uint2(0u, 0u);
    if (d.y <= MED_LO_CAP) idxLo[atLo + pLo] = g; else idxHi[atHi + pHi] = g;
}

// knobs (tests, diagnostics): read from the environment once per process, or set through knz_hip_tune(). Each one forces, at test
// sizes, a path that some inputs take by themselves (round-0 key length, no run round, the run groups' fall-back, the plain labels of
// blocks above 256 MiB, the plain keys of blocks above 8 MiB, where the link step starts), or reports (stats).
struct FwdTuning { int nsym; int noRunRound; int runFallback; int stats; int link; int plainLabels; int noPack; int noUnsplitSkip; int noGroupSleep; int noMediumFuse; int runSort; int runInSort; };
static FwdTuning& fwd_tuning()
{
    static FwdTuning t = [] {
        FwdTuning x; x.nsym = 0; x.noRunRound = 0; x.runFallback = 0; x.stats = 0; x.link = 1; x.plainLabels = 0; x.noPack = 0; x.noUnsplitSkip = 0; x.noGroupSleep = 0; x.noMediumFuse = 0; x.runSort = 0; x.runInSort = 0;     // link: 0 off, 1 on (from h = 32), n > 1: from h = n
        if (getenv("KNZ_BWT_PLAIN_LABELS")) x.plainLabels = 1;
        if (getenv("KNZ_BWT_NO_PACK")) x.noPack = 1;
        if (getenv("KNZ_BWT_NO_UNSPLIT_SKIP")) x.noUnsplitSkip = 1;
        if (getenv("KNZ_BWT_NO_GROUP_SLEEP")) x.noGroupSleep = 1;
        if (getenv("KNZ_BWT_NO_MEDIUM_FUSE")) x.noMediumFuse = 1;
        if (const char* e = getenv("KNZ_BWT_RUN_SORT")) x.runSort = atoi(e);
        if (const char* e = getenv("KNZ_BWT_RUN_IN_SORT")) x.runInSort = atoi(e);
        if (const char* e = getenv("KNZ_BWT_LINK")) x.link = atoi(e);
        if (getenv("KNZ_BWT_STATS")) x.stats = 1;
        if (const char* e = getenv("KNZ_BWT_NSYM")) x.nsym = atoi(e);
        if (getenv("KNZ_BWT_NO_RUN_ROUND")) x.noRunRound = 1;
        if (getenv("KNZ_BWT_RUN_FALLBACK")) x.runFallback = 1;
        return x;
    }();
    return t;
}
int bwt_forward_tune(const char* key, int value)
{
    FwdTuning& t = fwd_tuning();
    if (!strcmp(key, "rs_onesweep")) { prims::rs_onesweep_knob().store(value); return 0; }
    if (!strcmp(key, "bwt_nsym")) t.nsym = value;
    else if (!strcmp(key, "bwt_no_run_round")) t.noRunRound = value;
    else if (!strcmp(key, "bwt_run_fallback")) t.runFallback = value;
    else if (!strcmp(key, "bwt_stats")) t.stats = value;
    else if (!strcmp(key, "bwt_link")) t.link = value;
    else if (!strcmp(key, "bwt_plain_labels")) t.plainLabels = value;
    else if (!strcmp(key, "bwt_no_pack")) t.noPack = value;      // small groups ranked on plain keys (three counts per pair) also where the packed keys fit
    else if (!strcmp(key, "bwt_no_unsplit_skip")) t.noUnsplitSkip = value;      // medium groups whose keys are all equal stored and sorted like any other
    else if (!strcmp(key, "bwt_no_group_sleep")) t.noGroupSleep = value;        // every such group gathered in every round (no k_bwt_f_med_sleep, no records)
    else if (!strcmp(key, "bwt_no_medium_fuse")) t.noMediumFuse = value;        // medium groups through k_bwt_f_gather_desc and k_bwt_f_sort_medium on versioned labels too
    else if (!strcmp(key, "bwt_run_sort")) t.runSort = value;                   // 1: the run round's members generated and sorted (k_bwt_f_run_members, _expand), not placed directly
    else if (!strcmp(key, "bwt_run_in_sort")) t.runInSort = value;              // 1: the run members go through round 0's sort (no FwdSort::run_scan, no gaps)
    else return -1;
    return 0;
}

struct FwdScratch {
    u64* keysA; u64* keysB;
    u32* valsA; u32* valsB;
    u32* SA; u32* ISA; u32* K; u64* ISA2;
    u32* t0; u32* t1; u32* t2; u32* t3;
    u32* gbits; u32* gnew; u32* rtbits; u32* ovr; size_t gbitsWords;
    uint2* med[2]; uint2* medStage; uint2* medVerdict[2]; u32* medFlags; u32* medPrefix; u32* medIdxLo; u32* medIdxHi; size_t medSlots; uint2* descInfo; uint2* large[2]; uint2* runList; u32* ebits;
    u32* loff; u32* lbase;
    u32* survTile;       // members still tied after a round's small-group sort, per window
    u32* linkedTile;     // members the link step linked, per window
    u32* base;
    u32* counters;
    u32* seg2;
    void* scanTmp;
    void* rsMem;
    u32* byteHist;       // [nBlocks][256]
    // run round: class table, run-start bit map (+ counts, prefix), run tables
    u32* classTab; u32* rbits; u32* rcount; u32* rprefix;
    u32* runPos; u32* runE; u32* runL; u32* sE; u32* rcnt; u32* moff;
    u64* runKeysA; u64* runKeysB; u64* sKey;
    u32* runTileStart; u32* runColTab;      // direct placement of the members: first runs of the tiles, column tables of the segments of several tiles
    u32* gapMembers; u32* gapFirst; u32* gapStart; u32* cbase;      // run members kept out of round 0's sort: [nBlocks][256] each, and the compact segments' bases
    size_t maxRuns;
};

static size_t fwd_align(size_t x) { return (x + 255) & ~(size_t)255; }

static size_t fwd_carve(u8* p, int nBlocks, size_t total, FwdScratch* w, u32 VS)
{
    u8* q = p;
    auto take = [&](size_t sz) { u8* r = q; q += fwd_align(sz); return r; };
    // (twice the medium groups there can be: the list of the first round may hold groups k_bwt_f_probe took apart, void, beside their parts)
    const size_t maxMed = 2 * (total / (SM_G + 1) + 2), maxLarge = total / (MED_CAP + 1) + 2;
    w->gbitsWords = ((total + 64) / 64 + SM_WIN / 64 + 4) * 2 + 128;       // (the placement kernel looks 2 SM_TS slots behind a window's start)
    w->keysA = (u64*)take(8 * total); w->keysB = (u64*)take(8 * total);
    w->valsA = (u32*)take(4 * total); w->valsB = (u32*)take(4 * total);
    w->SA = (u32*)take(4 * total); w->ISA = (u32*)take(4 * total); w->K = (u32*)take(4 * total);
    w->ISA2 = (VS <= (1u << LAB_BITS)) ? (u64*)take(8 * total) : (u64*)nullptr;     // versioned labels (lab_old / lab_set; blocks up to 2^LAB_BITS bytes)
    w->t0 = (u32*)take(4 * total); w->t1 = (u32*)take(4 * total); w->t2 = (u32*)take(4 * total); w->t3 = (u32*)take(4 * total);
    w->gbits = (u32*)take(4 * w->gbitsWords);
    w->gnew = (u32*)take(4 * w->gbitsWords);
    w->rtbits = (u32*)take(4 * w->gbitsWords);
    w->ovr = (u32*)take(4 * total);
    w->med[0] = (uint2*)take(8 * maxMed); w->med[1] = (uint2*)take(8 * maxMed);
    w->medSlots = total / 256 + 2;
    w->medStage = (uint2*)take(8 * w->medSlots); w->medFlags = (u32*)take(8 * w->medSlots + 64); w->medPrefix = (u32*)take(8 * w->medSlots + 64);     // (two flags per slot: k_bwt_f_med_flags)
    w->medIdxLo = (u32*)take(4 * maxMed); w->medIdxHi = (u32*)take(4 * maxMed);
    w->medVerdict[0] = (uint2*)take(16 * w->medSlots); w->medVerdict[1] = w->medVerdict[0] + w->medSlots;
    w->large[0] = (uint2*)take(8 * maxLarge); w->large[1] = (uint2*)take(8 * maxLarge);
    w->runList = (uint2*)take(8 * maxMed);
    w->descInfo = (uint2*)take(8 * maxMed);
    w->ebits = (u32*)take(4 * w->gbitsWords);
    w->loff = (u32*)take(4 * (maxMed + 1));
    w->lbase = (u32*)take(4 * (maxMed + 1));
    w->survTile = (u32*)take(4 * (total / SM_TS + 64));
    w->linkedTile = (u32*)take(4 * (total / SM_TS + 64));
    w->base = (u32*)take(4ull * (nBlocks + 2));
    w->counters = (u32*)take(256);
    w->byteHist = (u32*)take(1024ull * (nBlocks + 1));
    w->seg2 = (u32*)take(64);
    w->scanTmp = take(prims::scan_tmp_bytes(total + 16));
    w->rsMem = take(prims::rs_ws_bytes(total, nBlocks + 1));
    w->maxRuns = total / 4 + 64;                                   // (runs of at least 4 symbols; with a shorter round-0 key there can be more: fallback)
    w->classTab = (u32*)take(1024ull * (size_t)nBlocks);
    const size_t rw = total / 32 + SM_WIN / 32 + 136;           // (+ the link step's bit map over the slots, whole windows)
    w->rbits = (u32*)take(4 * rw); w->rcount = (u32*)take(4 * rw); w->rprefix = (u32*)take(4 * rw);
    w->runPos = (u32*)take(4 * w->maxRuns); w->runE = (u32*)take(4 * w->maxRuns); w->runL = (u32*)take(4 * w->maxRuns);
    w->sE = (u32*)take(4 * w->maxRuns); w->rcnt = (u32*)take(4 * w->maxRuns); w->moff = (u32*)take(4 * w->maxRuns + 64);
    w->runKeysA = (u64*)take(8 * w->maxRuns); w->runKeysB = (u64*)take(8 * w->maxRuns); w->sKey = (u64*)take(8 * w->maxRuns);
    // direct placement: a tile per RUN_TILE runs or segment (4 bytes each), and RUN_COLS counts for each of the at most 2 maxRuns / RUN_TILE
    // tiles of segments of several tiles -- 8 * RUN_COLS / RUN_TILE = 8 bytes per run, 2 per byte of input, whatever the input holds
    w->runTileStart = (u32*)take(4 * w->maxRuns + 64);
    w->runColTab = (u32*)take(4ull * RUN_COLS * run_tile_slots(w->maxRuns));
    w->gapMembers = (u32*)take(1024ull * (size_t)nBlocks); w->gapFirst = (u32*)take(1024ull * (size_t)nBlocks); w->gapStart = (u32*)take(1024ull * (size_t)nBlocks);
    w->cbase = (u32*)take(4ull * (nBlocks + 2));
    return (size_t)(q - p);
}

size_t bwt_forward_scratch_bytes(int nBlocks, u32 VS, size_t total)
{
    FwdScratch w;
    return fwd_carve(nullptr, nBlocks, total, &w, VS) + 4096;
}

#define GRID1(n) dim3((unsigned)(((n) + 255) / 256)), dim3(256), 0, s

static int bits_for(u64 n, int lo) { while ((1ull << lo) < n) lo++; return lo; }     // the least b >= lo with 2^b >= n

// When the link step (k_bwt_f_link_small) runs, once the rounds are past the depth where most ties are chance. Whether it pays is a
// property of the data (it does where groups are whole repeats: copied spans, files that hold a part twice; it does not where every group
// has members that leave it one by one, as in the file mix of config 9): the first application, at h = 32, is a trial; what it linked
// against what was still tied after the round decides whether the rounds that follow apply it too, and every application is judged again.
// The trial is made on the windows of up to THREE WHOLE BLOCKS of the batch, the first, the middle and the last one (a run never leaves its
// block, so a block's runs are complete; a sample of windows all over the batch would cut every run), and must pay in each of them: 0.15 ms
// per 8 MiB where the step applied to a 212 MB batch costs 2-4 ms. (Round 5 looked at the first block only: in the real-file corpus that
// is one shared object, the trial said yes, and the application to the whole batch cost 3.5 ms for 1.7 ms of later rounds.)
struct LinkPlan {
    enum Mode { UNTRIED, TRIAL, ON, APPLIED, OFF } mode = UNTRIED;     // TRIAL, APPLIED: the step ran in the round before, to be judged
    int trials = 0; u32 retryH = 0xFFFFFFFFu;
    // judges the previous application by its payoff (members linked, their windows' members still tied) and decides this round's (true: run)
    bool next(u32 h, u32 survMembers, u32 total, u32 linked, u32 tied, bool stats)
    {
        if (mode == TRIAL || mode == APPLIED) {
            const bool paid = linked >= 4096 && tied < linked / 2;
            mode = paid ? ON : OFF;
            if (!paid) retryH = (trials < 2) ? h * 8 : 0xFFFFFFFFu;    // (chance ties of the early rounds may have hidden the repeats: once more, three rounds on)
            if (stats) fprintf(stderr, "link step: %u members linked, %u of the windows' members still tied after the round -> %s\n", linked, tied, paid ? "on" : "off");
        }
        if (mode == OFF && h >= retryH) mode = UNTRIED;
        if (mode == UNTRIED && survMembers >= total / 8) { mode = TRIAL; trials++; return true; }
        if (mode == ON && survMembers >= total / 64) { mode = APPLIED; return true; }
        return false;
    }
};

// One forward suffix sort, phase by phase (bwt_forward_run). A phase that reads the counters back (fetch) synchronises the stream: the
// phases after it size their launches by what came back.
struct FwdSort {
    hipStream_t s; const XfStage& st; u32* hp;            // hp: host copy of the counters, slot for slot (word 0: `total`, after the set-up)
    const FwdTuning tune = fwd_tuning();
    BwtView bv; FwdView v; FwdScratch w; size_t maxTotal;
    prims::RsWs rs1;                                       // the single-segment sorts of the rounds: [0, seg2[1])
    u32 total, medSlots, nTiles; int nsym, pbits, kbits;   // (tiles: windows of SM_TS slots)
    bool groupSleep = false;                               // medium groups sleep through rounds whose verdict is known (k_bwt_f_med_sleep)
    u32 h = 1; int cur = 0;                                // offset of the doubling round; its lists w.med[cur], w.large[cur] (the next round's: cur ^ 1)
    u64 *keysFree, *keysFree2;                             // key buffers of the rounds (keysFree2: round 0's sorted keys until they are placed)
    bool medFuse = false;                                  // medium groups through k_bwt_f_medium_fused (versioned labels; knob bwt_no_medium_fuse)
    bool runDirect = false;                                // the run round placed its members directly (k_bwt_f_run_emit; knob bwt_run_sort)
    bool gaps = false;                                     // the run members stay out of round 0's sort (run_scan; knob bwt_run_in_sort)
    u32 gapClasses = 0, keptOut = 0, scanRuns = 0, scanLongest = 0;     // what run_scan found: run groups, their members, runs of their bytes, longest run
    u32 r0Skipped = 0;                                     // workgroups of k_bwt_f_r0_flags that lay inside a gap (counted with the knob bwt_stats)
    u32 nMedLo = 0;                                        // descriptors of the lower size class among the nMed of the list
    u32 nRun, runElems, surv, nMed, nLarge, largeElems, survMembers;   // run groups of round 0 and their members; left: small groups (!= 0),
                                                                       // medium and large groups, large members, small members still tied
    LinkPlan link; LinkTrial linkTr; std::chrono::steady_clock::time_point statT;
    // counters [first, first + n) -> hp[first, first + n), then the stream synchronised
    int fetch(u32 first, u32 n) { return hipMemcpyAsync(hp + first, w.counters + first, 4 * (size_t)n, hipMemcpyDeviceToHost, s) == hipSuccess && hipStreamSynchronize(s) == hipSuccess ? 0 : -1; }
    void merge_bits() { hipLaunchKernelGGL(k_bwt_f_merge_bits, GRID1(total / 32 + 2), w.gbits, w.gnew, total / 32 + 2); }
    // the doubling rounds look max(R, h) positions on for the members of a group the run round left (FwdView::ovr, rtbits)
    void enable_run_tiebits() { if (!v.rtbits) { hipMemsetAsync(w.rtbits, 0, 4 * w.gbitsWords, s); v.ovr = w.ovr; v.rtbits = w.rtbits; } }
    // the medium groups staged by the kernels of a round -> descriptor list `dst` (in slot order) behind the `at` it holds, the indexes of
    // its two size classes behind their atLo and at - atLo entries; CNT_MED and CNT_MED_LO count what was added
    void compact_medium(uint2* dst, u32 at = 0, u32 atLo = 0)
    {
        KScope ks_("k_bwt_f_med_compact");
        hipLaunchKernelGGL(k_bwt_f_med_flags, GRID1(medSlots), w.medStage, medSlots, w.medFlags);
        prims::launch_scan<prims::SCAN_SUM_EXCL>(s, w.medFlags, w.medPrefix, 2 * (size_t)medSlots, nullptr, w.scanTmp, w.counters + CNT_MED);
        hipLaunchKernelGGL(k_bwt_f_med_compact, GRID1(medSlots), w.medStage, medSlots, w.medPrefix, dst, at, w.medIdxLo, atLo, w.medIdxHi, at - atLo, w.counters + CNT_MED_LO);
    }
    // running maximum of t0 into t1 (the last group start at or before an element; `last`) and running minimum of t2 into t3 (the first
    // one at or after it, mirrored) over n values; with a bit map over `len` elements, t0 / t2 are first taken per window of `wordsPerWin` words
    void bounds(u32 n, bool last, const u32* bits = nullptr, u32 len = 0, u32 wordsPerWin = 0)
    {
        if (bits) { KScope ks_("k_bwt_f_r0_winsum"); hipLaunchKernelGGL(k_bwt_f_r0_winsum, GRID1(n), bits, len, n, w.t0, w.t2, wordsPerWin); }
        if (last) { KScope ks_("k_bwt_f_scan_max"); prims::launch_scan<prims::SCAN_MAX_INCL>(s, w.t0, w.t1, n, nullptr, w.scanTmp); }
        KScope ks_("k_bwt_f_scan_min"); prims::launch_scan<prims::SCAN_MIN_INCL>(s, w.t2, w.t3, n, nullptr, w.scanTmp);
    }
    // a sort of n keys as one segment; 0: the result is in (ka, va), 1: in (kb, vb)
    template <class KEY, bool HAS_VAL> int sort_one_segment(u32 n, KEY* ka, KEY* kb, u32* va, u32* vb, int loBit, int hiBit, bool oneRead = true)
    {
        hipLaunchKernelGGL(prims::k_rs_one_segment, dim3(1), dim3(64), 0, s, w.seg2, n);
        prims::rs_launch_layout(s, rs1);
        return prims::rs_sort<KEY, HAS_VAL>(s, rs1, ka, kb, va, vb, (size_t)n, loBit, hiBit, oneRead);
    }
    // bases of the blocks, byte histograms and the round-0 key length; `total` read back (0: nothing to sort)
    int setup(void* scratch, size_t scratchBytes, BwtSuffixArrays* sa)
    {
        bv.src = st.src; bv.dst = st.dst; bv.len = st.len; bv.cap = st.cap; bv.VS = st.maxLen; bv.nBlocks = st.nBlocks;
        maxTotal = (size_t)st.nBlocks * bv.VS;
        if (fwd_carve(reinterpret_cast<u8*>(scratch), st.nBlocks, maxTotal, &w, bv.VS) > scratchBytes) return -2;
        { KScope ks_("k_bwt_f_bases"); hipLaunchKernelGGL(k_bwt_bases, dim3(1), dim3(64), 0, s, bv, w.base, st.ok, w.counters + CNT_LONGEST_BLOCK, sa ? 1 : 0); }
        hipMemsetAsync(st.newLen, 0, sizeof(u32) * st.nBlocks, s);
        { KScope ks_("k_bwt_f_r0_hist");                                // byte histograms: the key length of round 0, later its digit counts
          hipMemsetAsync(w.byteHist, 0, 1024ull * st.nBlocks, s);
          hipLaunchKernelGGL(k_bwt_f_bytehist, dim3(64, (unsigned)st.nBlocks), dim3(256), 0, s, bv, w.base, w.byteHist);
          hipLaunchKernelGGL(k_bwt_f_choose_nsym, dim3(1), dim3(256), 0, s, w.byteHist, st.nBlocks, w.counters + CNT_LONGEST_BLOCK, w.counters + CNT_NSYM); }
        if (hipMemcpyAsync(hp, w.base + st.nBlocks, 4, hipMemcpyDeviceToHost, s) != hipSuccess || fetch(CNT_LONGEST_BLOCK, 2)) return -1;
        total = hp[0];
        if (sa) { sa->SA = w.SA; sa->base = w.base; sa->total = total; }
        if (total == 0) return 0;
        v.base = w.base; v.nBlocks = st.nBlocks; v.total = total; v.SA = w.SA; v.ISA = w.ISA; v.K = w.K; v.ISA2 = (w.ISA2 != nullptr && !tune.plainLabels) ? w.ISA2 : (u64*)nullptr;
        v.round = 0; v.gbits = w.gbits; v.gnew = w.gnew; v.counters = w.counters; v.medStage = w.medStage; v.ovr = nullptr; v.rtbits = nullptr;
        v.verdictNow = nullptr; v.verdictWas = nullptr;
        medSlots = (u32)((size_t)total / 256 + 1); nTiles = (total + SM_TS - 1) / SM_TS;
        survMembers = total;                                          // (not counted before the first round: assume many)
        hipMemsetAsync(w.medStage, 0, 8ull * w.medSlots, s);
        medFuse = v.ISA2 != nullptr && !tune.noMediumFuse;
        groupSleep = !tune.noUnsplitSkip && !tune.noGroupSleep;      // (the records are the verdicts of the unsplit skip)
        if (groupSleep) hipMemsetAsync(w.medVerdict[0], 0, 16ull * w.medSlots, s);      // (round 0 in every record: no round reads that)
        pbits = bits_for(hp[CNT_LONGEST_BLOCK], 1);                   // positions inside the longest block the transform applies to
        // Four or five symbols (as many as fit the key beside the position when the block is larger than 8 / 16 MiB), by the batch's order-0
        // entropy (k_bwt_f_choose_nsym). Measured on 212 MB with 8 MiB blocks, MB/s of the whole round trip, round 3: 4 symbols 4437 (mixed
        // stand-in) / 3859 (text); 5 symbols with h = 5, 10, ...: 4243 / 4155; 5 symbols with h = 4, 8, ...: 4319 / 3970. Round 4 (the
        // doubling offsets stay 4, 8, ...): 4 symbols 5034 / 4314, 5 symbols 4961 / 4564 -- text likes the deeper first round, the stand-in
        // (periodic and sparse stretches, noise) gains nothing from it and pays the fifth pass.
        const int fit = (64 - pbits) / 8, want = (hp[CNT_NSYM] == 5u) ? 5 : 4;
        nsym = fit < want ? fit : want;
        if (tune.nsym >= 1) nsym = tune.nsym < fit ? tune.nsym : fit;   // tuning knob: other round-0 key lengths
        if (nsym < 1) return -4;
        // The doubling starts at the largest power of two the round-0 depth covers (groups and labels of depth nsym >= h are what a round
        // with offset h needs): h = 4, 8, 16, ... meets the periods real data has (record and row sizes are powers of two more often than
        // not), which is what lets the chain round (med_chain_round) see a group look at itself.
        while (2 * h <= (u32)nsym) h <<= 1;
        return 0;
    }
    // 30-bit counts in the look-back words (a 1 GiB block: count + scatter)
    bool one_read() const { return prims::rs_onesweep_knob().load() != 0 && nsym <= prims::RS_MAXPASS && (size_t)bv.VS < (size_t)prims::RS_VAL_MASK; }
    // The run groups found in the text before round 0 sorts anything, so that their members can stay out of the sort (see TextSrcKept): the
    // run round's own first steps -- run ends, run lengths (R stays in w.K until the run round has read it), the runs of run-group bytes
    // compacted -- with the members counted per (block, byte) on the way. Everything the run round could fall back on is known after the
    // one read-back, which is the run round's, moved here: `gaps` is set only when it will take every run group.
    int run_scan()
    {
        gaps = false; keptOut = 0;
        kbits = bits_for((u64)bv.VS + 2, 1);
        if (tune.noRunRound || tune.runFallback || tune.runInSort || (2 * kbits + 1) >= 64 || !one_read() || nsym < 2) return 0;
        const u32 nWin = (total + SM_WIN - 1) / SM_WIN, nRW = nWin * (SM_WIN / 32);
        hipMemsetAsync(w.counters, 0, 4 * (CNT_GAP_MEMBERS + 1), s);
        hipMemsetAsync(w.gapMembers, 0, 1024ull * (size_t)st.nBlocks, s); hipMemsetAsync(w.gapFirst, 0xFF, 1024ull * (size_t)st.nBlocks, s);
        { KScope ks_("k_bwt_f_run_ends"); hipLaunchKernelGGL(k_bwt_f_run_ends, dim3(nWin), dim3(256), 0, s, bv, v, reinterpret_cast<u8*>(w.ebits)); }
        bounds(nWin, false, w.ebits, total, SM_WIN / 32);
        { KScope ks_("k_bwt_f_run_len"); hipLaunchKernelGGL(k_bwt_f_run_len<true>, dim3(nWin), dim3(256), 0, s, bv, v, w.ebits, w.t3, nWin, w.K, (const u32*)nullptr, (u32)nsym,
                                                            reinterpret_cast<unsigned long long*>(w.rbits), w.rcount, w.gapMembers, w.gapFirst); }
        { KScope ks_("k_bwt_f_run_scan_classes");
          hipLaunchKernelGGL(k_bwt_f_run_scan_classes, dim3(1), dim3(256), 0, s, w.gapMembers, w.classTab, w.base, w.cbase, st.nBlocks, w.counters);
          hipLaunchKernelGGL(k_bwt_f_run_starts, GRID1(nRW), bv, v, w.rbits, nRW, w.classTab, w.rcount); }
        { KScope ks_("k_bwt_f_scan_sum"); prims::launch_scan<prims::SCAN_SUM_EXCL>(s, w.rcount, w.rprefix, nRW, nullptr, w.scanTmp, w.counters + CNT_RUNS); }
        { KScope ks_("k_bwt_f_run_compact"); hipLaunchKernelGGL(k_bwt_f_run_compact, GRID1(nRW), w.rbits, w.rprefix, nRW, w.runPos); }
        if (fetch(CNT_RUN_LONGEST, CNT_GAP_MEMBERS + 1 - CNT_RUN_LONGEST)) return -1;
        gapClasses = hp[CNT_GAP_CLASSES]; scanRuns = hp[CNT_RUNS]; scanLongest = hp[CNT_RUN_LONGEST];
        // (the conditions of run_round's fall-backs, with the groups round 0 is going to list)
        const int hbits = bits_for((u64)scanLongest + 1, 1) + 1, rbits = bits_for(gapClasses, 0), idxBits = bits_for(scanRuns, 1);
        if (gapClasses == 0 || (u64)gapClasses > (1ull << (64 - (2 * kbits + 1)))) return 0;
        if (scanRuns == 0 || scanRuns > w.maxRuns || rbits + hbits > 32 || idxBits + kbits + 1 + rbits > 64) return 0;
        gaps = true; keptOut = hp[CNT_GAP_MEMBERS];
        return 0;
    }
    // round 0's sort without the run members: compact segments up to the last pass, which leaves the gaps; the gaps filled
    void round0_sort_gaps(const prims::RsWs& rs)
    {
        const prims::RsWs rsC = prims::rs_carve(w.rsMem, maxTotal, st.nBlocks + 1, w.cbase, st.nBlocks);      // (the same memory: one layout at a time)
        u64* kin = w.keysA; u64* kout = w.keysB;
        KScope ks_("k_bwt_f_r0_sort");
        hipLaunchKernelGGL(k_bwt_f_r0_counts, dim3((unsigned)rs.L.nSeg), dim3(256), 0, s, bv, w.base, w.byteHist, nsym, rs.L, w.gapMembers);
        hipLaunchKernelGGL(k_bwt_f_r0_bases, dim3((unsigned)rs.L.nSeg, (unsigned)nsym), dim3(256), 0, s, rs.L, w.base, w.cbase, nsym, w.gapMembers, w.gapStart);
        for (int pass = 0; pass < nsym; pass++) {
            if (pass == 0) {                                          // reads every position of the blocks (layout: base), keeps the others
                TextSrcKept src; src.src = bv.src; src.P = nsym; src.pbits = pbits; src.shift = pbits; src.members = w.gapMembers;
                prims::rs_launch_pass_os<u64, false>(s, rs, src, nullptr, kout, nullptr, (size_t)bv.VS, pass);
                prims::rs_launch_layout(s, rsC);
            } else if (pass + 1 < nsym) {
                prims::DigitOfKey<u64> src; src.keys = kin; src.shift = pbits + 8 * pass; src.mask = 255u;
                prims::rs_launch_pass_os<u64, false>(s, rsC, src, nullptr, kout, nullptr, (size_t)bv.VS, pass);
            } else {
                LastPassSrc src; src.keys = kin; src.shift = pbits + 8 * pass; src.mask = 255u; src.members = w.gapMembers; src.gapStart = w.gapStart; src.P = nsym; src.pbits = pbits;
                prims::rs_launch_pass_os<u64, false>(s, rsC, src, nullptr, kout, nullptr, (size_t)bv.VS, pass);
            }
            std::swap(kin, kout);
        }
        hipLaunchKernelGGL(k_bwt_f_r0_fill, dim3(256, (unsigned)st.nBlocks), dim3(256), 0, s, kin, w.gapMembers, w.gapStart, w.gapFirst, nsym, pbits);
        keysFree = kout; keysFree2 = kin;
    }
    // Round 0: the suffixes of every block sorted by their first nsym symbols. Keys = [nsym bytes | position in the block]; one stable LSD
    // pass per symbol, the first one reads the text, the blocks are the segments of the sort.
    void round0_sort()
    {
        const prims::RsWs rs = prims::rs_carve(w.rsMem, maxTotal, st.nBlocks + 1, w.base, st.nBlocks);
        rs1 = prims::rs_carve(w.rsMem, maxTotal, st.nBlocks + 1, w.seg2, 1);
        { KScope ks_("k_bwt_f_r0_layout"); prims::rs_launch_layout(s, rs); }
        u64* kin = w.keysA; u64* kout = w.keysB;
        const bool oneRead = one_read();
        if (gaps) { round0_sort_gaps(rs); return; }
        if (oneRead) {                                                // the digits of all passes counted from the text, once
            KScope ks_("k_bwt_f_r0_sort");
            hipLaunchKernelGGL(k_bwt_f_r0_counts, dim3((unsigned)rs.L.nSeg), dim3(256), 0, s, bv, w.base, w.byteHist, nsym, rs.L, (const u32*)nullptr);
            hipLaunchKernelGGL(prims::k_rs_digit_bases, dim3((unsigned)rs.L.nSeg, (unsigned)nsym), dim3(256), 0, s, rs.L);
        }
        auto sortPass = [&](const auto& src, int pass) {
            if (oneRead) prims::rs_launch_pass_os<u64, false>(s, rs, src, nullptr, kout, nullptr, (size_t)bv.VS, pass);
            else prims::rs_launch_pass<u64, false>(s, rs, src, nullptr, kout, nullptr, (size_t)bv.VS);
        };
        for (int pass = 0; pass < nsym; pass++) {
            KScope ks_("k_bwt_f_r0_sort");
            if (pass == 0) { TextSrc src; src.src = bv.src; src.P = nsym; src.pbits = pbits; src.shift = pbits; sortPass(src, pass); }
            else { prims::DigitOfKey<u64> src; src.keys = kin; src.shift = pbits + 8 * pass; src.mask = 255u; sortPass(src, pass); }
            std::swap(kin, kout);
        }
        keysFree = kout; keysFree2 = kin;                             // (the last pass wrote into what is now `kin`)
    }
    // Round 0's groups from its sorted keys: the small ones refined on the text behind the key, the others listed, the run groups apart
    int round0_place()
    {
        // every bit from `total` on is set (end sentinel, and windows may look past the end)
        hipMemsetAsync(w.gbits, 0xFF, 4 * w.gbitsWords, s); hipMemsetAsync(w.gnew, 0, 4 * w.gbitsWords, s);
        hipMemsetAsync(w.counters, 0, 4 * CNT_ROUND_SLOTS, s);
        { KScope ks_("k_bwt_f_r0_flags"); hipLaunchKernelGGL(k_bwt_f_r0_flags, dim3((total + 256 * R0F_ROWS - 1) / (256 * R0F_ROWS)), dim3(256), 0, s, keysFree2, w.base, st.nBlocks, total, nsym, pbits,
                                                             reinterpret_cast<unsigned long long*>(w.gbits), gaps ? w.gapMembers : (const u32*)nullptr, w.gapStart,
                                                             tune.stats ? w.counters + CNT_STAT_R0_SKIPPED : (u32*)nullptr); }
        // group starts before / after every window of SM_TS slots (the windows of the placement): two scans over ~total/1792 values
        bounds(nTiles, true, w.gbits, total, SM_TS / 32);
        kbits = bits_for((u64)bv.VS + 2, 1);
        // the run-length round needs descriptor index + (kbits + 1) + kbits bits in one 64-bit key
        // (2 * kbits + 1 >= 64 needs VS >= 2^31 - 1: no block of an encode, only a per-stage call, knz_hip_transform_forward, with n or dst_cap
        // that close to 2 GiB)
        const bool runRound = (2 * kbits + 1) < 64 && !tune.noRunRound;
        { KScope ks_("k_bwt_f_r0_place");
          hipLaunchKernelGGL(k_bwt_f_r0_place_text, dim3(nTiles), dim3(256), 0, s, bv, v, w.t1, w.t3, nTiles, w.large[cur], keysFree2, nsym, pbits, runRound ? w.runList : (uint2*)nullptr,
                             gaps ? w.classTab : (const u32*)nullptr, w.gapMembers, w.gapStart);
          merge_bits(); }
        if (fetch(0, CNT_ROUND_SLOTS)) return -1;
        nRun = hp[CNT_RUN]; runElems = hp[CNT_RUN_MEMBERS]; r0Skipped = hp[CNT_STAT_R0_SKIPPED];
        return 0;
    }
    // the run groups go the ordinary way (the medium and large lists)
    int run_fallback()
    {
        { KScope ks_("k_bwt_f_run_fallback"); hipLaunchKernelGGL(k_bwt_f_run_fallback, GRID1(nRun), v, w.runList, nRun, w.med[cur], w.large[cur]); }
        nRun = 0; return fetch(0, CNT_ROUND_SLOTS);
    }
    // Run round: the run groups of round 0 (4 equal symbols) in one round by run length: the run lengths of every position (text order),
    // the runs sorted, then one sort of the members on (run length, what follows)
    int run_round()
    {
        // more run groups than the key has index bits left for (thousands of blocks in one batch; the knob: tests force this path)
        if (nRun && ((u64)nRun > (1ull << (64 - (2 * kbits + 1))) || tune.runFallback) && run_fallback()) return -1;
        if (gaps) {
            // run_scan has done the steps up to the read-back, and knows that none of the fall-backs applies; round 0 must have listed the
            // groups it counted. The class table gets the descriptor indexes.
            if (nRun != gapClasses || runElems != keptOut) return -1;
            { KScope ks_("k_bwt_f_run_classes"); hipLaunchKernelGGL(k_bwt_f_run_classes, GRID1(nRun), bv, v, w.runList, nRun, w.classTab); }
            return run_round_sorted(scanRuns, scanLongest);
        }
        if (!nRun) return 0;
        const u32 nWin = (total + SM_WIN - 1) / SM_WIN;          // (windows of 2048 positions)
        { KScope ks_("k_bwt_f_run_ends"); hipLaunchKernelGGL(k_bwt_f_run_ends, dim3(nWin), dim3(256), 0, s, bv, v, reinterpret_cast<u8*>(w.ebits)); }
        bounds(nWin, false, w.ebits, total, SM_WIN / 32);
        // run lengths of every position, and the starts of the runs of run-group bytes as a bit map
        hipMemsetAsync(w.classTab, 0xFF, 1024ull * (size_t)st.nBlocks, s);
        { KScope ks_("k_bwt_f_run_classes"); hipLaunchKernelGGL(k_bwt_f_run_classes, GRID1(nRun), bv, v, w.runList, nRun, w.classTab); }
        { KScope ks_("k_bwt_f_run_len"); hipLaunchKernelGGL(k_bwt_f_run_len<false>, dim3(nWin), dim3(256), 0, s, bv, v, w.ebits, w.t3, nWin, w.K, w.classTab, (u32)nsym,
                                                            reinterpret_cast<unsigned long long*>(w.rbits), w.rcount, (u32*)nullptr, (u32*)nullptr); }
        // the runs themselves, compacted in position order (the windows of k_bwt_f_run_len cover whole words up to nWin * 2048)
        const u32 nRW = nWin * (SM_WIN / 32);
        { KScope ks_("k_bwt_f_scan_sum"); prims::launch_scan<prims::SCAN_SUM_EXCL>(s, w.rcount, w.rprefix, nRW, nullptr, w.scanTmp, w.counters + CNT_RUNS); }
        { KScope ks_("k_bwt_f_run_compact"); hipLaunchKernelGGL(k_bwt_f_run_compact, GRID1(nRW), w.rbits, w.rprefix, nRW, w.runPos); }
        if (fetch(CNT_RUN_LONGEST, 3)) return -1;
        return run_round_sorted(hp[CNT_RUNS], hp[CNT_RUN_LONGEST]);
    }
    // the rest of the run round: nRuns runs of run-group bytes in w.runPos, R in w.K, the class table filled
    int run_round_sorted(const u32 nRuns, const u32 longest)
    {
        const int hbits = bits_for((u64)longest + 1, 1) + 1;     // (+ 1: both halves of the order: R and 2^hbits - 1 - R)
        const int rbits = bits_for(nRun, 0), idxBits = bits_for(nRuns, 1);
        // more runs than the tables hold (a round-0 key shorter than 4 symbols) or fields that do not fit their words: the ordinary way
        if (nRuns == 0 || nRuns > w.maxRuns || rbits + hbits > 32 || idxBits + kbits + 1 + rbits > 64) return gaps ? -1 : run_fallback();
        { KScope ks_("k_bwt_f_large_prefix"); hipLaunchKernelGGL(k_bwt_f_large_prefix, dim3(1), dim3(1024), 0, s, w.runList, nRun, w.loff, w.base, st.nBlocks, w.lbase); }
        { KScope ks_("k_bwt_f_run_table"); hipLaunchKernelGGL(k_bwt_f_run_table, GRID1(nRuns), bv, v, w.runPos, nRuns, w.K, w.classTab, kbits, idxBits, w.runKeysA, w.runE, w.runL,
                                                              gaps ? w.runList : (const uint2*)nullptr, (u32)nsym); }
        const u64* rkSorted;
        { KScope ks_("k_bwt_f_sort_runs");
          rkSorted = sort_one_segment<u64, false>(nRuns, w.runKeysA, w.runKeysB, nullptr, nullptr, idxBits, idxBits + kbits + 1 + rbits) ? w.runKeysB : w.runKeysA; }
        { KScope ks_("k_bwt_f_run_sorted"); hipLaunchKernelGGL(k_bwt_f_run_sorted, GRID1(nRuns), rkSorted, nRuns, idxBits, w.runE, w.runL, (u32)nsym, w.sE, w.sKey, w.rcnt); }
        { KScope ks_("k_bwt_f_scan_sum"); prims::launch_scan<prims::SCAN_SUM_EXCL>(s, w.rcnt, w.moff, nRuns, nullptr, w.scanTmp); }
        u64* rk = nullptr; u32* rv = w.valsA;
        u32* mbits = w.ebits; const u32 nWinM = (runElems + SM_WIN - 1) / SM_WIN;     // (the members' bit map reuses the run-end map, which nobody reads any more)
        runDirect = !tune.runSort && longest <= RUN_DIRECT_LMAX && idxBits + RUN_LBITS <= 32;
        if (runDirect) {
            // the members placed without a sort (k_bwt_f_run_emit): segments and tiles of the sorted runs, the column tables of the segments
            // of several tiles, the records. The tables of the unsorted runs are free by now: runPos holds the segments' first runs, runE
            // the tiles' numbers. One workgroup per tile there can be: a segment's last tile may be short, and there are two segments per class.
            KScope ks_("k_bwt_f_run_direct");
            u32* segStart = w.runPos; u32* tileIdx = w.runE; u32* tie = w.runL;
            u8* flags = reinterpret_cast<u8*>(keysFree);                // (a byte per member; round 0's sorted keys, keysFree2, are placed by now, too)
            const u32 maxTiles = (u32)std::min<u64>((u64)nRuns, 2ull * nRun + nRuns / RUN_TILE + 1);
            hipLaunchKernelGGL(k_bwt_f_run_seg_marks, GRID1(nRuns), w.sKey, nRuns, kbits, segStart, tie);
            prims::launch_scan<prims::SCAN_MAX_INCL>(s, segStart, segStart, nRuns, nullptr, w.scanTmp);
            prims::launch_scan<prims::SCAN_MAX_INCL>(s, tie, tie, nRuns, nullptr, w.scanTmp);
            hipLaunchKernelGGL(k_bwt_f_run_tie_marks, GRID1(nRuns), tie, w.rcnt, nRuns, (u32)nsym);
            prims::launch_scan<prims::SCAN_MAX_INCL>(s, tie, tie, nRuns, nullptr, w.scanTmp);
            hipLaunchKernelGGL(k_bwt_f_run_tile_marks, GRID1(nRuns), segStart, nRuns, tileIdx);
            prims::launch_scan<prims::SCAN_SUM_EXCL>(s, tileIdx, tileIdx, nRuns, nullptr, w.scanTmp, w.counters + CNT_RUN_TILES);
            hipLaunchKernelGGL(k_bwt_f_run_tile_starts, GRID1(nRuns), segStart, tileIdx, nRuns, w.runTileStart);
            if (nRuns > RUN_TILE) {                                     // (no segment of several tiles otherwise)
                hipLaunchKernelGGL(k_bwt_f_run_tile_counts, dim3(maxTiles), dim3(256), 0, s, w.runTileStart, segStart, w.rcnt, nRuns, w.counters + CNT_RUN_TILES, (u32)nsym, w.runColTab);
                hipLaunchKernelGGL(k_bwt_f_run_tile_scan, dim3(maxTiles), dim3(256), 0, s, w.runTileStart, segStart, w.sKey, nRuns, w.counters + CNT_RUN_TILES, (u32)nsym, kbits, w.runColTab);
            }
            hipLaunchKernelGGL(k_bwt_f_run_emit, dim3(maxTiles), dim3(256), 0, s, w.runTileStart, segStart, w.rcnt, w.moff, w.sKey, w.sE, nRuns, runElems, w.counters + CNT_RUN_TILES,
                               w.runColTab, (u32)nsym, kbits, w.runList, w.loff, tie, w.SA, w.ovr, flags);
            hipLaunchKernelGGL(k_bwt_f_run_tie_bits, GRID1(nWinM * (SM_WIN / 32)), flags, runElems, nWinM * (SM_WIN / 32), mbits);
        } else {
            { KScope ks_("k_bwt_f_run_members"); hipLaunchKernelGGL(k_bwt_f_run_members, dim3((runElems + 2047) / 2048), dim3(256), 0, s, w.moff, nRuns, runElems, w.sKey, kbits, hbits,
                                                                    (u32)nsym, keysFree); }
            { KScope ks_("k_bwt_f_sort_members");
              const int r = sort_one_segment<u64, false>(runElems, keysFree, keysFree2, nullptr, nullptr, 32, 32 + hbits + rbits);
              rk = r ? keysFree : keysFree2;
              hipLaunchKernelGGL(k_bwt_f_run_expand, GRID1(runElems), r ? keysFree2 : keysFree, runElems, w.sKey, w.sE, kbits, hbits, rk, rv, w.valsB); }
            // ties among the sorted members as a bit map (the direct path has written its own: k_bwt_f_run_tie_marks, k_bwt_f_run_emit)
            KScope ks_("k_bwt_f_large_flags");
            hipLaunchKernelGGL(k_bwt_f_run_flags, dim3(nWinM * (SM_WIN / 256)), dim3(256), 0, s, rk, runElems, reinterpret_cast<unsigned long long*>(mbits));
        }
        // heads and sizes per window of 2048 members
        bounds(nWinM, true, mbits, runElems, SM_WIN / 32);
        { KScope ks_("k_bwt_f_large_place");
          hipMemsetAsync(w.rtbits, 0, 4 * w.gbitsWords, s);
          if (runDirect)
              hipLaunchKernelGGL(k_bwt_f_run_place<true>, dim3((runElems + 255) / 256), dim3(256), 0, s, v, w.runList, w.loff, nRun, runElems, hbits + kbits, (const u64*)nullptr,
                                 (const u32*)nullptr, mbits, w.t1, w.t3, nWinM, w.large[cur], (const u32*)nullptr, w.ovr, w.rtbits, w.lbase, gaps ? 1 : 0);
          else
              hipLaunchKernelGGL(k_bwt_f_run_place<false>, dim3((runElems + 255) / 256), dim3(256), 0, s, v, w.runList, w.loff, nRun, runElems, hbits + kbits, rk, rv, mbits, w.t1, w.t3,
                                 nWinM, w.large[cur], w.valsB, w.ovr, w.rtbits, w.lbase, gaps ? 1 : 0);
          v.ovr = w.ovr; v.rtbits = w.rtbits; }
        { KScope ks_("k_bwt_f_merge_bits"); merge_bits(); }
        return 0;
    }
    // Round 0's medium groups compacted, and periodic stretches of a period the doubling offsets never meet taken apart by looking at the
    // text (k_bwt_f_probe) before the first round: the groups it takes apart are void in the list (length 0), their parts that are medium
    // groups are appended to it. Candidates among the medium groups of the list just compacted; their number comes back with the counters.
    int probe()
    {
        u32* probeCand = w.medFlags;                                  // (free between two compactions)
        compact_medium(w.med[cur]);
        { KScope ks_("k_bwt_f_probe"); hipLaunchKernelGGL(k_bwt_f_probe_scan, dim3(256), dim3(256), 0, s, v, w.med[cur], (u32)nsym, v.rtbits, probeCand); }
        if (fetch(0, CNT_ROUND_SLOTS)) return -1;
        surv = hp[CNT_SMALL_LEFT]; nMed = hp[CNT_MED]; nMedLo = hp[CNT_MED_LO]; nLarge = hp[CNT_LARGE]; largeElems = hp[CNT_LARGE_MEMBERS];
        if (const u32 nCand = hp[CNT_PROBE_CAND]) {
            enable_run_tiebits();
            hipMemsetAsync(w.counters, 0, 4 * CNT_PROBE_SLOTS, s);
            { KScope ks_("k_bwt_f_probe");
              hipLaunchKernelGGL(k_bwt_f_probe, dim3(std::min<u32>(nCand, 4096)), dim3(512), 0, s, bv, v, w.med[cur], probeCand, nCand, (u32)nsym, w.med[cur ^ 1], w.large[cur], w.ovr, w.rtbits);
              merge_bits(); }
            compact_medium(w.med[cur], nMed, nMedLo);
            if (fetch(0, CNT_MED_LO + 1)) return -1;                    // (the probe's two slots, and the class count that goes with CNT_MED)
            surv |= hp[CNT_SMALL_LEFT]; nMed += hp[CNT_MED]; nMedLo += hp[CNT_MED_LO];
        }
        if (tune.stats) fprintf(stderr, "after round 0 (nsym %d, total %u): run groups %u (%u members); small left %u, medium %u, large %u (%u members); run members placed directly %u, sorted %u, kept out of the round-0 sort %u; flag workgroups inside a gap %u\n",
                                nsym, total, nRun, runElems, surv, nMed, nLarge, largeElems, (nRun && runDirect) ? runElems : 0u, (nRun && !runDirect) ? runElems : 0u, gaps ? keptOut : 0u,
                                gaps ? r0Skipped : 0u);
        statT = std::chrono::steady_clock::now();
        return 0;
    }
    // Link step: small groups inside long repeats linked to the group one position on (k_bwt_f_link_small); a trial looks at whole
    // blocks, the first, the middle and the last one of the batch (blocks next to each other would share a window)
    void link_step()
    {
        KScope ks_("k_bwt_f_link");
        u32* posflag = w.ebits; u32* linked = w.rbits; u32* rev = w.rcount; u32* sufRev = w.rprefix;
        const bool trial = link.mode == LinkPlan::TRIAL; linkTr.n = 0;
        if (trial) { linkTr.blk[linkTr.n++] = 0; if (st.nBlocks >= 5) linkTr.blk[linkTr.n++] = st.nBlocks / 2; if (st.nBlocks >= 3) linkTr.blk[linkTr.n++] = st.nBlocks - 1; }
        const u32 nW = total / 32 + 1;
        hipMemsetAsync(posflag, 0, 4 * (size_t)nW, s);
        hipMemsetAsync(linked, 0, 4 * ((size_t)nTiles * (SM_TS / 32) + 64), s);
        enable_run_tiebits();
        // (a block covers at most VS / SM_TS + 2 windows; the kernels' window stride is 1: every window)
        const u32 nTrial = (u32)std::min<u64>((u64)nTiles, ((u64)bv.VS + SM_TS - 1) / SM_TS + 2);
        const dim3 gridL(trial ? nTrial : nTiles, (unsigned)(linkTr.n ? linkTr.n : 1));
        hipLaunchKernelGGL(k_bwt_f_link_small, gridL, dim3(256), 0, s, v, posflag, linked, tune.stats, 1u, w.linkedTile, linkTr);
        hipLaunchKernelGGL(k_bwt_f_link_zeros, GRID1(nW), posflag, nW, rev);
        prims::launch_scan<prims::SCAN_MIN_INCL>(s, rev, sufRev, nW, nullptr, w.scanTmp);
        hipLaunchKernelGGL(k_bwt_f_link_apply, gridL, dim3(256), 0, s, v, posflag, sufRev, nW, linked, h, w.ovr, w.rtbits, 1u, linkTr);
    }
    // small groups, ranked in windows of the bit map (with versioned labels the kernel fetches their keys itself); the link step's payoff
    void sort_small(bool linked)
    {
        KScope ks_("k_bwt_f_sort_small");
        u32* survTile = tune.link ? w.survTile : nullptr;
        if (v.ISA2 && pbits <= 23 && !tune.noPack) hipLaunchKernelGGL(k_bwt_f_small_fused<true>, dim3(nTiles), dim3(256), 0, s, v, h, survTile, tune.stats);
        else if (v.ISA2) hipLaunchKernelGGL(k_bwt_f_small_fused<false>, dim3(nTiles), dim3(256), 0, s, v, h, survTile, tune.stats);
        else hipLaunchKernelGGL(k_bwt_f_sort_small, dim3(nTiles), dim3(256), 0, s, v, survTile);
        if (linked) hipLaunchKernelGGL(k_bwt_f_link_payoff, dim3(1), dim3(256), 0, s, v, w.linkedTile, w.survTile, nTiles, 1u, w.counters + CNT_LINKED, linkTr);
        if (tune.link) prims::launch_scan<prims::SCAN_SUM_EXCL>(s, w.survTile, w.survTile, nTiles, nullptr, w.scanTmp, w.counters + CNT_TIED);
    }
    // medium groups: two workgroup shapes, each takes the groups of its size class: 256 threads x 8 elements (21 KB of LDS, groups up to
    // MED_LO_CAP) and 512 threads x 16 elements (76 KB: two groups per CU in flight); a group that takes the chain round is finished by the
    // workgroup that holds it. Fused (versioned labels): a launch per class over that class's index, none for a class without groups;
    // else both shapes walk the whole list.
    void sort_medium()
    {
        const int npass = (kbits + 7) / 8, nxt = cur ^ 1;
        if (medFuse) {
            KScope ks_("k_bwt_f_medium_fused"); const int skip = tune.noUnsplitSkip ? 0 : 1; const u32 nMedHi = nMed - nMedLo;
            const auto fuse256 = tune.stats ? k_bwt_f_medium_fused<256, 8, true> : k_bwt_f_medium_fused<256, 8, false>;
            const auto fuse512 = tune.stats ? k_bwt_f_medium_fused<512, 16, true> : k_bwt_f_medium_fused<512, 16, false>;
            // (whole multiples of 8 workgroups, one eighth of a class per XCD; four and two workgroups per CU at once)
            if (nMedLo) hipLaunchKernelGGL(fuse256, dim3(std::min<u32>((nMedLo + 7) / 8 * 8, 2048)), dim3(256), 0, s, v, w.med[cur], w.medIdxLo, nMedLo, h, npass, skip, w.med[nxt], w.large[nxt]);
            if (nMedHi) hipLaunchKernelGGL(fuse512, dim3(std::min<u32>((nMedHi + 7) / 8 * 8, 1024)), dim3(512), 0, s, v, w.med[cur], w.medIdxHi, nMedHi, h, npass, skip, w.med[nxt], w.large[nxt]);
        } else { KScope ks_("k_bwt_f_sort_medium"); const dim3 gridM(std::min<u32>(nMed, 8192));
          const auto sort256 = tune.stats ? k_bwt_f_sort_medium<256, 8, true> : k_bwt_f_sort_medium<256, 8, false>;
          const auto sort512 = tune.stats ? k_bwt_f_sort_medium<512, 16, true> : k_bwt_f_sort_medium<512, 16, false>;
          hipLaunchKernelGGL(sort256, gridM, dim3(256), 0, s, v, w.med[cur], nMed, h, npass, SM_G, w.med[nxt], w.large[nxt], w.descInfo);
          hipLaunchKernelGGL(sort512, gridM, dim3(512), 0, s, v, w.med[cur], nMed, h, npass, MED_LO_CAP, w.med[nxt], w.large[nxt], w.descInfo); }
    }
    // large groups: (descriptor index, key) pairs, KEY = u32 where kbits + lbits bits fit. The keys are gathered before any kernel of the
    // round changes a label; the sort and the placement come after the small and medium groups.
    template <class KEY> void large_keys()
    {
        { KScope ks_("k_bwt_f_large_prefix"); hipLaunchKernelGGL(k_bwt_f_large_prefix, dim3(1), dim3(1024), 0, s, w.large[cur], nLarge, w.loff, w.base, st.nBlocks, w.lbase); }
        KScope ks_("k_bwt_f_large_keys");
        hipLaunchKernelGGL(k_bwt_f_large_keys<KEY>, GRID1(largeElems), v, w.large[cur], nLarge, w.loff, largeElems, h, kbits, reinterpret_cast<KEY*>(keysFree), w.valsA);
    }
    template <class KEY> void sort_large(int lbits)
    {
        KEY* ka = reinterpret_cast<KEY*>(keysFree); KEY* kb = reinterpret_cast<KEY*>(keysFree2); int r;
        { KScope ks_("k_bwt_f_sort_large");
          // (count + scatter passes here: with the many passes of these keys, most of them on constant digits, counting all of
          // them ahead costs more than it saves -- period 3 / 5 / 7 / 768 at 8 MiB: 11.1-17.6 ms against 11.8-18.2)
          // (from LARGE_OS_MIN members on the passes are the one-sweep ones; real files' 27 M members in the first round: 4.11 -> 3.94 ms,
          // and counted for every sort they cost the many small ones of periodic data more than they save: 4.11 -> 4.56)
          r = sort_one_segment<KEY, true>(largeElems, ka, kb, w.valsA, w.valsB, 0, kbits + lbits, largeElems >= LARGE_OS_MIN); }
        const KEY* sk = r ? kb : ka; const u32* sv = r ? w.valsB : w.valsA;
        { KScope ks_("k_bwt_f_large_flags"); hipLaunchKernelGGL(k_bwt_f_large_flags<KEY>, GRID1(largeElems), sk, largeElems, w.t0, w.t2); }
        bounds(largeElems, true);
        { KScope ks_("k_bwt_f_large_place");
          hipLaunchKernelGGL(k_bwt_f_large_place<KEY>, GRID1(largeElems), v, w.large[cur], w.loff, largeElems, kbits, sk, sv, w.t1, w.t3, w.med[cur ^ 1], w.large[cur ^ 1], w.lbase); }
    }
    // the round's group starts merged, its medium groups compacted into the next round's list, the counters read back
    int end_round()
    {
        { KScope ks_("k_bwt_f_merge_bits"); merge_bits(); }
        compact_medium(w.med[cur ^ 1]);
        if (fetch(0, CNT_ROUND_SLOTS)) return -1;
        surv = hp[CNT_SMALL_LEFT]; nMed = hp[CNT_MED]; nMedLo = hp[CNT_MED_LO]; nLarge = hp[CNT_LARGE]; largeElems = hp[CNT_LARGE_MEMBERS]; survMembers = hp[CNT_TIED];
        if (tune.stats) {
            // windows that still hold tied small groups (from the scanned per-window counts; developer statistics only)
            std::vector<u32> hs(nTiles); u32 activeTiles = 0;
            if (tune.link && hipMemcpyAsync(hs.data(), w.survTile, 4 * (size_t)nTiles, hipMemcpyDeviceToHost, s) == hipSuccess && hipStreamSynchronize(s) == hipSuccess) {
                for (u32 t = 0; t + 1 < nTiles; t++) activeTiles += hs[t + 1] != hs[t] ? 1u : 0u;
                fprintf(stderr, "  windows with tied small groups after the round: %u of %u\n", activeTiles, nTiles);
            }
            const std::chrono::steady_clock::time_point now = std::chrono::steady_clock::now();
            fprintf(stderr, "round h=%u (%.3f ms): small members worked on %u in %u groups, medium members %u; after it: small left %u, medium groups %u, large %u (%u members); %u groups took the chain round; %u small members still tied\n",
                    h, std::chrono::duration<double, std::milli>(now - statT).count(), hp[CNT_STAT_SMALL], hp[CNT_STAT_SMALL_GROUPS], hp[CNT_STAT_MED], surv, nMed, nLarge, largeElems,
                    hp[CNT_CHAINED], hp[CNT_TIED]);
            fprintf(stderr, "  medium groups worked on %u (%u members): all keys equal in %u (%u members)%s, majority path %u (%u members), asleep %u (%u members)\n", hp[CNT_STAT_MED_GROUPS], hp[CNT_STAT_MED],
                    hp[CNT_STAT_UNSPLIT], hp[CNT_STAT_UNSPLIT_MEMBERS], tune.noUnsplitSkip ? "" : " -- left alone", hp[CNT_STAT_MAJ], hp[CNT_STAT_MAJ_MEMBERS], hp[CNT_STAT_ASLEEP], hp[CNT_STAT_ASLEEP_MEMBERS]);
            statT = now;
        }
        cur ^= 1; h <<= 1;
        return 0;
    }
    // One doubling round on offset h: all keys first (a round sorts on the labels as they stood when it began), then the refinements
    int round()
    {
        if (h > bv.VS) return -5;                                    // cannot happen: suffixes of one block differ in length
        { KScope ks_("k_bwt_f_round"); hipMemsetAsync(w.counters, 0, 4 * CNT_ROUND_SLOTS, s); }     // (the scope counts the doubling rounds for the profile)
        if (++v.round > 255) return -5;                              // (the number the round's label writes carry; at most log2(block) + a few)
        const bool linked = surv && tune.link && h >= (u32)(tune.link > 1 ? tune.link : 32)
                            && link.next(h, survMembers, total, hp[CNT_LINKED], hp[CNT_LINK_TIED], tune.stats);
        if (linked) link_step();
        // (with versioned labels the small groups fetch their keys in k_bwt_f_small_fused; the medium list is in slot order: k_bwt_f_med_compact)
        if (surv && !v.ISA2) { KScope ks_("k_bwt_f_gather_small"); hipLaunchKernelGGL(k_bwt_f_gather_small, dim3(nTiles), dim3(256), 0, s, v, h, tune.stats); }
        // the first round's list is not in slot order (the probe appends) and has no round before it
        if (groupSleep) { v.verdictNow = w.medVerdict[v.round & 1]; v.verdictWas = w.medVerdict[(v.round & 1) ^ 1]; }
        if (groupSleep && nMed && v.round >= 2) { KScope ks_("k_bwt_f_med_sleep"); hipLaunchKernelGGL(k_bwt_f_med_sleep, GRID1(nMed), v, w.med[cur], nMed, tune.stats); }
        // (k_bwt_f_medium_fused fetches the medium groups' keys itself, behind the small groups' kernel)
        if (nMed && !medFuse) { KScope ks_("k_bwt_f_gather_desc"); hipLaunchKernelGGL(k_bwt_f_gather_desc, dim3(1024), dim3(GATHER_THREADS), 0, s, v, w.med[cur], nMed, h, w.descInfo, tune.stats, tune.noUnsplitSkip ? 0 : 1); }
        const int lbits = bits_for(nLarge, 0); const bool key32 = kbits + lbits <= 32;
        if (nLarge) { if (key32) large_keys<u32>(); else large_keys<u64>(); }
        if (surv) sort_small(linked);
        if (nMed) sort_medium();
        if (nLarge) { if (key32) sort_large<u32>(lbits); else sort_large<u64>(lbits); }
        return end_round();
    }
    // the codec's output: header and BWT bytes
    void emit()
    {
        KScope ks_("k_bwt_f_emit");
        hipLaunchKernelGGL(k_bwt_f_emit, dim3((unsigned)std::min<size_t>(((size_t)bv.VS + 255) / 256, 4096), st.nBlocks), dim3(256), 0, s, bv, w.base, st.ok, w.SA, v, st.newLen);
    }
};

// Returns 0 or a negative HIP error. Synchronises the stream (the sizes of the work lists are read back per round).
// sa == nullptr: the BWT block codec (emits header + BWT bytes). Otherwise the suffix arrays only, left in the scratch (bwt_suffix_arrays).
static int bwt_forward_run(hipStream_t s, const XfStage& st, void* scratch, size_t scratchBytes, u32* h_pinned, BwtSuffixArrays* sa)
{
    FwdSort f{ s, st, h_pinned };
    if (int r = f.setup(scratch, scratchBytes, sa)) return r;
    if (f.total == 0) return 0;
    if (f.run_scan()) return -1;
    f.round0_sort();
    if (f.round0_place() || f.run_round() || f.probe()) return -1;
    while (f.surv || f.nMed || f.nLarge) if (int r = f.round()) return r;
    if (!sa) f.emit();
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int launch_bwt_forward(hipStream_t s, const XfStage& st, void* scratch, size_t scratchBytes, u32* h_pinned)
{ return bwt_forward_run(s, st, scratch, scratchBytes, h_pinned, nullptr); }
int bwt_suffix_arrays(hipStream_t s, const XfStage& st, void* scratch, size_t scratchBytes, u32* h_pinned, BwtSuffixArrays* out)
{ return bwt_forward_run(s, st, scratch, scratchBytes, h_pinned, out); }

}  // namespace knz
