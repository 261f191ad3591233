// TPAQ and TPAQX on gfx950 (kanzi "TPAQ" / "TPAQX", entropy ids 7 and 9): the binary arithmetic coder of CM (binary_coder.hpp) behind
// the TPAQ predictor, templated on TPAQX as the reference is.
//
// NOT BUILT YET: staging one byte's states in LDS (the windows (ctx + c0) & mask, c0 = 1..255, of contexts 2 to 6 fetched once per
// byte, walked for eight bits and written back). What is here is the per-bit shape: one dependent trip to the big table per bit.
//
// Reference being replaced (bit-identical streams): entropy/TPAQPredictor.hpp:297-632, TPAQPredictor.cpp:20-60,
// AdaptiveProbMap.hpp:93-130, Global.cpp:90-120 (squash / stretch). Every stream path of the reference builds the predictor with a
// Context of bitstream version 6: the masks of the ring buffer and the hash are size - 1 without rounding to a power of two, and are
// applied with &. Version 7 and up (rounded sizes) is not built here (api.hip refuses it); versions 3 to 5 take the path of 6.
//
// Tables of one block, in global memory (tpaq_layout; zeroed on the stream before every launch; between about 20 MiB and 1.4 GiB):
//   big states (4 MiB .. 256 MiB by the stream's block size, x 4 for TPAQX; KNZ_TPAQ_STATES_LOG forces 2^k for tests), small states 0
//   (64 KiB) and 1 (16 MiB), hash of buffer positions (min(16 Mi, 16 * count) words, x 4), ring buffer (min(block size, 64 MiB) bytes),
//   mixers (2^8 .. 2^16 by the block's length, x 4; 40 bytes each: eight weights, skew, learn rate -- inputs and _pr belong to the one
//   live get / update pair and stay in registers) and, for TPAQX, the second SSE map of 65536 x 33 cells.
//   Mixers and SSE cells are stored as the DIFFERENCE to their initial value, so that zeroed memory is the initial state.
// In LDS: the first SSE map (256 x 33 cells), squash, stretch, STATE_MAP, both transition rows, MATCH_PRED. In registers: the current
// mixer (lane i < 8 holds weight i and input i), the contexts and pointers (lane i < 7 owns context i).
//
// One bit, one wave. Lane i < 7: apply the transition behind its old pointer, form the new pointer, read the state there, look it up
// in STATE_MAP. The eight products weight x input are summed across lanes 0-7. Mixer update, SSE and the interval are wave-uniform.
//
// Equal pointers. _cp2 .. _cp6 point into one table and the reference steps the state behind each in sequence, so a cell that m of
// them share is stepped m times. Here every lane counts the lanes that hold its address (mTotal) and those in front of it (mBefore),
// applies the transition mTotal times to the value it holds (all sharers hold the same value: every lane's value is what memory
// holds behind its pointer), and the first sharer stores. TPAQX steps the cell behind the old _cp6 AFTER the new _cp2 .. _cp5 were
// read (TPAQPredictor.hpp:488-524): lane 6 joins the same store phase, and a lane of 2-5 whose NEW address is lane 6's OLD one
// predicts from the value in front of lane 6's step (lane 6's `pre`), while it remembers what memory holds.
//
// Store, then load, in one wave. Nothing is assumed about what a later load of this wave sees of an earlier store in the L1. The L1
// is write-through, so every store reaches the L2 of the wave's XCD; stores are workgroup-scope relaxed atomics (`sc0`), which keep
// the line in that L2 (the agent-scope `sc1` form drops it, and the next load pays a trip to memory: measured, 10.4 and 17.4 us per
// byte at 1 MiB against the 7.3 and 13.2 of DESIGN.md 3.3). Every load phase is preceded by s_waitcnt vmcnt(0), which on this ISA counts stores
// until they are acknowledged, and every load of the tables is an agent-scope relaxed atomic (`sc1`), which bypasses the L1 and is
// served by that same L2 (MI355X_MICROARCH, visibility). So a load is issued only after the L2 holds every earlier store of the
// wave, and reads there. A block's tables are touched by its one wave only. Within one call, a value that was just computed is
// forwarded in registers instead of being read back (SSE cells). On the CPU emulator lanes are fibers that run apart between
// collectives; the same wait is a collective there.
#include "common.hpp"
#include "stages.hpp"
#include "binary_coder.hpp"

#include <stdlib.h>
#include <vector>

namespace knz {

constexpr int TPAQ_MAX_LENGTH = 88;
constexpr u32 TPAQ_HASH = 0x7FEB352Du;
constexpr int TPAQ_BEGIN_LEARN_RATE = 60 << 7;
constexpr int TPAQ_END_LEARN_RATE = 11 << 7;

struct TpaqLut { int16_t squash[4096]; int16_t stretch[4096]; };
constexpr TpaqLut tpaq_make_lut()
{
    // Global.cpp:90-120
    constexpr int INV_EXP[33] = { 0, 8, 22, 47, 88, 160, 283, 492, 848, 1451, 2459, 4117, 6766, 10819, 16608, 24127, 32768, 41409, 48928, 54717,
                                  58770, 61419, 63077, 64085, 64688, 65044, 65253, 65376, 65448, 65489, 65514, 65528, 65536 };
    TpaqLut t{};
    for (int x = 1; x < 4096; x++) {
        const int w = x & 127, y = x >> 7;
        t.squash[x - 1] = (int16_t)((INV_EXP[y] * (128 - w) + INV_EXP[y + 1] * w) >> 11);
    }
    t.squash[4095] = 4095;
    int n = 0;
    for (int x = -2047; x <= 2047 && n < 4096; x++) {
        const int sq = t.squash[x + 2047];
        while (n <= sq) t.stretch[n++] = (int16_t)x;
    }
    t.stretch[4095] = 2047;
    return t;
}
static __device__ const TpaqLut TPAQ_LUT = tpaq_make_lut();

static __device__ const u8 TPAQ_TRANSITIONS[2][256] = {
    { 1, 3, 143, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20, 21, 22, 23, 24, 25, 26, 27, 28, 29, 30,
      31, 32, 33, 34, 35, 36, 37, 38, 39, 40, 41, 42, 43, 44, 45, 46, 47, 48, 49, 50, 51, 52, 47, 54, 55, 56, 57, 58, 59, 60,
      61, 62, 63, 64, 65, 66, 67, 68, 69, 6, 71, 71, 71, 61, 75, 56, 77, 78, 77, 80, 81, 82, 83, 84, 85, 86, 87, 88, 77, 90,
      91, 92, 80, 94, 95, 96, 97, 98, 99, 90, 101, 94, 103, 101, 102, 104, 107, 104, 105, 108, 111, 112, 113, 114, 115, 116, 92, 118, 94, 103,
      119, 122, 123, 94, 113, 126, 113, 128, 129, 114, 131, 132, 112, 134, 111, 134, 110, 134, 134, 128, 128, 142, 143, 115, 113, 142, 128, 148, 149, 79,
      148, 142, 148, 150, 155, 149, 157, 149, 159, 149, 131, 101, 98, 115, 114, 91, 79, 58, 1, 170, 129, 128, 110, 174, 128, 176, 129, 174, 179, 174,
      176, 141, 157, 179, 185, 157, 187, 188, 168, 151, 191, 192, 188, 187, 172, 175, 170, 152, 185, 170, 176, 170, 203, 148, 185, 203, 185, 192, 209, 188,
      211, 192, 213, 214, 188, 216, 168, 84, 54, 54, 221, 54, 55, 85, 69, 63, 56, 86, 58, 230, 231, 57, 229, 56, 224, 54, 54, 66, 58, 54,
      61, 57, 222, 78, 85, 82, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0 },
    { 2, 163, 169, 163, 165, 89, 245, 217, 245, 245, 233, 244, 227, 74, 221, 221, 218, 226, 243, 218, 238, 242, 74, 238, 241, 240, 239, 224, 225, 221,
      232, 72, 224, 228, 223, 225, 238, 73, 167, 76, 237, 234, 231, 72, 31, 63, 225, 237, 236, 235, 53, 234, 53, 234, 229, 219, 229, 233, 232, 228,
      226, 72, 74, 222, 75, 220, 167, 57, 218, 70, 168, 72, 73, 74, 217, 76, 167, 79, 79, 166, 162, 162, 162, 162, 165, 89, 89, 165, 89, 162,
      93, 93, 93, 161, 100, 93, 93, 93, 93, 93, 161, 102, 120, 104, 105, 106, 108, 106, 109, 110, 160, 134, 108, 108, 126, 117, 117, 121, 119, 120,
      107, 124, 117, 117, 125, 127, 124, 139, 130, 124, 133, 109, 110, 135, 110, 136, 137, 138, 127, 140, 141, 145, 144, 124, 125, 146, 147, 151, 125, 150,
      127, 152, 153, 154, 156, 139, 158, 139, 156, 139, 130, 117, 163, 164, 141, 163, 147, 2, 2, 199, 171, 172, 173, 177, 175, 171, 171, 178, 180, 172,
      181, 182, 183, 184, 186, 178, 189, 181, 181, 190, 193, 182, 182, 194, 195, 196, 197, 198, 169, 200, 201, 202, 204, 180, 205, 206, 207, 208, 210, 194,
      212, 184, 215, 193, 184, 208, 193, 163, 219, 168, 94, 217, 223, 224, 225, 76, 227, 217, 229, 219, 79, 86, 165, 217, 214, 225, 216, 216, 234, 75,
      214, 237, 74, 74, 163, 217, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0 }
};

static __device__ const int16_t TPAQ_STATE_MAP[256] = {
    -31, -400, 406, -547, -642, -743, -827, -901, -901, -974, -945, -955, -1060, -1031, -1044, -956,
    -994, -1035, -1147, -1069, -1111, -1145, -1096, -1084, -1171, -1199, -1062, -1498, -1199, -1199, -1328, -1405,
    -1275, -1248, -1167, -1448, -1441, -1199, -1357, -1160, -1437, -1428, -1238, -1343, -1526, -1331, -1443, -2047,
    -2047, -2044, -2047, -2047, -2047, -232, -414, -573, -517, -768, -627, -666, -644, -740, -721, -829,
    -770, -963, -863, -1099, -811, -830, -277, -1036, -286, -218, -42, -411, 141, -1014, -1028, -226,
    -469, -540, -573, -581, -594, -610, -628, -711, -670, -144, -408, -485, -464, -173, -221, -310,
    -335, -375, -324, -413, -99, -179, -105, -150, -63, -9, 56, 83, 119, 144, 198, 118,
    -42, -96, -188, -285, -376, 107, -138, 38, -82, 186, -114, -190, 200, 327, 65, 406,
    108, -95, 308, 171, -18, 343, 135, 398, 415, 464, 514, 494, 508, 519, 92, -123,
    343, 575, 585, 516, -7, -156, 209, 574, 613, 621, 670, 107, 989, 210, 961, 246,
    254, -12, -108, 97, 281, -143, 41, 173, -209, 583, -55, 250, 354, 558, 43, 274,
    14, 488, 545, 84, 528, 519, 587, 634, 663, 95, 700, 94, -184, 730, 742, 162,
    -10, 708, 692, 773, 707, 855, 811, 703, 790, 871, 806, 9, 867, 840, 990, 1023,
    1409, 194, 1397, 183, 1462, 178, -23, 1403, 247, 172, 1, -32, -170, 72, -508, -46,
    -365, -26, -146, 101, -18, -163, -422, -461, -146, -69, -78, -319, -334, -232, -99, 0,
    47, -74, 0, -452, 14, -57, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1
};

static __device__ const int16_t TPAQ_MATCH_PRED[TPAQ_MAX_LENGTH] = {
    0, 64, 128, 192, 256, 320, 384, 448, 512, 576, 640, 704, 768, 832, 896, 960,
    1024, 1038, 1053, 1067, 1082, 1096, 1111, 1125, 1139, 1154, 1168, 1183, 1197, 1211, 1226, 1240,
    1255, 1269, 1284, 1298, 1312, 1327, 1341, 1356, 1370, 1385, 1399, 1413, 1428, 1442, 1457, 1471,
    1486, 1500, 1514, 1529, 1543, 1558, 1572, 1586, 1601, 1615, 1630, 1644, 1659, 1673, 1687, 1702,
    1716, 1731, 1745, 1760, 1774, 1788, 1803, 1817, 1832, 1846, 1861, 1875, 1889, 1904, 1918, 1933,
    1947, 1961, 1976, 1990, 2005, 2019, 2034, 2047
};

// ------------------------------------------------------------------------------------------------
// sizes (TPAQPredictor.hpp:302-363 with a Context of bitstream version 6)
// ------------------------------------------------------------------------------------------------
__host__ __device__ __forceinline__ TpaqSizes tpaq_sizes(u32 rbsz, u32 absz, int extra)
{
    TpaqSizes z;
    if (rbsz >= 64u << 20) z.states = 1u << 28;
    else if (rbsz >= 16u << 20) z.states = 1u << 27;
    else if (rbsz >= 4u << 20) z.states = 1u << 26;
    else z.states = (rbsz >= 1u << 20) ? 1u << 24 : 1u << 22;
    if (absz >= 32u << 20) z.mixers = 1u << 16;
    else if (absz >= 16u << 20) z.mixers = 1u << 15;
    else if (absz >= 8u << 20) z.mixers = 1u << 14;
    else if (absz >= 4u << 20) z.mixers = 1u << 13;
    else z.mixers = (absz >= 1u << 20) ? 1u << 11 : 1u << 8;
    z.buffer = rbsz < (64u << 20) ? rbsz : 64u << 20;
    const u32 mxsz = absz < (1u << 26) ? absz * 16 : 1u << 30;
    z.hash = (16u << 20) < mxsz ? 16u << 20 : mxsz;
    z.mixers <<= 2 * extra;
    z.states <<= 2 * extra;
    z.hash <<= 2 * extra;
    z.sse0 = 256;
    z.sse1 = extra ? 65536 : 256;
    return z;
}

TpaqSizes tpaq_params(u32 rbsz, u32 absz, int extra) { return tpaq_sizes(rbsz, absz, extra); }

// KNZ_TPAQ_STATES_LOG=k (a debugging aid like KNZ_CM_TIER1_DIV, read on every call): the big states table has 2^k bytes whatever the
// block size says, so that a test can make pointers of different contexts meet. 0 = the format's size.
u32 tpaq_states_log()
{
#ifdef KNZ_EMU_TPAQ_STATES_LOG
    return KNZ_EMU_TPAQ_STATES_LOG;
#else
    const char* e = getenv("KNZ_TPAQ_STATES_LOG");
    const int v = e ? atoi(e) : 0;
    return (v >= 8 && v <= 30) ? (u32)v : 0u;
#endif
}

// KNZ_TPAQ_TABLES_MAX=bytes: what the tables of the blocks that run at once may take (default 16 GiB). A batch whose tables exceed it
// runs in slices of as many blocks as fit, at least one: a block never gets fewer tables than the format says.
static size_t tpaq_budget()
{
    const char* e = getenv("KNZ_TPAQ_TABLES_MAX");
    const long long v = e ? atoll(e) : 0;
    return v > 0 ? (size_t)v : ((size_t)16 << 30);
}

struct TpaqLayout { u64 big, small0, small1, hashes, buffer, mixers, sse1, stride; u32 statesLog, abszMax; };

// (sizes grow with absz, so the layout of the longest block a batch can hold serves every block of it)
static TpaqLayout tpaq_layout(u32 rbsz, u32 abszMax, int extra, u32 statesLog)
{
    const TpaqSizes z = tpaq_sizes(rbsz, abszMax, extra);
    TpaqLayout l;
    u64 o = 0;
    auto take = [&](u64 bytes) { const u64 at = o; o += (bytes + 255) & ~255ull; return at; };
    l.big = take(statesLog ? (1ull << statesLog) : (u64)z.states);
    l.small0 = take(1u << 16);
    l.small1 = take(1u << 24);
    l.hashes = take(4ull * z.hash);
    l.buffer = take(z.buffer ? z.buffer : 1);
    l.mixers = take(40ull * z.mixers);
    l.sse1 = take(extra ? 2ull * 33 * 65536 : 0);
    l.stride = o;
    l.statesLog = statesLog;
    l.abszMax = abszMax;
    return l;
}

size_t tpaq_table_bytes(u32 rbsz, u32 abszMax, int extra) { return (size_t)tpaq_layout(rbsz, abszMax, extra, tpaq_states_log()).stride; }

int tpaq_slice_blocks(size_t tableBytes, int nBlocks)
{
    const size_t fit = tpaq_budget() / (tableBytes ? tableBytes : 1);
    return (int)(fit < 1 ? 1 : fit > (size_t)nBlocks ? (size_t)nBlocks : fit);
}

// ------------------------------------------------------------------------------------------------
// table accesses
// ------------------------------------------------------------------------------------------------
// loads are ld_agent (common.hpp); the store is relaxed at WORKGROUP scope, not agent scope like the loads: kept as found
template <class T> __device__ __forceinline__ void st_wg(T* p, T v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
#ifdef KNZ_EMU
__device__ __forceinline__ void tq_drain() { (void)__ballot(1); }
#else
__device__ __forceinline__ void tq_drain() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }
#endif

struct TpaqLds {
    u16 sse0[256 * 33];
    int16_t squash[4096];
    int16_t stretch[4096];
    int16_t stateMap[256];
    int16_t matchPred[TPAQ_MAX_LENGTH];
    u16 sseRow[34];                 // the initial row of an SSE map
    u8 trans[2 * 256];
};
static_assert(sizeof(TpaqLds) + 4 * CM_RING_WORDS + 64 <= KNZ_LDS_BYTES, "the small tables of a block live in the LDS of one workgroup");

__device__ __forceinline__ int tpaq_squash(const TpaqLds& L, int d)
{
    return d >= 2048 ? 4095 : d <= -2048 ? 0 : (int)L.squash[d + 2047];
}

__device__ __forceinline__ void tpaq_lds_init(TpaqLds& L, int lane)
{
    for (u32 i = (u32)lane; i < 4096; i += 64) { L.squash[i] = TPAQ_LUT.squash[i]; L.stretch[i] = TPAQ_LUT.stretch[i]; }
    for (u32 i = (u32)lane; i < 256; i += 64) L.stateMap[i] = TPAQ_STATE_MAP[i];
    for (u32 i = (u32)lane; i < 512; i += 64) L.trans[i] = TPAQ_TRANSITIONS[i >> 8][i & 255];
    for (u32 i = (u32)lane; i < (u32)TPAQ_MAX_LENGTH; i += 64) L.matchPred[i] = TPAQ_MATCH_PRED[i];
    // LogisticAdaptiveProbMap: cell j of every context starts at squash((j - 16) * 128) << 4
    for (u32 i = (u32)lane; i < 256 * 33; i += 64) {
        const int d = ((int)(i % 33) - 16) * 128;
        const int sq = d >= 2048 ? 4095 : d <= -2048 ? 0 : (int)TPAQ_LUT.squash[d + 2047];
        L.sse0[i] = (u16)(sq << 4);
        if (i < 33) L.sseRow[i] = (u16)(sq << 4);
    }
}

template <bool X>
struct TpaqPred {
    TpaqLds& L;
    const int lane;
    // tables
    u8* big; u8* small0; u8* small1; u8* buffer; int* hashes; int* mixers; u16* sse1;
    u32 statesMask, mixersMask, hashMask, bufMask;
    // wave-uniform state
    u32 pr, c0, c4, c8, hash;
    int bpos, pos, binCount, matchLen, matchPos, matchVal;
    int skew, lr, mixPr;
    u32 mixIdx, sse0Idx, sse1Idx, sse1Col;
    // per lane: context i, the cell behind its pointer (an id that tells tables apart, the address, the value memory holds there),
    // the mixer's input i and weight i (lanes 8 and 9 carry skew and learn rate to and from memory)
    u32 myCtx, myId, myVal;
    u8* myPtr;
    int myIn, myW;

    __device__ __forceinline__ TpaqPred(TpaqLds& lds, int ln, u8* tables, const TpaqLayout& lay, u32 rbsz, u32 absz) : L(lds), lane(ln)
    {
        const TpaqSizes z = tpaq_sizes(rbsz, absz, X ? 1 : 0);
        big = tables + lay.big; small0 = tables + lay.small0; small1 = tables + lay.small1; buffer = tables + lay.buffer;
        hashes = reinterpret_cast<int*>(tables + lay.hashes); mixers = reinterpret_cast<int*>(tables + lay.mixers);
        sse1 = reinterpret_cast<u16*>(tables + lay.sse1);
        statesMask = (lay.statesLog ? (1u << lay.statesLog) : z.states) - 1;
        mixersMask = (z.mixers - 1) & ~1u;
        hashMask = (z.hash ? z.hash : 1u) - 1;             // (no block that is coded has a length or a block size of 0; the
        bufMask = (z.buffer ? z.buffer : 1u) - 1;          //  masks of such sizes would reach past the tables)
        pr = 2048; c0 = 1; c4 = 0; c8 = 0; hash = 0;
        bpos = 8; pos = 0; binCount = 0; matchLen = 0; matchPos = 0; matchVal = 0;
        skew = 0; lr = TPAQ_BEGIN_LEARN_RATE; mixPr = 2048;
        mixIdx = 0; sse0Idx = 0; sse1Idx = 0; sse1Col = 0;
        myCtx = 0; myVal = 0; myIn = 0;
        myW = lane < 8 ? 32768 : 0;
        // _cp0 and _cp1 at the start of the small tables, _cp2 .. _cp6 at the start of the big one
        const int last = X ? 6 : 5;
        myPtr = lane == 0 ? small0 : lane == 1 ? small1 : big;
        myId = lane == 0 ? 0x80000000u : lane == 1 ? 0xC0000000u : lane <= last ? 0u : 0xFFFFFFFFu;
    }

    __device__ __forceinline__ u32 get() const { return pr; }

    __device__ __forceinline__ u32 rl(u32 v, int l) const { return knz::rl(v, (u32)l); }

    static __device__ __forceinline__ u32 create_context(u32 ctxId, u32 cx)
    {
        cx = cx * 987654323u + ctxId;
        cx = (cx << 16) | (cx >> 16);
        return cx * 123456791u + ctxId;
    }
    static __device__ __forceinline__ u32 hash2(u32 x, u32 y)
    {
        const int h = (int)(x * TPAQ_HASH ^ y * TPAQ_HASH);
        return (u32)(h >> 1) ^ (u32)(h >> 9) ^ (x >> 2) ^ (y >> 3) ^ TPAQ_HASH;
    }

    __device__ __forceinline__ u32 buf_at(u32 i) const { return (u32)ld_agent(buffer + (i & bufMask)); }

    // TPAQPredictor::findMatch (:545-602). The 8-byte big-endian compare: lane k < 8 holds byte k of both words; the lowest 16 bits of
    // the difference that are not zero belong to the highest k that differs.
    __device__ __forceinline__ void find_match()
    {
        if (matchLen > 0) {
            if (matchLen < TPAQ_MAX_LENGTH) matchLen++;
            matchPos++;
            return;
        }
        matchPos = (int)uni((u32)ld_agent(hashes + hash));
        if (matchPos == 0 || (u32)(pos - matchPos) > bufMask) return;
        int r = matchLen + 2;
        while (r + 6 <= TPAQ_MAX_LENGTH) {
            const u32 p0 = (u32)(pos - r - 7) & bufMask;
            const u32 p1 = (u32)(matchPos - r - 7) & bufMask;
            if (p0 > bufMask - 7 || p1 > bufMask - 7) break;
            bool ne = false;
            if (lane < 8) ne = ld_agent(buffer + p0 + lane) != ld_agent(buffer + p1 + lane);
            const u32 diff = (u32)__ballot(ne) & 0xFFu;
            if (diff != 0) {
                const int hi = 31 - __builtin_clz(diff);          // bytes hi + 1 .. 7 agree: 8 * (7 - hi) trailing zero bits
                r += ((7 - hi) >> 1) << 1;
                break;
            }
            r += 8;
        }
        // pair by pair, 32 pairs at a time: lane k looks at the pair at r + 2 k
        while (r <= TPAQ_MAX_LENGTH) {
            const int rk = r + 2 * lane;
            bool ne = false;
            if (lane < 32 && rk <= TPAQ_MAX_LENGTH)
                ne = buf_at((u32)(pos - rk - 1)) != buf_at((u32)(matchPos - rk - 1)) || buf_at((u32)(pos - rk)) != buf_at((u32)(matchPos - rk));
            const u32 bad = (u32)__ballot(ne);
            if (bad != 0) { r += 2 * __builtin_ctz(bad); break; }
            const int pairs = (TPAQ_MAX_LENGTH - r) / 2 + 1;
            r += 2 * (pairs < 32 ? pairs : 32);
        }
        matchLen = r - 2;
    }

    __device__ __forceinline__ void byte_done()
    {
        if (lane == 0) st_wg(buffer + ((u32)pos & bufMask), (u8)c0);
        pos++;
        c8 = (c8 << 8) | ((c4 >> 24) & 0xFF);
        c4 = (c4 << 8) | (c0 & 0xFF);
        hash = (((hash * TPAQ_HASH) << 4) + c4) & hashMask;
        c0 = 1;
        bpos = 8;
        binCount += (int)((c4 >> 7) & 1);
        // the mixer of the next byte, chosen with the match length from before findMatch
        const u32 newMix = (c4 & mixersMask) + (matchLen != 0 ? 1u : 0u);
        if (newMix != mixIdx) {
            if (lane == 8) myW = skew;
            if (lane == 9) myW = lr;
            const int init = lane < 8 ? 32768 : lane == 8 ? 0 : TPAQ_BEGIN_LEARN_RATE;
            if (lane < 10) {
                st_wg(mixers + (size_t)mixIdx * 10 + lane, myW - init);
                myW = ld_agent(mixers + (size_t)newMix * 10 + lane) + init;          // (another mixer: no store of this byte is behind the load)
            }
            skew = (int)rl((u32)myW, 8);
            lr = (int)rl((u32)myW, 9);
            mixIdx = newMix;
        }
        const u32 ctx0 = (c4 & 0xFF) << 8;
        const u32 ctx1 = (c4 & 0xFFFF) << 8;
        const u32 ctx2 = create_context(2, c4 & 0x00FFFFFFu);
        const u32 ctx3 = create_context(3, c4);
        u32 ctx4, ctx5, ctx6 = myCtx;
        bool set6 = X;
        if (binCount < (pos >> 2)) {
            // mostly text or mixed
            ctx4 = create_context(ctx1, c4 ^ (c8 & 0xFFFF));
            ctx5 = (c8 & 0xF0F0F000u) | ((c4 & 0xF0F0F000u) >> 4);
            if (X) {
                const u32 h1 = ((c4 & 0x80808080u) == 0) ? c4 & 0x4F4FFFFFu : c4 & 0x80808080u;
                const u32 h2 = ((c8 & 0x80808080u) == 0) ? c8 & 0x4F4FFFFFu : c8 & 0x80808080u;
                ctx6 = hash2(h1 << 2, h2 >> 2);
            }
        } else {
            // mostly binary
            ctx4 = create_context(TPAQ_HASH + (u32)matchLen, c4 ^ (c4 & 0x000FFFFFu));
            ctx5 = ctx0 | (c8 << 16);
            if (X) ctx6 = hash2(c4 & 0xFFFF0000u, c8 >> 16);
        }
        myCtx = lane == 0 ? ctx0 : lane == 1 ? ctx1 : lane == 2 ? ctx2 : lane == 3 ? ctx3 : lane == 4 ? ctx4 : lane == 5 ? ctx5 : (lane == 6 && set6) ? ctx6 : myCtx;
        tq_drain();                                     // the byte just stored may be read below
        find_match();
        matchVal = (int)(uni(buf_at((u32)matchPos)) | 0x100u);
        if (lane == 0) st_wg(hashes + hash, pos);
    }

    // LogisticAdaptiveProbMap<false, RATE>::get on the map in LDS: every lane stores the same values
    template <int RATE>
    __device__ __forceinline__ int apm0(int bit, int p, u32 ctx)
    {
        const int g = bit ? 65528 : 0;
        const int a = (int)uni(L.sse0[sse0Idx]), b = (int)uni(L.sse0[sse0Idx + 1]);
        L.sse0[sse0Idx] = (u16)(a + ((g - a) >> RATE) + bit);
        L.sse0[sse0Idx + 1] = (u16)(b + ((g - b) >> RATE) + bit);
        const int s = L.stretch[p];
        sse0Idx = (u32)((s + 2048) >> 7) + 33 * ctx;
        const int w = s & 127;
        const int ca = (int)uni(L.sse0[sse0Idx]), cb = (int)uni(L.sse0[sse0Idx + 1]);
        return ((ca << 7) + (cb - ca) * w) >> 11;
    }

    // ... on the map in global memory (TPAQX, rate 7): cells are stored as the difference to their initial value; a cell moved in this
    // call is taken from the registers
    __device__ __forceinline__ int apm1(int bit, int p, u32 ctx)
    {
        const int g = bit ? 65528 : 0;
        const u32 i0 = sse1Idx, col0 = sse1Col;
        const int a = (int)(u16)(uni(ld_agent(sse1 + i0)) + L.sseRow[col0]), b = (int)(u16)(uni(ld_agent(sse1 + i0 + 1)) + L.sseRow[col0 + 1]);
        const int na = (int)(u16)(a + ((g - a) >> 7) + bit), nb = (int)(u16)(b + ((g - b) >> 7) + bit);
        if (lane == 0) { st_wg(sse1 + i0, (u16)(na - L.sseRow[col0])); st_wg(sse1 + i0 + 1, (u16)(nb - L.sseRow[col0 + 1])); }
        const int s = L.stretch[p];
        const u32 col = (u32)((s + 2048) >> 7);
        const u32 i1 = col + 33 * ctx;
        sse1Idx = i1; sse1Col = col;
        const int w = s & 127;
        const int la = (int)(u16)(uni(ld_agent(sse1 + i1)) + L.sseRow[col]), lb = (int)(u16)(uni(ld_agent(sse1 + i1 + 1)) + L.sseRow[col + 1]);
        const int ca = i1 == i0 ? na : i1 == i0 + 1 ? nb : la;
        const int cb = i1 + 1 == i0 ? na : i1 == i0 ? nb : lb;
        return ((ca << 7) + (cb - ca) * w) >> 11;
    }

    // TPAQPredictor::update (:417-542)
    __device__ __forceinline__ void update(bool one)
    {
        const int bit = one ? 1 : 0;
        // TPAQMixer::update
        const int err = (((bit << 12) - mixPr) * lr) >> 10;
        if (err != 0) {
            lr -= (lr > TPAQ_END_LEARN_RATE) ? 1 : 0;
            skew += err;
            if (lane < 8) myW += (myIn * err) >> 12;
        }
        c0 += c0 + (u32)bit;
        bpos--;
        if (bpos == 0) byte_done();
        const u32 sseCtx = ((c4 & 0xFF) << 8) + c0;     // _ctx0 + _c0: _ctx0 follows c4, which changes only in byte_done

        // the transitions behind the old pointers, once per lane that shares the cell
        const int last = X ? 6 : 5;
        const bool active = lane <= last;
        int mTotal = 0, mBefore = 0;
#pragma unroll
        for (int j = 0; j < 7; j++) {
            const bool eq = rl(myId, j) == myId;
            mTotal += eq ? 1 : 0;
            mBefore += (eq && j < lane) ? 1 : 0;
        }
        const u8* row = L.trans + 256 * bit;
        u32 v = myVal, pre = myVal;
#pragma unroll
        for (int k = 0; k < 5; k++) {
            if (k == mBefore) pre = v;
            if (k < mTotal) v = row[v];
        }
        if (active && mBefore == 0) st_wg(myPtr, (u8)v);
        const u32 oldId6 = rl(myId, 6), pre6 = rl(pre, 6);
        // the new pointers
        u32 idx;
        if (lane == 0) { idx = myCtx + c0; myPtr = small0 + idx; myId = 0x80000000u | idx; }
        else if (lane == 1) { idx = myCtx + c0; myPtr = small1 + idx; myId = 0xC0000000u | idx; }
        else if (active) { idx = (lane == 5 ? (myCtx ^ c0) : (myCtx + c0)) & statesMask; myPtr = big + idx; myId = idx; }
        tq_drain();
        u32 seen = 0;
        if (active) { myVal = (u32)ld_agent(myPtr); seen = (X && lane >= 2 && lane <= 5 && myId == oldId6) ? pre6 : myVal; }
        // the match model's prediction (getMatchContextPred clears the match in the middle of a byte)
        int p7 = 0;
        if (matchLen != 0) {
            if (c0 == ((u32)matchVal >> bpos)) {
                const int mp = L.matchPred[matchLen - 1];
                p7 = ((matchVal >> (bpos - 1)) & 1) ? mp : -mp;
            } else matchLen = 0;
        }
        myIn = active ? (int)L.stateMap[seen] : 0;
        if (lane == 7 || (!X && lane == 6)) myIn = p7;
        // TPAQMixer::get: the dot product over lanes 0-7
        int dot = lane < 8 ? myIn * myW : 0;
        dot += __shfl_xor(dot, 1);
        dot += __shfl_xor(dot, 2);
        dot += __shfl_xor(dot, 4);
        dot = (int)uni((u32)dot) + skew + 65536;
        int p = mixPr = tpaq_squash(L, dot >> 17);
        // SSE
        if (!X) {
            if (binCount < (pos >> 3)) p = (3 * apm0<7>(bit, p, c0) + p) >> 2;
        } else {
            if (binCount < (pos >> 3)) p = apm1(bit, p, sseCtx);
            else {
                if (binCount >= (pos >> 2)) p = (3 * apm0<6>(bit, p, c0) + p) >> 2;
                p = (3 * apm1(bit, p, sseCtx) + p) >> 2;
            }
        }
        pr = (u32)(p + (p < 2048 ? 1 : 0));
    }
};

// ------------------------------------------------------------------------------------------------
// kernels: one wave per block; block b0 + blockIdx.x, tables of slot blockIdx.x
// ------------------------------------------------------------------------------------------------
template <bool X>
__global__ __launch_bounds__(64) void k_tpaq_encode(BlockView view, const u32* __restrict__ origLen, u32 copyThreshold, int maxChunks,
                                                    ChunkDesc* __restrict__ desc, u8* __restrict__ tmp, u64 tmpStride, u32* __restrict__ ctrl,
                                                    u8* __restrict__ big, const u64* __restrict__ bigOff, int pass, u32 tier1Div,
                                                    int b0, u8* __restrict__ tables, TpaqLayout lay, u32 rbsz)
{
    __shared__ TpaqLds L;
    __shared__ u32 ring[CM_RING_WORDS];
    const int b = b0 + (int)blockIdx.x;
    const int lane = lane_id();
    const u32 count = view.len[b];
    const u8* blk = view.ptr[b];
    ChunkDesc* cds = desc + (size_t)b * maxChunks;
    if (pass == 1 && ctrl[1 + b] != 1) return;
    if (origLen[b] <= copyThreshold) {
        if (lane == 0) binary_copy_desc(cds[0], blk, count);
        return;
    }
    tpaq_lds_init(L, lane);
    __syncthreads();
    if (count > lay.abszMax) return;                    // (cannot happen: the tables were laid out for the longest block of the batch)
    u8* buf = pass ? big + bigOff[b] : tmp + (size_t)b * tmpStride;
    const u64 cap = pass ? 32ull * count + 16 : cm_stage1(count, tier1Div);
    TpaqPred<X> pr(L, lane, tables + (size_t)blockIdx.x * lay.stride, lay, rbsz, count);
    const bool full = binary_encode_block(pr, blk, count, buf, cap, cds, ring, lane);
    if (full && pass == 0 && lane == 0) { ctrl[1 + b] = 1; atomicAdd(&ctrl[0], 1u); }
}

template <bool X>
__global__ __launch_bounds__(64) void k_tpaq_decode(BitSrc src, DecBlock* __restrict__ blocks, u8* const* __restrict__ outPtr,
                                                    int b0, u8* __restrict__ tables, TpaqLayout lay, u32 rbsz)
{
    __shared__ TpaqLds L;
    const int b = b0 + (int)blockIdx.x;
    const int lane = lane_id();
    DecBlock& db = blocks[b];
    BitSrc s;
    u8* block = outPtr[b];
    if (binary_decode_head(src, db, s, block, lane)) return;
    if (db.preLen > lay.abszMax) {                      // the tables were laid out for blocks of up to abszMax bytes
        if (lane == 0) { db.error = KNZ_ERR_PROCESS_BLOCK; db.usedBits = 0; }
        return;
    }
    u64 pos = db.entropyBit;
    tpaq_lds_init(L, lane);
    __syncthreads();
    TpaqPred<X> pr(L, lane, tables + (size_t)blockIdx.x * lay.stride, lay, rbsz, db.preLen);
    const bool fail = binary_decode_block(pr, src, s, pos, db.preLen, block, lane);
    if (lane == 0) {
        if (fail) db.error = KNZ_ERR_PROCESS_BLOCK;
        db.usedBits = pos - db.entropyBit;
    }
}

// One pass of the encoder over the batch, in slices of tpaq_slice_blocks blocks: the tables are zeroed on the stream before each slice.
static void tpaq_encode_pass(hipStream_t s, int extra, BlockView view, const u32* origLen, u32 copyThreshold, int nBlocks, int maxChunks,
                             ChunkDesc* desc, u8* tmp, u64 tmpStride, u32* ctrl, u8* big, const u64* bigOff, int pass, u32 tier1Div,
                             void* tables, u32 rbsz, u32 abszMax)
{
    const TpaqLayout lay = tpaq_layout(rbsz, abszMax, extra, tpaq_states_log());
    const int per = tpaq_slice_blocks((size_t)lay.stride, nBlocks);
    for (int b0 = 0; b0 < nBlocks; b0 += per) {
        const int nb = nBlocks - b0 < per ? nBlocks - b0 : per;
        hipMemsetAsync(tables, 0, (size_t)lay.stride * nb, s);
        KScope ks_("k_tpaq_encode");
        if (extra) hipLaunchKernelGGL(k_tpaq_encode<true>, dim3(nb), dim3(64), 0, s, view, origLen, copyThreshold, maxChunks, desc, tmp, tmpStride, ctrl,
                                      big, bigOff, pass, tier1Div, b0, (u8*)tables, lay, rbsz);
        else hipLaunchKernelGGL(k_tpaq_encode<false>, dim3(nb), dim3(64), 0, s, view, origLen, copyThreshold, maxChunks, desc, tmp, tmpStride, ctrl,
                                big, bigOff, pass, tier1Div, b0, (u8*)tables, lay, rbsz);
    }
}

void launch_tpaq_encode(hipStream_t s, int extra, BlockView view, const u32* origLen, u32 copyThreshold, int nBlocks, int maxChunks, ChunkDesc* desc,
                        u8* tmp, u64 tmpStride, void* ctrlMem, void* tables, u32 rbsz, u32 abszMax)
{
    u32* ctrl = reinterpret_cast<u32*>(ctrlMem);
    hipMemsetAsync(desc, 0, sizeof(ChunkDesc) * (size_t)nBlocks * maxChunks, s);
    hipMemsetAsync(ctrl, 0, 4 * ((size_t)nBlocks + 1), s);
    tpaq_encode_pass(s, extra, view, origLen, copyThreshold, nBlocks, maxChunks, desc, tmp, tmpStride, ctrl, nullptr, nullptr, 0, cm_tier1_div(), tables, rbsz, abszMax);
}

// The rare path, as launch_cm_encode_again
int launch_tpaq_encode_again(hipStream_t s, int extra, BlockView view, const u32* origLen, u32 copyThreshold, int nBlocks, int maxChunks, ChunkDesc* desc,
                             u8* tmp, u64 tmpStride, void* ctrlMem, CmBigAlloc bigAlloc, void* user, void* tables, u32 rbsz, u32 abszMax)
{
    u32* ctrl = reinterpret_cast<u32*>(ctrlMem);
    u64* bigOff = nullptr;
    u8* big = nullptr;
    const int marked = binary_again_prepare(s, view, nBlocks, ctrlMem, bigAlloc, user, &bigOff, &big);
    if (marked < 0) return marked;
    tpaq_encode_pass(s, extra, view, origLen, copyThreshold, nBlocks, maxChunks, desc, tmp, tmpStride, ctrl, big, bigOff, 1, 0u, tables, rbsz, abszMax);
    return marked;
}

void launch_tpaq_decode(hipStream_t s, int extra, BitSrc src, DecBlock* blocks, int nBlocks, u8* const* outPtr, void* tables, u32 rbsz, u32 abszMax)
{
    const TpaqLayout lay = tpaq_layout(rbsz, abszMax, extra, tpaq_states_log());
    const int per = tpaq_slice_blocks((size_t)lay.stride, nBlocks);
    for (int b0 = 0; b0 < nBlocks; b0 += per) {
        const int nb = nBlocks - b0 < per ? nBlocks - b0 : per;
        hipMemsetAsync(tables, 0, (size_t)lay.stride * nb, s);
        KScope ks_("k_tpaq_decode");
        if (extra) hipLaunchKernelGGL(k_tpaq_decode<true>, dim3(nb), dim3(64), 0, s, src, blocks, outPtr, b0, (u8*)tables, lay, rbsz);
        else hipLaunchKernelGGL(k_tpaq_decode<false>, dim3(nb), dim3(64), 0, s, src, blocks, outPtr, b0, (u8*)tables, lay, rbsz);
    }
}

}  // namespace knz
