// rANS table construction shared by the order-0 (ans.hip) and order-1 (ans1.hip) encoders.
#pragma once
#include "common.hpp"

namespace knz {

// ------------------------------------------------------------------------------------------------
// Byte counts of one chunk by one wave (Global.cpp:170-221), shared by the order-0 rANS and the RANGE statistics kernels: 16 bytes per
// lane per iteration into 8 private histograms chosen by lane -- one ds_add instruction never sends more than 8 lanes to the same copy,
// which is what bounds the same-address serialisation on skewed data (text: 15 % spaces). Row stride 264: copy c of a symbol sits 8c
// banks away, not in the same bank. `hist` must be zero; f[k] = count of symbol 4 * lane + k.
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ void ans_chunk_counts(int lane, const u8* blk, u32 n, u32 (*hist)[264], u32 f[4])
{
    u32* myHist = hist[lane & 7];
    const u32 n16 = n & ~15u;
    const bool aligned = ((reinterpret_cast<uintptr_t>(blk) & 15) == 0);
    if (aligned) {
        const uint4* p4 = reinterpret_cast<const uint4*>(blk);
        for (u32 i = lane; i < (n16 >> 4); i += 64) {
            const uint4 v = p4[i];
            const u32 w[4] = { v.x, v.y, v.z, v.w };
#pragma unroll
            for (int k = 0; k < 4; k++) {
                atomicAdd(&myHist[w[k] & 0xFF], 1u);
                atomicAdd(&myHist[(w[k] >> 8) & 0xFF], 1u);
                atomicAdd(&myHist[(w[k] >> 16) & 0xFF], 1u);
                atomicAdd(&myHist[w[k] >> 24], 1u);
            }
        }
    } else {
        for (u32 i = lane; i < n16; i += 64) atomicAdd(&myHist[blk[i]], 1u);
    }
    for (u32 i = n16 + lane; i < n; i += 64) atomicAdd(&myHist[blk[i]], 1u);
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int s = 4 * lane + k;
        u32 acc = 0;
#pragma unroll
        for (int c = 0; c < 8; c++) acc += hist[c][s];
        f[k] = acc;
    }
}

// ------------------------------------------------------------------------------------------------
// pieces shared by order 0 (one table per 16 KiB chunk) and order 1 (one table per context of a 4 MiB chunk);
// one wave, lane owns symbols 4*lane .. 4*lane+3
// ------------------------------------------------------------------------------------------------
// (LR a run-time value: the RANGE coder lowers it for short chunks; the rANS coders pass a constant through the wrappers below, which the
// compiler folds)
__device__ __forceinline__ void ans_normalize_lr(int lane, u32 f[4], u32 n, u32 asz, const u32 LR)
{
    const u32 SCALE = 1u << LR;
    // normalizeFrequencies (EntropyUtils.cpp:131-245), totalFreq = n, scale = 2^LR
    if (n != SCALE) {
        if (asz == 1) {
#pragma unroll
            for (int k = 0; k < 4; k++) if (f[k]) f[k] = SCALE;
        } else {
            u32 ssum = 0;
#pragma unroll
            for (int k = 0; k < 4; k++) {
                if (f[k]) {
                    if (n <= (1u << (31 - LR))) {                       // 32-bit arithmetic is exact here
                        const u32 sf = f[k] * SCALE;
                        f[k] = (sf <= n) ? 1u : (sf + (n >> 1)) / n;
                    } else {
                        const u64 sf = (u64)f[k] * SCALE;
                        f[k] = (sf <= (u64)n) ? 1u : (u32)((sf + (n >> 1)) / n);
                    }
                    ssum += f[k];
                }
            }
            const u32 sumScaled = wave_sum(ssum);
            if (sumScaled != SCALE) {
                // idxMax = first index holding the maximum scaled frequency
                u32 key = 0;
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    const u32 kk = (f[k] << 8) | (255u - (u32)(4 * lane + k));
                    key = kk > key ? kk : key;
                }
                key = wave_max(key);
                const u32 idxMax = 255u - (key & 0xFF);
                const u32 fmax = key >> 8;
                int delta = (int)sumScaled - (int)SCALE;
                const int errThr = (int)(fmax >> 4);
                const bool ownMax = ((idxMax >> 2) == (u32)lane);
                const int km = (int)(idxMax & 3);
                if (abs(delta) <= errThr) {
                    if (ownMax) {
#pragma unroll
                        for (int k = 0; k < 4; k++) if (k == km) f[k] -= (u32)delta;
                    }
                } else {
                    if (delta < 0) {
                        delta += errThr;
                        if (ownMax) {
#pragma unroll
                            for (int k = 0; k < 4; k++) if (k == km) f[k] += (u32)errThr;
                        }
                    } else {
                        delta -= errThr;
                        if (ownMax) {
#pragma unroll
                            for (int k = 0; k < 4; k++) if (k == km) f[k] -= (u32)errThr;
                        }
                    }
                    const int inc = (delta < 0) ? 1 : -1;
                    delta = abs(delta);
                    int round = 0;
                    while ((++round < 6) && (delta > 0)) {
                        // symbols with f > 2, in alphabet order, each get one adjustment until delta runs out
                        u32 elig = 0;
#pragma unroll
                        for (int k = 0; k < 4; k++) elig |= (f[k] > 2 ? 1u : 0u) << k;
                        const u32 ec = __popc(elig);
                        const u32 incl = wave_incl_scan(ec);
                        const u32 totalElig = (u32)__shfl((int)incl, 63, 64);
                        u32 r = incl - ec;
#pragma unroll
                        for (int k = 0; k < 4; k++) {
                            if ((elig >> k) & 1) {
                                if (r < (u32)delta) f[k] += (u32)inc;
                                r++;
                            }
                        }
                        if (totalElig == 0) break;
                        delta -= (int)((totalElig < (u32)delta) ? totalElig : (u32)delta);
                    }
                    if (ownMax) {
#pragma unroll
                        for (int k = 0; k < 4; k++) {
                            if (k == km) {
                                const u32 v = f[k] - (u32)delta;      // uint32 wrap as in the reference
                                f[k] = v > 1u ? v : 1u;
                            }
                        }
                    }
                }
            }
        }
    }

}

template <u32 LR>
__device__ void ans_normalize(int lane, u32 f[4], u32 n, u32 asz) { ans_normalize_lr(lane, f, n, asz, LR); }

// Appends the alphabet + frequency groups of one table to the LDS bit buffer `hdrw` at bit `pos`
// (ANSRangeEncoder.cpp:119-155, EntropyUtils.cpp:57-89); returns the new position. The 3 bits of LR - 8 go in front of the alphabet
// (lrWhere 1: rANS order 0), behind a non-empty one (2: RANGE, RangeEncoder.cpp:83-93) or nowhere (0).
__device__ __forceinline__ u32 ans_header_bits_lr(int lane, const u32 f[4], u32 present, u32 asz, u32 rankBase, int lrWhere, const u32 LR,
                                                  u32* hdrw, u32* grpMax, u32* grpOff, u32 pos)
{
    if (lrWhere == 1) { if (lane == 0) or_bits_words(hdrw, pos, LR - 8, 3); pos += 3; }
    if (asz == 0) {
        if (lane == 0) or_bits_words(hdrw, pos, 1, 2);   // FULL_ALPHABET(0), ALPHABET_0(1)
        pos += 2;
    } else if (asz == 256) {
        pos += 2;                                   // FULL_ALPHABET(0), ALPHABET_256(0)
    } else {
        // PARTIAL_ALPHABET(1), 5 bits lastMask, masks
        const u64 anyMask = __ballot(present != 0);
        const int lastLane = 63 - __clzll((long long)anyMask);
        const u32 lastMask = (u32)lastLane >> 1;    // symbol >> 3 == lane >> 1
        if (lane == 0) {
            or_bits_words(hdrw, pos, 1, 1);
            or_bits_words(hdrw, pos + 1, lastMask, 5);
        }
        pos += 6;
        // mask byte m: low nibble from lane 2m, high nibble from lane 2m+1 ; bit (s&7) = symbol present
        const u32 other = (u32)__shfl_xor((int)present, 1, 64);
        if ((lane & 1) == 0 && ((u32)lane >> 1) <= lastMask) {
            const u32 byte = present | (other << 4);
            or_bits_words(hdrw, pos + 8 * ((u32)lane >> 1), byte, 8);
        }
        pos += 8 * (lastMask + 1);
    }
    if (lrWhere == 2 && asz != 0) { if (lane == 0) or_bits_words(hdrw, pos, LR - 8, 3); pos += 3; }

    if (asz > 1) {
        const u32 chk = (asz >= 64) ? 8u : 6u;
        const u32 llr = 4;                           // log2(LR) + 1 for every LR from 8 to 15
        // per group maximum of bitlen(f-1) over alphabet indices 1..asz-1
        u32 r = rankBase;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            if (f[k]) {
                if (r >= 1) atomicMax(&grpMax[(r - 1) / chk], bitlen_u32(f[k] - 1));
                r++;
            }
        }
        __syncthreads();
        const u32 nGroups = (asz - 1 + chk - 1) / chk;
        u32 gbits = 0;
        if ((u32)lane < nGroups) {
            const u32 first = 1 + (u32)lane * chk;
            const u32 cnt = (first + chk <= asz) ? chk : (asz - first);
            gbits = llr + cnt * grpMax[lane];
        }
        const u32 gincl = wave_incl_scan(gbits);
        const u32 totalFreqBits = (u32)__shfl((int)gincl, 63, 64);
        const u32 goff = gincl - gbits;
        if ((u32)lane < nGroups) or_bits_words(hdrw, pos + goff, grpMax[lane], llr);
        // stash group offsets for the members
        grpOff[lane] = goff;
        __syncthreads();
        r = rankBase;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            if (f[k]) {
                if (r >= 1) {
                    const u32 g = (r - 1) / chk;
                    const u32 lm = grpMax[g];
                    if (lm) or_bits_words(hdrw, pos + grpOff[g] + llr + ((r - 1) - g * chk) * lm, f[k] - 1, lm);
                }
                r++;
            }
        }
        pos += totalFreqBits;
    }
    __syncthreads();

    return pos;
}

template <u32 LR>
__device__ u32 ans_header_bits(int lane, const u32 f[4], u32 present, u32 asz, u32 rankBase, bool lrPrefix,
                               u32* hdrw, u32* grpMax, u32* grpOff, u32 pos)
{
    return ans_header_bits_lr(lane, f, present, asz, rankBase, lrPrefix ? 1 : 0, LR, hdrw, grpMax, grpOff, pos);
}

// ANSEncSymbol::reset for the 4 symbols of every lane (ANSRangeEncoder.hpp:92-117)
template <u32 LR>
__device__ void ans_enc_table(int lane, const u32 f[4], uint2* tab)
{
    constexpr u32 SCALE = 1u << LR;
    {
        // cumulative frequencies in symbol order; ANSEncSymbol::reset (ANSRangeEncoder.hpp:92-117)
        const u32 lsum = f[0] + f[1] + f[2] + f[3];
        const u32 lincl = wave_incl_scan(lsum);
        u32 cum = lincl - lsum;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            u32 fr = f[k];
            uint2 e = make_uint2(0, 0);
            if (fr) {
                if (fr >= SCALE) fr = SCALE - 1;
                if (fr < 2) {
                    e.x = 0xFFFFFFFFu;
                    e.y = fr | (0u << 13) | ((cum + SCALE - 1) << 17);
                } else {
                    u32 shift = 0;
                    while (fr > (1u << shift)) shift++;
                    const u64 inv = (((1ull << (shift + 31)) + fr - 1) / fr) & 0xFFFFFFFFull;
                    e.x = (u32)inv;
                    e.y = fr | ((shift - 1) << 13) | (cum << 17);      // invShift - 32 = shift - 1
                }
            }
            tab[4 * lane + k] = e;
            cum += f[k];
        }
    }
}

}  // namespace knz
