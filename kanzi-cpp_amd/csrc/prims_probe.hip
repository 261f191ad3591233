// Test entry to prims.hpp (knz_hip_prims_info / _scan / _sort): the device-wide scans and the segmented radix sort run by themselves on
// arrays the caller owns, so that tests can compare them with a host reference at the sizes where the kernels change path. Every buffer
// the primitives write into that the caller does not own (scan scratch, sort workspace, ping-pong arrays) sits between two guards of
// a fixed byte pattern that are checked after the run: a write just outside a buffer would otherwise land in allocator slack unseen.
// No kernels of its own.
#include "common.hpp"
#include "stages.hpp"
#include "prims.hpp"

#include <stdarg.h>
#include <stdio.h>
#include <string.h>
#include <vector>

namespace knz {

namespace {

constexpr size_t PP_GUARD = 4096;
constexpr int PP_GUARD_BYTE = 0xA7;
constexpr int PP_FILL_BYTE = 0x5C;           // what a buffer holds before the primitive runs: nothing may count on zeroes

struct PpBuf { u8* raw; size_t payload; const char* name; };

struct Probe {
    hipStream_t s;
    char* err;
    size_t errCap;
    std::vector<PpBuf> bufs;

    Probe(hipStream_t s_, char* err_, size_t errCap_) : s(s_), err(err_), errCap(errCap_) {}
    Probe(const Probe&) = delete;
    Probe& operator=(const Probe&) = delete;
    ~Probe() { for (const PpBuf& b : bufs) (void)hipFree(b.raw); }

    int say(int code, const char* fmt, ...)
    {
        va_list ap;
        va_start(ap, fmt);
        if (err != nullptr && errCap != 0) vsnprintf(err, errCap, fmt, ap);
        va_end(ap);
        return code;
    }
};

#define PPCHK(p, call) do { hipError_t e_ = (call); if (e_ != hipSuccess) return (p).say(-1, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, __LINE__); } while (0)

// `bytes` of device memory between two guards (the payload is rounded up to 256 bytes, which the guards follow directly)
int pp_alloc(Probe& p, const char* name, size_t bytes, u8** out)
{
    const size_t payload = (bytes + 255) & ~(size_t)255;
    u8* raw = nullptr;
    PPCHK(p, hipMalloc(reinterpret_cast<void**>(&raw), payload + 2 * PP_GUARD));
    p.bufs.push_back(PpBuf{ raw, payload, name });
    PPCHK(p, hipMemsetAsync(raw, PP_GUARD_BYTE, PP_GUARD, p.s));
    if (payload) PPCHK(p, hipMemsetAsync(raw + PP_GUARD, PP_FILL_BYTE, payload, p.s));
    PPCHK(p, hipMemsetAsync(raw + PP_GUARD + payload, PP_GUARD_BYTE, PP_GUARD, p.s));
    *out = raw + PP_GUARD;
    return 0;
}

// (the stream has been synchronised)
int pp_check_guards(Probe& p)
{
    std::vector<u8> h(2 * PP_GUARD);
    for (const PpBuf& b : p.bufs) {
        PPCHK(p, hipMemcpy(h.data(), b.raw, PP_GUARD, hipMemcpyDeviceToHost));
        PPCHK(p, hipMemcpy(h.data() + PP_GUARD, b.raw + PP_GUARD + b.payload, PP_GUARD, hipMemcpyDeviceToHost));
        for (size_t i = 0; i < 2 * PP_GUARD; i++) {
            if (h[i] == (u8)PP_GUARD_BYTE) continue;
            if (i < PP_GUARD) return p.say(-3, "%s: byte %zu in front of the buffer was overwritten", b.name, PP_GUARD - i);
            return p.say(-3, "%s: byte %zu behind the buffer (%zu bytes) was overwritten", b.name, i - PP_GUARD, b.payload);
        }
    }
    return 0;
}

template <class KEY, bool HAS_VAL>
int pp_sort(Probe& p, int keep, bool oneRead, const KEY* keys, const u32* vals, const u32* segBase, int nSeg, size_t n, size_t maxSegLen, int loBit,
            int hiBit, KEY* keysOut, u32* valsOut)
{
    hipStream_t s = p.s;
    u8 *wsMem = nullptr, *kx = nullptr, *ky = nullptr, *vx = nullptr, *vy = nullptr;
    if (int r = pp_alloc(p, "sort workspace", prims::rs_ws_bytes(n, nSeg), &wsMem)) return r;
    if (int r = pp_alloc(p, keep ? "keys b" : "keys a", n * sizeof(KEY), &kx)) return r;
    if (int r = pp_alloc(p, keep ? "keys c" : "keys b", n * sizeof(KEY), &ky)) return r;
    if (HAS_VAL) {
        if (int r = pp_alloc(p, keep ? "values b" : "values a", n * 4, &vx)) return r;
        if (int r = pp_alloc(p, keep ? "values c" : "values b", n * 4, &vy)) return r;
    }
    KEY *k0 = reinterpret_cast<KEY*>(kx), *k1 = reinterpret_cast<KEY*>(ky);
    u32 *v0 = reinterpret_cast<u32*>(vx), *v1 = reinterpret_cast<u32*>(vy);
    const prims::RsWs rs = prims::rs_carve(wsMem, n, nSeg, segBase, nSeg);
    prims::rs_launch_layout(s, rs);
    int res;
    if (keep) {
        res = prims::rs_sort_keep<KEY, HAS_VAL>(s, rs, keys, vals, k0, k1, v0, v1, maxSegLen, loBit, hiBit, oneRead);
    } else {
        PPCHK(p, hipMemcpyAsync(k0, keys, n * sizeof(KEY), hipMemcpyDeviceToDevice, s));
        if (HAS_VAL) PPCHK(p, hipMemcpyAsync(v0, vals, n * 4, hipMemcpyDeviceToDevice, s));
        res = prims::rs_sort<KEY, HAS_VAL>(s, rs, k0, k1, v0, v1, maxSegLen, loBit, hiBit, oneRead);
    }
    PPCHK(p, hipGetLastError());
    PPCHK(p, hipMemcpyAsync(keysOut, res ? k1 : k0, n * sizeof(KEY), hipMemcpyDeviceToDevice, s));
    if (HAS_VAL) PPCHK(p, hipMemcpyAsync(valsOut, res ? v1 : v0, n * 4, hipMemcpyDeviceToDevice, s));
    PPCHK(p, hipStreamSynchronize(s));
    return pp_check_guards(p);
}

}  // namespace

void prims_probe_info(u32 out[4])
{
    out[0] = prims::RS_TILE; out[1] = prims::RS_GROUP; out[2] = prims::SC_TILE; out[3] = (u32)prims::RS_MAXPASS;
}

int prims_probe_scan(hipStream_t s, int op, const u32* in, u32* out, size_t nMax, const u32* nDev, u32* totalOut, char* err, size_t errCap)
{
    Probe p(s, err, errCap);
    if (op != prims::SCAN_SUM_EXCL && op != prims::SCAN_MAX_INCL && op != prims::SCAN_MIN_INCL) return p.say(KNZ_ERR_INVALID_PARAM, "unknown op %d", op);
    if (totalOut != nullptr && op != prims::SCAN_SUM_EXCL) return p.say(KNZ_ERR_INVALID_PARAM, "a total exists for the sum only");
    if (nMax == 0) return 0;                                                     // (launch_scan launches nothing)
    if (nMax > ((size_t)1 << 31)) return p.say(KNZ_ERR_INVALID_PARAM, "%zu words are more than the probe takes", nMax);
    if (in == nullptr || out == nullptr || ((reinterpret_cast<uintptr_t>(in) | reinterpret_cast<uintptr_t>(out)) & 15) != 0)
        return p.say(KNZ_ERR_INVALID_PARAM, "the arrays must be 16-byte aligned");
    u8* tmp = nullptr;
    if (int r = pp_alloc(p, "scan scratch", prims::scan_tmp_bytes(nMax), &tmp)) return r;
    if (op == prims::SCAN_SUM_EXCL) prims::launch_scan<prims::SCAN_SUM_EXCL>(s, in, out, nMax, nDev, tmp, totalOut);
    else if (op == prims::SCAN_MAX_INCL) prims::launch_scan<prims::SCAN_MAX_INCL>(s, in, out, nMax, nDev, tmp);
    else prims::launch_scan<prims::SCAN_MIN_INCL>(s, in, out, nMax, nDev, tmp);
    PPCHK(p, hipGetLastError());
    PPCHK(p, hipStreamSynchronize(s));
    return pp_check_guards(p);
}

int prims_probe_sort(hipStream_t s, int keyBytes, int hasVal, int keep, int oneRead, const void* keys, const u32* vals, const u32* segBase, int nSeg,
                     size_t maxSegLen, int loBit, int hiBit, void* keysOut, u32* valsOut, char* err, size_t errCap)
{
    Probe p(s, err, errCap);
    if (keyBytes != 4 && keyBytes != 8) return p.say(KNZ_ERR_INVALID_PARAM, "keys of %d bytes", keyBytes);
    if ((hasVal != 0 && hasVal != 1) || (keep != 0 && keep != 1) || (oneRead != 0 && oneRead != 1)) return p.say(KNZ_ERR_INVALID_PARAM, "a flag is neither 0 nor 1");
    if (loBit < 0 || hiBit <= loBit || hiBit > 8 * keyBytes) return p.say(KNZ_ERR_INVALID_PARAM, "bits [%d,%d) of a %d-bit key", loBit, hiBit, 8 * keyBytes);
    if (nSeg < 1 || nSeg > 65535) return p.say(KNZ_ERR_INVALID_PARAM, "%d segments (1..65535: one row of the grid each)", nSeg);
    if (keys == nullptr || keysOut == nullptr || segBase == nullptr || (hasVal && (vals == nullptr || valsOut == nullptr))) return p.say(KNZ_ERR_INVALID_PARAM, "null array");
    if (oneRead && prims::rs_onesweep_knob().load() == 0) return p.say(KNZ_ERR_INVALID_PARAM, "one_read = 1 while the knob rs_onesweep is 0");
    // the kernels trust the segment table: check it here
    std::vector<u32> base((size_t)nSeg + 1);
    PPCHK(p, hipMemcpyAsync(base.data(), segBase, 4 * base.size(), hipMemcpyDeviceToHost, s));
    PPCHK(p, hipStreamSynchronize(s));
    if (base[0] != 0) return p.say(KNZ_ERR_INVALID_PARAM, "the first segment starts at %u", base[0]);
    for (int g = 0; g < nSeg; g++) {
        if (base[g + 1] < base[g]) return p.say(KNZ_ERR_INVALID_PARAM, "segment %d ends in front of its start", g);
        if ((size_t)(base[g + 1] - base[g]) > maxSegLen) return p.say(KNZ_ERR_INVALID_PARAM, "segment %d has %u keys, max_seg_len is %zu", g, base[g + 1] - base[g], maxSegLen);
    }
    const size_t n = base[nSeg];
    if (n == 0) return 0;
    if (n >= (size_t)prims::RS_VAL_MASK) return p.say(KNZ_ERR_INVALID_PARAM, "%zu keys are more than the probe takes", n);
    if (keyBytes == 8) {
        if (hasVal) return pp_sort<u64, true>(p, keep, oneRead != 0, reinterpret_cast<const u64*>(keys), vals, segBase, nSeg, n, maxSegLen, loBit, hiBit, reinterpret_cast<u64*>(keysOut), valsOut);
        return pp_sort<u64, false>(p, keep, oneRead != 0, reinterpret_cast<const u64*>(keys), nullptr, segBase, nSeg, n, maxSegLen, loBit, hiBit, reinterpret_cast<u64*>(keysOut), nullptr);
    }
    if (hasVal) return pp_sort<u32, true>(p, keep, oneRead != 0, reinterpret_cast<const u32*>(keys), vals, segBase, nSeg, n, maxSegLen, loBit, hiBit, reinterpret_cast<u32*>(keysOut), valsOut);
    return pp_sort<u32, false>(p, keep, oneRead != 0, reinterpret_cast<const u32*>(keys), nullptr, segBase, nSeg, n, maxSegLen, loBit, hiBit, reinterpret_cast<u32*>(keysOut), nullptr);
}

}  // namespace knz
