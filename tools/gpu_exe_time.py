"""Times EXE (EXECodec) forward and inverse on N blocks of 8 MiB of the x86 generator of tests/exe_cases.py (1 MiB of it, repeated
from a different offset for every block): one batch through knz_hip_encode_blocks / _decode_blocks with NONE entropy; the stage's figure
is the HIP-event time of its kernels (knz_hip_set_profiling), warm, the median of --steps runs, with the kernels listed one by one.
Beside it the reference's EXE / NONE through ref_time_roundtrip on one core (-j 1) on the same bytes (skipped where the build is absent).
    python tools/gpu_exe_time.py [--blocks 26] [--steps 5]
"""
import argparse
import ctypes as C
import importlib
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import exe_cases  # noqa: E402
import knzlib  # noqa: E402

BS = 8 << 20


def x86_blocks(blocks):
    unit = exe_cases.make(exe_cases.TIME_UNIT)
    out = bytearray()
    for b in range(blocks):
        off = (b * 65521) % len(unit)
        out += ((unit[off:] + unit) + unit * (BS // len(unit)))[:BS]
    return bytes(out)


def stage(ctx, data, steps):
    n = len(data)
    p = ctx.params("EXE", "NONE", BS)
    cap = ctx.encode_bound(p, n)
    d_in, d_out, d_dec = ctx.malloc(n + 64), ctx.malloc(cap), ctx.malloc(n + BS + 64)
    ctx.h2d(d_in, data)
    kf, ki, names = [], [], {}
    ctx.set_profiling(True)
    for i in range(steps + 1):
        bits = ctx.encode_blocks(p, d_in, n, d_out, cap)
        kt = ctx.kernel_times()
        ob, _, _ = ctx.decode_blocks(p, d_out, bits, 0, d_dec, n + BS)
        kd = ctx.kernel_times()
        assert ob == n
        if i < 1:
            continue
        kf.append(sum(ms for name, ms, _ in kt if name.startswith("k_ex_")))
        ki.append(sum(ms for name, ms, _ in kd if name.startswith("k_ex_")))
        for name, ms, _ in list(kt) + list(kd):
            if name.startswith("k_ex_"):
                names.setdefault(name, []).append(ms)
    ctx.set_profiling(False)
    assert ctx.d2h(d_dec, 1 << 20) == data[:1 << 20]
    for ptr in (d_in, d_out, d_dec):
        ctx.free(ptr)
    m = statistics.median
    return {"chain": "EXE", "entropy": "NONE", "bytes": n, "compressed": (bits + 7) // 8,
            "exe_forward_kernels_ms": round(m(kf), 3), "exe_inverse_kernels_ms": round(m(ki), 3),
            "kernels_ms": {k: round(m(v), 3) for k, v in sorted(names.items())}}


def reference(data, jobs):
    so = knzlib.ensure_ref()
    if so is None:
        return None
    import numpy as np
    L = C.CDLL(so)
    u8p = C.POINTER(C.c_uint8)
    L.ref_time_roundtrip.restype = C.c_int
    L.ref_time_roundtrip.argtypes = [u8p, C.c_size_t, C.c_char_p, C.c_char_p, C.c_int, C.c_int, u8p, C.c_size_t,
                                     C.POINTER(C.c_size_t), u8p, C.POINTER(C.c_double), C.POINTER(C.c_double)]
    n = len(data)
    src = np.frombuffer(data, dtype=np.uint8)
    comp = np.empty(n + n // 2 + (1 << 20), dtype=np.uint8)
    back = np.empty(n, dtype=np.uint8)
    out = {}
    for chain in ("EXE", "NONE"):                 # (NONE / NONE: what the stream costs without the stage)
        clen, rte, rtd = C.c_size_t(0), C.c_double(0), C.c_double(0)
        rc = L.ref_time_roundtrip(src.ctypes.data_as(u8p), n, chain.encode(), b"NONE", BS, jobs, comp.ctypes.data_as(u8p), comp.size,
                                  C.byref(clen), back.ctypes.data_as(u8p), C.byref(rte), C.byref(rtd))
        if rc != 0:
            return None
        k = chain.lower()
        out.update({"ref_jobs": jobs, "ref_%s_encode_ms" % k: round(1e3 * rte.value, 1), "ref_%s_decode_ms" % k: round(1e3 * rtd.value, 1),
                    "ref_%s_compressed" % k: clen.value})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=26)
    ap.add_argument("--steps", type=int, default=5)
    a = ap.parse_args()
    knzlib.load_pkg()
    hipapi = importlib.import_module("kanzi_amd.hipapi")
    data = x86_blocks(a.blocks)
    ctx = hipapi.Context(0)
    res = stage(ctx, data, a.steps)
    ctx.close()
    res.update(reference(data, 1) or {})
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
