"""Times LZP (LZPCodec) forward and inverse on N blocks of 8 MiB of corpus.repeats, corpus.text and random bytes (the literal-only worst
case): one batch through knz_hip_encode_blocks / _decode_blocks with NONE entropy; the stage's figure is the HIP-event time of its kernel
(knz_hip_set_profiling), warm, the median of --steps runs. Beside it the reference's LZP / NONE through ref_time_roundtrip at -j N on the
same bytes (skipped where the build is absent). Then the question LZP is there for: real files (corpus.local, --local-limit bytes) through
BWT+MTFT+ZRLT / ANS0 and through LZP+BWT+MTFT+ZRLT / ANS0: whole-call encode time, the kernels' time without LZP's, LZP's own, compressed size.
    python tools/gpu_lzp_time.py [--blocks 26] [--steps 5] [--local-limit 218103808]
"""
import argparse
import ctypes as C
import importlib
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import knzlib  # noqa: E402

BS = 8 << 20


def run(ctx, chain, entropy, data, steps):
    n = len(data)
    p = ctx.params(chain, entropy, BS)
    cap = ctx.encode_bound(p, n)
    d_in, d_out, d_dec = ctx.malloc(n + 64), ctx.malloc(cap), ctx.malloc(n + BS + 64)
    ctx.h2d(d_in, data)
    te, td, lf, li, other = [], [], [], [], []
    for prof in (False, True):
        ctx.set_profiling(prof)
        for i in range(steps + 1):
            t0 = time.perf_counter()
            bits = ctx.encode_blocks(p, d_in, n, d_out, cap)
            t1 = time.perf_counter()
            kt = ctx.kernel_times() if prof else []
            t2 = time.perf_counter()
            ob, _, _ = ctx.decode_blocks(p, d_out, bits, 0, d_dec, n + BS)
            t3 = time.perf_counter()
            assert ob == n
            if i < 1:
                continue
            if prof:
                lf.append(sum(ms for name, ms, _ in kt if name.startswith("k_lzp")))
                other.append(sum(ms for name, ms, _ in kt if not name.startswith("k_lzp")))
                li.append(sum(ms for name, ms, _ in ctx.kernel_times() if name.startswith("k_lzp")))
            else:
                te.append(1e3 * (t1 - t0))
                td.append(1e3 * (t3 - t2))
    ctx.set_profiling(False)
    back = ctx.d2h(d_dec, min(n, 1 << 20))
    assert back == data[:len(back)]
    for ptr in (d_in, d_out, d_dec):
        ctx.free(ptr)
    m = statistics.median
    return {"chain": chain, "entropy": entropy, "bytes": n, "compressed": (bits + 7) // 8, "encode_ms": round(m(te), 2), "decode_ms": round(m(td), 2),
            "lzp_forward_kernel_ms": round(m(lf), 3), "lzp_inverse_kernel_ms": round(m(li), 3), "other_encode_kernels_ms": round(m(other), 2)}


def reference(data, chain, entropy, jobs):
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
    clen, rte, rtd = C.c_size_t(0), C.c_double(0), C.c_double(0)
    rc = L.ref_time_roundtrip(src.ctypes.data_as(u8p), n, chain.encode(), entropy.encode(), BS, jobs, comp.ctypes.data_as(u8p), comp.size,
                              C.byref(clen), back.ctypes.data_as(u8p), C.byref(rte), C.byref(rtd))
    if rc != 0:
        return None
    return {"ref_jobs": jobs, "ref_encode_ms": round(1e3 * rte.value, 1), "ref_decode_ms": round(1e3 * rtd.value, 1), "ref_compressed": clen.value}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=26)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--local-limit", type=int, default=26 * BS)
    a = ap.parse_args()
    knzlib.load_pkg()
    hipapi = importlib.import_module("kanzi_amd.hipapi")
    corpus = importlib.import_module("kanzi_amd.corpus")
    import numpy as np
    ctx = hipapi.Context(0)
    n = a.blocks * BS
    for kind, data in (("repeats", corpus.repeats(n, 3)), ("text", corpus.text(n, 3)),
                       ("random", np.random.default_rng(3).integers(0, 256, n, dtype=np.uint8).tobytes())):
        res = dict(run(ctx, "LZP", "NONE", data, a.steps), input=kind)
        res.update(reference(data, "LZP", "NONE", a.blocks) or {})
        print(json.dumps(res), flush=True)
    if a.local_limit > 0:
        data, _, desc = corpus.local(a.local_limit)
        for chain in ("BWT+MTFT+ZRLT", "LZP+BWT+MTFT+ZRLT"):
            print(json.dumps(dict(run(ctx, chain, "ANS0", data, a.steps), input="local: " + desc)), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
