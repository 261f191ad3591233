"""Times ROLZX (ROLZCodec2) forward and inverse on one block and on a batch of N blocks of the benchmark's block size (8 MiB) of
corpus.text, corpus.repeats and random bytes (which the stage refuses near the block's end: the literal-only worst case): one batch
through knz_hip_encode_blocks / _decode_blocks with NONE entropy. The stage's figure is the HIP-event time of its kernel
(knz_hip_set_profiling), warm, the median of --steps runs, and MB/s of input from it. Beside it the reference's ROLZX / NONE through
ref_time_roundtrip at -j N on the same bytes (skipped where the build is absent). No threshold: the figures are a record.
    python tools/gpu_rolzx_time.py [--blocks 26] [--steps 3] [--block-mib 8] [--inputs text,repeats,random]
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


def run(ctx, data, bs, steps):
    n = len(data)
    p = ctx.params("ROLZX", "NONE", bs)
    cap = ctx.encode_bound(p, n)
    d_in, d_out, d_dec = ctx.malloc(n + 64), ctx.malloc(cap), ctx.malloc(n + bs + 64)
    ctx.h2d(d_in, data)
    te, td, kf, ki = [], [], [], []
    for prof in (False, True):
        ctx.set_profiling(prof)
        for i in range(steps + 1):
            t0 = time.perf_counter()
            bits = ctx.encode_blocks(p, d_in, n, d_out, cap)
            t1 = time.perf_counter()
            kt = ctx.kernel_times() if prof else []
            t2 = time.perf_counter()
            ob, _, _ = ctx.decode_blocks(p, d_out, bits, 0, d_dec, n + bs)
            t3 = time.perf_counter()
            assert ob == n
            if i < 1:
                continue
            if prof:
                kf.append(sum(ms for name, ms, _ in kt if name.startswith("k_rolzx")))
                ki.append(sum(ms for name, ms, _ in ctx.kernel_times() if name.startswith("k_rolzx")))
            else:
                te.append(1e3 * (t1 - t0))
                td.append(1e3 * (t3 - t2))
    ctx.set_profiling(False)
    back = ctx.d2h(d_dec, min(n, 1 << 20))
    assert back == data[:len(back)]
    for ptr in (d_in, d_out, d_dec):
        ctx.free(ptr)
    m = statistics.median
    mbs = lambda ms: round(n / 1e6 / (ms / 1e3), 2) if ms >= 0.05 else None      # noqa: E731 (None: the stage refused the blocks)
    return {"bytes": n, "blocks": (n + bs - 1) // bs, "compressed": (bits + 7) // 8, "encode_ms": round(m(te), 1), "decode_ms": round(m(td), 1),
            "forward_kernel_ms": round(m(kf), 1), "inverse_kernel_ms": round(m(ki), 1),
            "forward_MBps": mbs(m(kf)), "inverse_MBps": mbs(m(ki))}


def reference(data, bs, jobs):
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
    rc = L.ref_time_roundtrip(src.ctypes.data_as(u8p), n, b"ROLZX", b"NONE", bs, jobs, comp.ctypes.data_as(u8p), comp.size,
                              C.byref(clen), back.ctypes.data_as(u8p), C.byref(rte), C.byref(rtd))
    if rc != 0:
        return None
    return {"ref_jobs": jobs, "ref_encode_ms": round(1e3 * rte.value, 1), "ref_decode_ms": round(1e3 * rtd.value, 1),
            "ref_encode_MBps": round(n / 1e6 / rte.value, 1), "ref_decode_MBps": round(n / 1e6 / rtd.value, 1), "ref_compressed": clen.value}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=26)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--block-mib", type=int, default=8)
    ap.add_argument("--inputs", default="text,repeats,random")
    a = ap.parse_args()
    knzlib.load_pkg()
    hipapi = importlib.import_module("kanzi_amd.hipapi")
    corpus = importlib.import_module("kanzi_amd.corpus")
    import numpy as np
    ctx = hipapi.Context(0)
    bs = a.block_mib << 20
    for kind in a.inputs.split(","):
        for blocks in (1, a.blocks):
            n = blocks * bs
            data = (np.random.default_rng(3).integers(0, 256, n, dtype=np.uint8).tobytes() if kind == "random"
                    else getattr(corpus, kind)(n, 3))
            res = dict(run(ctx, data, bs, a.steps), input=kind)
            res.update(reference(data, bs, min(blocks, 16)) or {})
            print(json.dumps(res), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
