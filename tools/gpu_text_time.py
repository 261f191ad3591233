"""Times TEXT (TextCodec) forward and inverse on N blocks of 8 MiB of corpus().text (a different seed for every block), for codec 1
(entropy FPAQ) and codec 2 (entropy NONE): one batch through knz_hip_encode_blocks / _decode_blocks; the stage's figure is the HIP-event
time of its kernels (knz_hip_set_profiling), warm, the median of --steps runs, with the kernels listed one by one. Beside it
knz_host_text_forward / _inverse (host/text_codec.cpp) on one core over the same blocks, and the reference's TEXT / NONE through
ref_time_roundtrip on one core (-j 1; skipped where the build is absent).
    python tools/gpu_text_time.py [--blocks 26] [--steps 3]
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


def text_blocks(blocks):
    corpus = knzlib.corpus()
    return b"".join(corpus.text(BS, 100 + b) for b in range(blocks))


def stage(ctx, data, entropy, steps):
    n = len(data)
    p = ctx.params("TEXT", entropy, BS)
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
        kf.append(sum(ms for name, ms, _ in kt if name.startswith("k_tx_")))
        ki.append(sum(ms for name, ms, _ in kd if name.startswith("k_tx_")))
        for name, ms, _ in list(kt) + list(kd):
            if name.startswith("k_tx_"):
                names.setdefault(name, []).append(ms)
    ctx.set_profiling(False)
    assert ctx.d2h(d_dec, 1 << 20) == data[:1 << 20]
    for ptr in (d_in, d_out, d_dec):
        ctx.free(ptr)
    m = statistics.median
    return {"entropy": entropy, "bytes": n, "compressed": (bits + 7) // 8,
            "text_forward_kernels_ms": round(m(kf), 3), "text_inverse_kernels_ms": round(m(ki), 3),
            "kernels_ms": {k: round(m(v), 3) for k, v in sorted(names.items())}}


def host(data, variant):
    """knz_host_text_forward / _inverse over the blocks, one after another on one core"""
    L = C.CDLL(os.path.join(knzlib.PKG, "libkanzi_amd.so"))
    u8p = C.POINTER(C.c_uint8)
    L.knz_host_text_forward.argtypes = [C.c_int, u8p, C.c_int, u8p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.knz_host_text_inverse.argtypes = [C.c_int, u8p, C.c_int, u8p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int)]
    tf = ti = 0.0
    out, back = (C.c_uint8 * (BS + 64))(), (C.c_uint8 * (BS + 64))()
    for off in range(0, len(data), BS):
        blk = data[off:off + BS]
        src = (C.c_uint8 * len(blk)).from_buffer_copy(blk)
        dt, ol, bl = C.c_int(0), C.c_int(0), C.c_int(0)
        t0 = time.perf_counter()
        ok = L.knz_host_text_forward(variant, src, len(blk), out, len(blk), BS, 6, C.byref(dt), C.byref(ol))
        t1 = time.perf_counter()
        assert ok
        ok = L.knz_host_text_inverse(variant, out, ol.value, back, len(blk), BS, 6, C.byref(bl))
        t2 = time.perf_counter()
        assert ok and bl.value == len(blk)
        tf += t1 - t0
        ti += t2 - t1
    return {"host_forward_ms": round(1e3 * tf, 1), "host_inverse_ms": round(1e3 * ti, 1)}


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
    for chain in ("TEXT", "NONE"):                # (NONE / NONE: what the stream costs without the stage)
        clen, rte, rtd = C.c_size_t(0), C.c_double(0), C.c_double(0)
        rc = L.ref_time_roundtrip(src.ctypes.data_as(u8p), n, chain.encode(), b"NONE", BS, jobs, comp.ctypes.data_as(u8p), comp.size,
                                  C.byref(clen), back.ctypes.data_as(u8p), C.byref(rte), C.byref(rtd))
        if rc != 0:
            return None
        k = chain.lower()
        out.update({"ref_jobs": jobs, "ref_%s_encode_ms" % k: round(1e3 * rte.value, 1), "ref_%s_decode_ms" % k: round(1e3 * rtd.value, 1)})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=26)
    ap.add_argument("--steps", type=int, default=3)
    a = ap.parse_args()
    knzlib.load_pkg()
    hipapi = importlib.import_module("kanzi_amd.hipapi")
    data = text_blocks(a.blocks)
    ctx = hipapi.Context(0)
    for entropy, variant in (("FPAQ", 1), ("NONE", 2)):
        res = {"codec": variant}
        res.update(stage(ctx, data, entropy, a.steps))
        res.update(host(data, variant))
        print(json.dumps(res), flush=True)
    ctx.close()
    print(json.dumps(reference(data, 1) or {}), flush=True)


if __name__ == "__main__":
    main()
