"""Times UTF (UTFCodec) forward and inverse on N blocks of 8 MiB of the utf8 test vector (4 MiB of it, repeated from a different offset
for every block), and of real UTF-8 files where corpus.local has them: one batch through knz_hip_encode_blocks / _decode_blocks with
NONE entropy; the stage's figure is the HIP-event time of its kernels (knz_hip_set_profiling), warm, the median of --steps runs, with
the kernels listed one by one. Beside it the reference's UTF / NONE through ref_time_roundtrip at -j N on the same bytes (skipped
where the build is absent). Then the two chains the stage was moved for, end to end through kz.Compressor / kz.Decompressor on the
same bytes: TEXT+UTF+BWT+RANK+ZRLT / ANS0 (TEXT on the host, one block per device call) and UTF+BWT+RANK+ZRLT / ANS0 (no host stage):
median, lowest and highest of --steps runs. --e2e-only leaves the stage part out, so that the same file runs on a tree whose device
has no UTF stage and the two trees can be compared.
    python tools/gpu_utf_time.py [--blocks 8] [--steps 5] [--local-limit 0] [--e2e-only]
"""
import argparse
import ctypes as C
import importlib
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import knzlib  # noqa: E402
import vectors  # noqa: E402

BS = 8 << 20
E2E = [("TEXT+UTF+BWT+RANK+ZRLT", "ANS0"), ("UTF+BWT+RANK+ZRLT", "ANS0")]


def utf8_blocks(blocks):
    unit = vectors.make(("utf8", 9 << 20, 7))[:4 << 20]
    out = bytearray()
    for b in range(blocks):
        off = (b * 65521) % len(unit)
        out += (unit[off:] + unit + unit)[:BS]
    return bytes(out)


def stage(ctx, data, steps):
    n = len(data)
    p = ctx.params("UTF", "NONE", BS)
    cap = ctx.encode_bound(p, n)
    d_in, d_out, d_dec = ctx.malloc(n + 64), ctx.malloc(cap), ctx.malloc(n + BS + 64)
    ctx.h2d(d_in, data)
    te, td, kf, ki = [], [], [], []
    names = {}
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
                kd = ctx.kernel_times()
                kf.append(sum(ms for name, ms, _ in kt if name.startswith("k_utf")))
                ki.append(sum(ms for name, ms, _ in kd if name.startswith("k_utf")))
                for name, ms, _ in list(kt) + list(kd):
                    if name.startswith("k_utf"):
                        names.setdefault(name, []).append(ms)
            else:
                te.append(1e3 * (t1 - t0))
                td.append(1e3 * (t3 - t2))
    ctx.set_profiling(False)
    back = ctx.d2h(d_dec, min(n, 1 << 20))
    assert back == data[:len(back)]
    for ptr in (d_in, d_out, d_dec):
        ctx.free(ptr)
    m = statistics.median
    return {"chain": "UTF", "entropy": "NONE", "bytes": n, "compressed": (bits + 7) // 8, "encode_ms": round(m(te), 2), "decode_ms": round(m(td), 2),
            "utf_forward_kernels_ms": round(m(kf), 3), "utf_inverse_kernels_ms": round(m(ki), 3),
            "kernels_ms": {k: round(m(v), 3) for k, v in sorted(names.items())}}


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


def end_to_end(kz, chain, entropy, data, steps, jobs):
    te, td = [], []
    size = 0
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "s.knz")
        for i in range(steps + 1):
            t0 = time.perf_counter()
            c = kz.Compressor(path, chain, entropy, BS, jobs)
            for off in range(0, len(data), BS):
                c.compress(data[off:off + BS])
            c.close()
            t1 = time.perf_counter()
            size = os.path.getsize(path)
            d = kz.Decompressor(path, buffer_size=BS, jobs=jobs)
            got = 0
            t2 = time.perf_counter()
            while True:
                chunk = d.decompress(BS)
                if got == 0:
                    assert chunk == data[:len(chunk)]
                got += len(chunk)
                if len(chunk) < BS:
                    break
            d.close()
            t3 = time.perf_counter()
            assert got == len(data)
            if i >= 1:
                te.append(1e3 * (t1 - t0))
                td.append(1e3 * (t3 - t2))
    m = statistics.median
    return {"chain": chain, "entropy": entropy, "bytes": len(data), "knz_bytes": size, "jobs": jobs,
            "e2e_encode_ms": [round(m(te), 1), round(min(te), 1), round(max(te), 1)],
            "e2e_decode_ms": [round(m(td), 1), round(min(td), 1), round(max(td), 1)]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=8)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--local-limit", type=int, default=0)
    ap.add_argument("--e2e-only", action="store_true")
    a = ap.parse_args()
    knzlib.load_pkg()
    hipapi = importlib.import_module("kanzi_amd.hipapi")
    corpus = importlib.import_module("kanzi_amd.corpus")
    kz = importlib.import_module("kanzi_amd.kanzi")
    inputs = [("utf8 vector", utf8_blocks(a.blocks))]
    if a.local_limit > 0:
        data, _, desc = corpus.local(a.local_limit)
        inputs.append(("local: " + desc, data))
    if not a.e2e_only:
        ctx = hipapi.Context(0)
        for kind, data in inputs:
            res = dict(stage(ctx, data, a.steps), input=kind)
            res.update(reference(data, "UTF", "NONE", a.blocks) or {})
            print(json.dumps(res), flush=True)
        ctx.close()
    for kind, data in inputs:
        for chain, entropy in E2E:
            print(json.dumps(dict(end_to_end(kz, chain, entropy, data, a.steps, a.blocks), input=kind)), flush=True)


if __name__ == "__main__":
    main()
