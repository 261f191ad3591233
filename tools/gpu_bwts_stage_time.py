"""BWTS against BWT on the device, and against the reference on the host (developer tool, numbers for DESIGN.md).

For each chain (BWT+MTFT+ZRLT and BWTS+MTFT+ZRLT, ANS0, 8 MiB blocks) on corpus.mixed(211957760, 2):
  * device-resident MB/s of encode, decode and the round trip (input and output stay in HBM; best of --reps),
  * the transform's forward and inverse stage times from the per-kernel timers (one profiled encode + decode; timing turns the
    split of the BWT stages into parts off, so these are the one-stream times),
  * the reference on the host cores (oracle/_ref, -j min(cores, 64, blocks)), when that build is present.
    python tools/gpu_bwts_stage_time.py [--size N] [--reps K] [--no-ref]
Prints one JSON line per chain.
"""
import argparse
import ctypes as C
import hashlib
import importlib
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
import knzlib  # noqa: E402


def stage_ms(times, prefixes):
    return round(sum(ms for name, ms, _ in times if name.startswith(prefixes)), 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=211957760)
    ap.add_argument("--block", type=int, default=8 << 20)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-ref", action="store_true")
    a = ap.parse_args()
    knzlib.load_pkg()
    hipapi = importlib.import_module("kanzi_amd.hipapi")
    corpus = importlib.import_module("kanzi_amd.corpus")
    data = corpus.mixed(a.size, 2)
    n, bs = len(data), a.block
    ctx = hipapi.Context(0)
    d_in = ctx.malloc(n + 64)
    ctx.h2d(d_in, data)
    for chain, fwd_pre, inv_pre in (("BWT+MTFT+ZRLT", ("k_bwt_f",), ("k_bwt_i",)), ("BWTS+MTFT+ZRLT", ("k_bwt_f", "k_bwts_f"), ("k_bwts_i",))):
        p = ctx.params(chain, "ANS0", bs)
        cap = ctx.encode_bound(p, n)
        d_out, d_dec = ctx.malloc(cap), ctx.malloc(n + bs + 64)
        bits = ctx.encode_blocks(p, d_in, n, d_out, cap)              # warm-up (workspaces)
        ctx.decode_blocks(p, d_out, bits, 0, d_dec, n + bs)
        te = td = None
        for _ in range(a.reps):
            t0 = time.perf_counter()
            bits = ctx.encode_blocks(p, d_in, n, d_out, cap)
            ctx.sync()
            t1 = time.perf_counter()
            ob, _, _ = ctx.decode_blocks(p, d_out, bits, 0, d_dec, n + bs)
            ctx.sync()
            t2 = time.perf_counter()
            te = min(te or 1e9, t1 - t0)
            td = min(td or 1e9, t2 - t1)
        enc = ctx.d2h(d_out, (bits + 7) // 8)
        ok = ob == n and ctx.d2h(d_dec, n) == data
        ctx.set_profiling(True)
        ctx.encode_blocks(p, d_in, n, d_out, cap)
        kf = ctx.kernel_times()
        ctx.set_profiling(False)
        ctx.set_profiling(True)
        ctx.decode_blocks(p, d_out, bits, 0, d_dec, n + bs)
        ki = ctx.kernel_times()
        ctx.set_profiling(False)
        res = {"chain": chain, "entropy": "ANS0", "block": bs, "bytes": n, "roundtrip_ok": ok, "compressed": len(enc),
               "knz_md5": hashlib.md5(enc).hexdigest(),
               "enc_ms": round(te * 1e3, 2), "dec_ms": round(td * 1e3, 2), "enc_MBps": round(n / te / 1e6, 1), "dec_MBps": round(n / td / 1e6, 1),
               "roundtrip_MBps": round(n / (te + td) / 1e6, 1),
               "fwd_stage_ms": stage_ms(kf, fwd_pre), "inv_stage_ms": stage_ms(ki, inv_pre)}
        ctx.free(d_out); ctx.free(d_dec)
        so = None if a.no_ref else knzlib.ensure_ref()
        if so is not None:
            import numpy as np
            L = C.CDLL(so)
            u8p = C.POINTER(C.c_uint8)
            L.ref_time_roundtrip.restype = C.c_int
            L.ref_time_roundtrip.argtypes = [u8p, C.c_size_t, C.c_char_p, C.c_char_p, C.c_int, C.c_int, u8p, C.c_size_t,
                                             C.POINTER(C.c_size_t), u8p, C.POINTER(C.c_double), C.POINTER(C.c_double)]
            src = np.frombuffer(data, dtype=np.uint8)
            comp = np.empty(n + n // 2 + (1 << 20), dtype=np.uint8)
            back = np.empty(n, dtype=np.uint8)
            jobs = max(1, min(os.cpu_count() or 1, 64, (n + bs - 1) // bs))
            clen, rte, rtd = C.c_size_t(0), C.c_double(0), C.c_double(0)
            rc = L.ref_time_roundtrip(src.ctypes.data_as(u8p), n, chain.encode(), b"ANS0", bs, jobs, comp.ctypes.data_as(u8p), comp.size,
                                      C.byref(clen), back.ctypes.data_as(u8p), C.byref(rte), C.byref(rtd))
            if rc == 0:
                res.update({"ref_jobs": jobs, "ref_enc_s": round(rte.value, 3), "ref_dec_s": round(rtd.value, 3),
                            "ref_roundtrip_MBps": round(n / (rte.value + rtd.value) / 1e6, 1)})
        print(json.dumps(res), flush=True)
    ctx.free(d_in)
    ctx.close()


if __name__ == "__main__":
    main()
