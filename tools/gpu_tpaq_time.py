"""Times the TPAQ and TPAQX coders (entropy ids 7 and 9) on one MI355X, encode and decode separately, on one block of 64 KiB and one
of 1 MiB of the mixed stand-in corpus (chain NONE). Both directions are one wave per block, so the time of a batch is the time of its
slowest block until the blocks outnumber what the device holds at once: the cost is given per byte of ONE block. The figures are the
sums of the coders' kernels' HIP-event times (knz_hip_set_profiling; the zeroing of the tables is not in them), warm, the median of
--steps runs, and the wall clock of the whole knz_hip_encode_blocks / _decode_blocks call (tables zeroed, stream assembled). Beside
them: the reference's command line on the same bytes with -j 1 (one host core; process start and file I/O included), where
oracle/_ref/kanzi has been built. Only the per-bit kernel shape exists (csrc/tpaq.hip), so there is one column per direction.
    timeout 900 python tools/gpu_tpaq_time.py [--steps 3]
"""
import argparse
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import knzlib  # noqa: E402

KERNELS = ("k_tpaq_encode", "k_tpaq_decode")
SIZES = [64 << 10, 1 << 20]


def device(ctx, entropy, data, bs, steps):
    p = ctx.params("NONE", entropy, bs)
    cap = ctx.encode_bound(p, len(data)) + 32 * len(data)
    d_in, d_out, d_dec = ctx.malloc(len(data) + 64), ctx.malloc(cap), ctx.malloc(len(data) + bs + 64)
    ctx.h2d(d_in, data)
    enc_k, dec_k, enc_w, dec_w, bits = [], [], [], [], 0
    for i in range(steps + 1):
        ctx.set_profiling(True)
        t0 = time.perf_counter()
        bits = ctx.encode_blocks(p, d_in, len(data), d_out, cap)
        t1 = time.perf_counter()
        ek = sum(ms for name, ms, _ in ctx.kernel_times() if name in KERNELS)
        ctx.set_profiling(True)
        t2 = time.perf_counter()
        ob, _, _ = ctx.decode_blocks(p, d_out, bits, 0, d_dec, len(data) + bs)
        t3 = time.perf_counter()
        dk = sum(ms for name, ms, _ in ctx.kernel_times() if name in KERNELS)
        ctx.set_profiling(False)
        assert ob == len(data)
        if i:
            enc_k.append(ek); dec_k.append(dk); enc_w.append(1e3 * (t1 - t0)); dec_w.append(1e3 * (t3 - t2))
    assert ctx.d2h(d_dec, len(data)) == data
    for ptr in (d_in, d_out, d_dec):
        ctx.free(ptr)
    m = statistics.median
    return m(enc_k), m(dec_k), m(enc_w), m(dec_w), bits


def reference(entropy, data, bs):
    """(encode ms, decode ms) of the reference's command line at -j 1, or None where it has not been built."""
    if not os.path.exists(knzlib.REF_BIN):
        return None
    with tempfile.TemporaryDirectory() as tmp:
        src, dst, back = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.knz"), os.path.join(tmp, "back.bin")
        with open(src, "wb") as f:
            f.write(data)
        t0 = time.perf_counter()
        subprocess.run([knzlib.REF_BIN, "-c", "-i", src, "-o", dst, "-f", "-t", "NONE", "-e", entropy, "-b", str(bs), "-j", "1"], check=True,
                       stdin=subprocess.DEVNULL, stdout=subprocess.DEVNULL)
        t1 = time.perf_counter()
        subprocess.run([knzlib.REF_BIN, "-d", "-i", dst, "-o", back, "-f", "-j", "1"], check=True, stdin=subprocess.DEVNULL, stdout=subprocess.DEVNULL)
        t2 = time.perf_counter()
        return 1e3 * (t1 - t0), 1e3 * (t2 - t1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=3)
    a = ap.parse_args()
    import importlib
    knzlib.load_pkg()
    hipapi = importlib.import_module("kanzi_amd.hipapi")
    ctx = hipapi.Context(0)
    src = knzlib.corpus().mixed(max(SIZES), 2)
    for bs in SIZES:
        data = src[len(src) - bs:]          # (the corpus starts with a stretch that barely needs coding: the tail is ordinary)
        print("one block of %d KiB" % (bs >> 10))
        for entropy in ("TPAQ", "TPAQX"):
            ek, dk, ew, dw, bits = device(ctx, entropy, data, bs, a.steps)
            line = ("  %-5s encode kernel %9.3f ms (%6.3f us per byte), call %9.3f ms | decode kernel %9.3f ms (%6.3f us per byte), call %9.3f ms | %d bytes out"
                    % (entropy, ek, ek * 1e3 / bs, ew, dk, dk * 1e3 / bs, dw, (bits + 7) // 8))
            r = reference(entropy, data, bs)
            if r:
                line += " | reference, one host core: encode %9.3f ms (%6.3f us per byte), decode %9.3f ms (%6.3f us per byte)" % (r[0], r[0] * 1e3 / bs, r[1], r[1] * 1e3 / bs)
            print(line, flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
