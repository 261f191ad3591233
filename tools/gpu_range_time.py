"""Times NONE / RANGE on N blocks of 4 MiB of config 2's input (the mixed stand-in corpus), encode and decode separately, on one
MI355X, beside
  (a) device ANS0 on the same batch,
  (b) the reference (oracle/_ref/kanzi -t NONE -e RANGE -b 4m) at -j = number of blocks on this box's cores: wall clock of the
      whole command, best of 3, files in a RAM-backed temporary directory where there is one (skipped where the build is absent).
The device figures are the sums of the coders' kernels' HIP-event times (knz_hip_set_profiling), warm, the median of --steps runs,
and the wall clock of the whole knz_hip_encode_blocks / _decode_blocks call. The decoder is one chain per block: its time does not
depend on the number of blocks until they outnumber the SIMDs, so its cost per byte is its time over ONE block's bytes.
    python tools/gpu_range_time.py [--blocks 16] [--steps 5]
For per-kernel times: rocprofv3 --kernel-trace --stats -d OUT -o run -- python tools/gpu_range_time.py --steps 2
"""
import argparse
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import knzlib  # noqa: E402

BS = 4 << 20
KERNELS = {"RANGE": ("k_range_stats", "k_range_encode", "k_range_decode"), "ANS0": ("k_ans0_stats", "k_ans0_encode", "k_ans_scan", "k_ans0_decode")}


def device(ctx, entropy, data, steps):
    p = ctx.params("NONE", entropy, BS)
    cap = ctx.encode_bound(p, len(data))
    d_in, d_out, d_dec = ctx.malloc(len(data) + 64), ctx.malloc(cap), ctx.malloc(len(data) + BS + 64)
    ctx.h2d(d_in, data)
    enc_k, dec_k, enc_w, dec_w, bits = [], [], [], [], 0
    for i in range(steps + 1):
        ctx.set_profiling(True)
        t0 = time.perf_counter()
        bits = ctx.encode_blocks(p, d_in, len(data), d_out, cap)
        t1 = time.perf_counter()
        ek = sum(ms for name, ms, _ in ctx.kernel_times() if name in KERNELS[entropy])
        ctx.set_profiling(True)
        t2 = time.perf_counter()
        ob, _, _ = ctx.decode_blocks(p, d_out, bits, 0, d_dec, len(data) + BS)
        t3 = time.perf_counter()
        dk = sum(ms for name, ms, _ in ctx.kernel_times() if name in KERNELS[entropy])
        ctx.set_profiling(False)
        assert ob == len(data)
        if i:
            enc_k.append(ek); dec_k.append(dk); enc_w.append(1e3 * (t1 - t0)); dec_w.append(1e3 * (t3 - t2))
    assert ctx.d2h(d_dec, len(data)) == data
    for ptr in (d_in, d_out, d_dec):
        ctx.free(ptr)
    m = statistics.median
    return m(enc_k), m(dec_k), m(enc_w), m(dec_w), bits


def reference(data, jobs):
    if not os.path.exists(knzlib.REF_BIN):
        return None
    tmp = tempfile.mkdtemp(dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
    try:
        src, knz, back = os.path.join(tmp, "in"), os.path.join(tmp, "out.knz"), os.path.join(tmp, "back")
        open(src, "wb").write(data)
        enc, dec = [], []
        for _ in range(3):
            t0 = time.perf_counter()
            subprocess.run([knzlib.REF_BIN, "-c", "-i", src, "-o", knz, "-f", "-t", "NONE", "-e", "RANGE", "-b", str(BS), "-j", str(jobs)], check=True, stdout=subprocess.DEVNULL)
            t1 = time.perf_counter()
            subprocess.run([knzlib.REF_BIN, "-d", "-i", knz, "-o", back, "-f", "-j", str(jobs)], check=True, stdout=subprocess.DEVNULL)
            t2 = time.perf_counter()
            enc.append(1e3 * (t1 - t0)); dec.append(1e3 * (t2 - t1))
        return min(enc), min(dec)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=16)
    ap.add_argument("--steps", type=int, default=5)
    a = ap.parse_args()
    import importlib
    knzlib.load_pkg()
    hipapi = importlib.import_module("kanzi_amd.hipapi")
    data = knzlib.corpus().mixed(a.blocks * BS, 2)
    ctx = hipapi.Context(0)
    mb = len(data) / 1e6
    print("input: %d blocks of 4 MiB (%.1f MB), mixed corpus" % (a.blocks, mb))
    for entropy in ("RANGE", "ANS0"):
        ek, dk, ew, dw, bits = device(ctx, entropy, data, a.steps)
        print("%-5s device: encode kernels %8.3f ms (%8.1f MB/s), call %8.3f ms | decode kernels %9.3f ms (%8.1f MB/s), call %9.3f ms | %d bytes out"
              % (entropy, ek, mb / ek * 1e3, ew, dk, mb / dk * 1e3, dw, (bits + 7) // 8))
        if entropy == "RANGE":
            print("RANGE decode, one chain per block: %.1f ns per byte of a block" % (dk * 1e6 / BS))
    ref = reference(data, a.blocks)
    if ref is None:
        print("reference: oracle/_ref/kanzi not built, skipped")
    else:
        print("RANGE reference -j %d (whole command, best of 3): compress %.1f ms (%.1f MB/s), decompress %.1f ms (%.1f MB/s)"
              % (a.blocks, ref[0], mb / ref[0] * 1e3, ref[1], mb / ref[1] * 1e3))
    ctx.close()


if __name__ == "__main__":
    main()
