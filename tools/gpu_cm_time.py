"""Times the CM coder (entropy id 6) on one MI355X, encode and decode separately, on the bytes it is meant for: the output of
BWT+RANK+ZRLT (made here with the device's per-stage transforms from 4 MiB blocks of the mixed stand-in corpus, and repeated where a
batch needs more than was made), as 26 blocks of 1 MiB and as 256 blocks of 256 KiB, with FPAQ on the same bytes for scale. Both
coders are one chain per block on the decode side, and CM's encoder is one too: the time of a batch is the time of its slowest block
until the blocks outnumber the compute units (CM holds 150 KB of LDS per block), so the cost per byte is the time over ONE block's
bytes. The figures are the sums of the coders' kernels' HIP-event times (knz_hip_set_profiling), warm, the median of --steps runs, and
the wall clock of the whole knz_hip_encode_blocks / _decode_blocks call.
    timeout 900 python tools/gpu_cm_time.py [--steps 3]
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import knzlib  # noqa: E402

KERNELS = {"CM": ("k_cm_encode", "k_cm_decode"), "FPAQ": ("k_fpaq_encode", "k_fpaq_decode")}
SHAPES = [(26, 1 << 20), (256, 256 << 10)]


def device(ctx, entropy, data, bs, steps):
    p = ctx.params("NONE", entropy, bs)
    cap = ctx.encode_bound(p, len(data))
    d_in, d_out, d_dec = ctx.malloc(len(data) + 64), ctx.malloc(cap), ctx.malloc(len(data) + bs + 64)
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
        ob, _, _ = ctx.decode_blocks(p, d_out, bits, 0, d_dec, len(data) + bs)
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


def transformed(ctx, want):
    """At least `want` bytes of BWT+RANK+ZRLT output, block after block of the corpus; repeated from the start where 64 MiB of input
    have not made enough."""
    out, src = bytearray(), knzlib.corpus().mixed(64 << 20, 2)
    for off in range(0, len(src), 4 << 20):
        blk = src[off:off + (4 << 20)]
        for t in ("BWT", "RANK", "ZRLT"):
            ok, blk = ctx.transform_forward(t, blk, len(blk) + (len(blk) >> 4) + 1024)
            assert ok, t
        out += blk
        if len(out) >= want:
            break
    made = len(out)
    while len(out) < want:
        out += out[:made]
    return bytes(out[:want]), made


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=3)
    a = ap.parse_args()
    import importlib
    knzlib.load_pkg()
    hipapi = importlib.import_module("kanzi_amd.hipapi")
    ctx = hipapi.Context(0)
    data, made = transformed(ctx, max(n * bs for n, bs in SHAPES))
    print("input: BWT+RANK+ZRLT output of the mixed corpus, %.1f MB made, repeated to %.1f MB" % (made / 1e6, len(data) / 1e6))
    for n, bs in SHAPES:
        part = data[:n * bs]
        mb = len(part) / 1e6
        print("%d blocks of %d KiB (%.1f MB)" % (n, bs >> 10, mb))
        for entropy in ("CM", "FPAQ"):
            ek, dk, ew, dw, bits = device(ctx, entropy, part, bs, a.steps)
            print("  %-4s encode kernels %9.3f ms (%7.1f MB/s, %6.1f ns per byte of a block), call %9.3f ms | decode kernels %9.3f ms (%7.1f MB/s, %6.1f ns per byte of a block), call %9.3f ms | %d bytes out"
                  % (entropy, ek, mb / ek * 1e3, ek * 1e6 / bs, ew, dk, mb / dk * 1e3, dk * 1e6 / bs, dw, (bits + 7) // 8))
    ctx.close()


if __name__ == "__main__":
    main()
