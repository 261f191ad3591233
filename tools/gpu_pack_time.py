"""Times PACK forward and inverse next to LZX on 64 blocks of 4 MiB of text, WAV and BMP (one batch through knz_hip_encode_blocks /
_decode_blocks, NONE entropy). For per-kernel times run it under rocprofv3 in a run of its own:
    rocprofv3 --kernel-trace --stats -d OUT -o run -- python tools/gpu_pack_time.py
    python tools/gpu_pack_time.py [--blocks 64] [--steps 5]
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import knzlib  # noqa: E402
import pack_cases  # noqa: E402

BS = 4 << 20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=64)
    ap.add_argument("--steps", type=int, default=5)
    a = ap.parse_args()
    knzlib.load_pkg()
    import importlib
    hipapi = importlib.import_module("kanzi_amd.hipapi")
    ctx = hipapi.Context(0)
    for kind in ("text", "wav", "bmp"):
        block = pack_cases.make([kind, BS, 7])
        data = block * a.blocks
        n = len(data)
        d_in = ctx.malloc(n + 64)
        ctx.h2d(d_in, data)
        for chain in ("PACK", "LZX"):
            p = ctx.params(chain, "NONE", BS)
            cap = ctx.encode_bound(p, n)
            d_out, d_dec = ctx.malloc(cap), ctx.malloc(n + BS + 64)
            bits = ctx.encode_blocks(p, d_in, n, d_out, cap)
            ctx.decode_blocks(p, d_out, bits, 0, d_dec, n + BS)
            te = td = 0.0
            for _ in range(a.steps):
                t0 = time.perf_counter()
                bits = ctx.encode_blocks(p, d_in, n, d_out, cap)
                t1 = time.perf_counter()
                ob, _, _ = ctx.decode_blocks(p, d_out, bits, 0, d_dec, n + BS)
                t2 = time.perf_counter()
                te += t1 - t0
                td += t2 - t1
            assert ob == n
            print("%-4s %-4s ratio %.3f  encode %7.2f ms  decode %7.2f ms  (%d x 4 MiB, NONE entropy, includes framing)" %
                  (kind, chain, (bits / 8) / n, 1e3 * te / a.steps, 1e3 * td / a.steps, a.blocks), flush=True)
            ctx.free(d_out)
            ctx.free(d_dec)
        ctx.free(d_in)
    ctx.close()


if __name__ == "__main__":
    main()
