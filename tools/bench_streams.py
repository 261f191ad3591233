"""Many small independent inputs: one knz_hip_encode_blocks / knz_hip_decode_blocks call per input (the only way before the batch
entry points existed) against one knz_hip_encode_streams / knz_hip_decode_streams call for all of them. 512 items of 64 KiB and 4,096
items of 4 KiB of corpus.mixed through BWT+RANK+ZRLT / ANS0 and LZX / HUFFMAN, block size 64 KiB and 4 KiB (one block per item).
Everything stays on the device: the inputs are uploaded once, the times are synchronised wall times of the calls alone (every call of
either kind ends with a host synchronisation), one warm-up run, then the median of --repeats runs. The launch counts come from
knz_hip_get_kernel_times with per-kernel timing on, in a run of their own.

    python tools/bench_streams.py [--out FILE] [--repeats N]
"""
import argparse
import importlib
import importlib.util
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "kanzi-cpp_amd")


def load():
    if "kanzi_amd" not in sys.modules:
        spec = importlib.util.spec_from_file_location("kanzi_amd", os.path.join(PKG, "__init__.py"), submodule_search_locations=[PKG])
        mod = importlib.util.module_from_spec(spec)
        sys.modules["kanzi_amd"] = mod
        spec.loader.exec_module(mod)
    return importlib.import_module("kanzi_amd.hipapi"), importlib.import_module("kanzi_amd.corpus")


def median_ms(fn, repeats):
    fn()                                       # warm-up: workspaces grown, code objects loaded
    times = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        times.append(1e3 * (time.perf_counter() - t0))
    return statistics.median(times)


def launches(ctx, fn):
    ctx.set_profiling(True)
    fn()
    n = sum(k[2] for k in ctx.kernel_times())
    ctx.set_profiling(False)
    return n


def shape(ctx, hipapi, data, n_items, size, transform, entropy, repeats, out):
    p = ctx.params(transform, entropy, size)
    step = (size + 15) & ~15
    d_in = ctx.malloc(n_items * step + 64)
    ctx.h2d(d_in, data[:n_items * step])
    items = (hipapi.Item * n_items)()
    for i in range(n_items):
        items[i].in_off, items[i].in_len = i * step, size
    cap1 = (ctx.encode_bound(p, size) + 64 + 15) & ~15
    cap = max(ctx.encode_streams_bound(p, items), n_items * cap1)
    d_enc, d_dec = ctx.malloc(cap), ctx.malloc(n_items * step + 64)
    bits = [0] * n_items

    def enc_loop(count=n_items):
        for i in range(count):
            bits[i] = ctx.encode_blocks(p, d_in + i * step, size, d_enc + i * cap1, cap1)

    def dec_loop(count=n_items):
        for i in range(count):
            ctx.decode_blocks(p, d_enc + i * cap1, bits[i], 0, d_dec + i * step, step)

    t_enc_loop = median_ms(enc_loop, repeats)
    t_dec_loop = median_ms(dec_loop, repeats)
    n_enc_loop, n_dec_loop = launches(ctx, lambda: enc_loop(1)), launches(ctx, lambda: dec_loop(1))
    ok_loop = ctx.d2h(d_dec, n_items * step) == data[:n_items * step]

    def enc_batch():
        ctx.encode_streams(p, d_in, items, d_enc, cap)

    t_enc_batch = median_ms(enc_batch, repeats)
    n_enc_batch = launches(ctx, enc_batch)
    ditems = (hipapi.Item * n_items)()
    for i in range(n_items):
        ditems[i].in_off, ditems[i].in_len, ditems[i].start_bit = items[i].out_off, items[i].out_len, 0
        ditems[i].out_off, ditems[i].out_cap = i * step, step
    ctx.h2d(d_dec, bytes(n_items * step))

    def dec_batch():
        ctx.decode_streams(p, d_enc, ditems, d_dec, n_items * step + 64)

    t_dec_batch = median_ms(dec_batch, repeats)
    n_dec_batch = launches(ctx, dec_batch)
    ok_batch = ctx.d2h(d_dec, n_items * step) == data[:n_items * step] and all(ditems[i].error == 0 for i in range(n_items))
    for ptr in (d_in, d_enc, d_dec):
        ctx.free(ptr)
    mb = n_items * size / 1e6
    out.write("%-16s %-8s %5d x %6d B | encode: loop %9.2f ms, batch %8.2f ms, x%6.1f (%7.1f MB/s) | decode: loop %9.2f ms, batch %8.2f ms, x%6.1f (%7.1f MB/s)\n"
              % (transform, entropy, n_items, size, t_enc_loop, t_enc_batch, t_enc_loop / t_enc_batch, mb / t_enc_batch * 1e3,
                 t_dec_loop, t_dec_batch, t_dec_loop / t_dec_batch, mb / t_dec_batch * 1e3))
    out.write("%-16s %-8s   launches per call | encode: single %d, batch of %d: %d | decode: single %d, batch: %d | round trips: loop %s, batch %s\n"
              % ("", "", n_enc_loop, n_items, n_enc_batch, n_dec_loop, n_dec_batch, "ok" if ok_loop else "WRONG", "ok" if ok_batch else "WRONG"))
    out.flush()
    return ok_loop and ok_batch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    hipapi, corpus = load()
    ctx = hipapi.Context(0)
    data = corpus.mixed(512 * 65536, 2)
    out = open(a.out, "w") if a.out else sys.stdout
    out.write("one call per item (knz_hip_encode_blocks / knz_hip_decode_blocks) against one call for all items (knz_hip_encode_streams / "
              "knz_hip_decode_streams); median of %d runs after a warm-up, synchronised wall time\n" % a.repeats)
    ok = True
    for transform, entropy in (("BWT+RANK+ZRLT", "ANS0"), ("LZX", "HUFFMAN")):
        for n_items, size in ((512, 65536), (4096, 4096)):
            ok &= shape(ctx, hipapi, data, n_items, size, transform, entropy, a.repeats, out)
    ctx.close()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
