"""Tensors that live on the GPU: (a) the batched copy kernel of knz_hip_copy_many beside dst.copy_(src) of one contiguous tensor of the
same bytes, (b) kanzi.TensorCodec beside the route a caller had before it (t.cpu() -> compress_many -> decompress_many -> .cuda()).

(a) 4,096 copies of 4 KiB and 64 copies of 16 MiB, each with src = dst (mod 16) and with the source one byte off. Times are device events
    on the codec's stream around `inner` calls in a row (the table upload of every call included), and the kernel alone from
    knz_hip_get_kernel_times in a run of its own. GB/s counts the bytes copied once (the memory moves twice as many).
(b) the same two shapes through LZ / HUFFMAN and BWT+RANK+ZRLT / ANS0 (blocks of 64 KiB for the small tensors, of 4 MiB for the large
    ones): synchronised wall time of compress + decompress, results on the device at the end of both routes.
Every figure is the median of --repeats runs after a warm-up run, with the fastest and the slowest beside it.

    python tools/bench_tensors.py [--out FILE] [--repeats N] [--inner N] [--only copy|codec] [--shapes small|large|both] [--chains lz|bwt|both]
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
SHAPES = {"small": (4096, 4096, 65536), "large": (64, 16 << 20, 4 << 20)}         # copies / tensors, bytes each, block size of (b)


def load():
    if "kanzi_amd" not in sys.modules:
        spec = importlib.util.spec_from_file_location("kanzi_amd", os.path.join(PKG, "__init__.py"), submodule_search_locations=[PKG])
        mod = importlib.util.module_from_spec(spec)
        sys.modules["kanzi_amd"] = mod
        spec.loader.exec_module(mod)
    return [importlib.import_module("kanzi_amd." + m) for m in ("hipapi", "corpus", "kanzi")]


def spread(times):
    return "%9.3f ms (%.3f - %.3f)" % (statistics.median(times), min(times), max(times))


def event_ms(torch, stream, fn, inner, repeats):
    """ms per call: device events on `stream` around `inner` calls, one warm-up, `repeats` measurements."""
    times = []
    for r in range(repeats + 1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        for _ in range(inner):
            fn()
        b.record(stream)
        b.synchronize()
        if r:
            times.append(a.elapsed_time(b) / inner)
    return times


def bench_copy(torch, hipapi, codec, n, size, inner, repeats, out):
    total = n * size
    src = torch.randint(0, 256, (total + 16,), dtype=torch.uint8, device=codec.device)
    dst = torch.empty(total + 16, dtype=torch.uint8, device=codec.device)
    assert src.data_ptr() % 16 == 0 and dst.data_ptr() % 16 == 0
    flat = event_ms(torch, codec.stream, lambda: dst[:total].copy_(src[:total]), inner, repeats)
    gbs = lambda ms: total / 1e6 / ms
    out.write("%5d x %8d B  dst.copy_(src), one tensor          : %s  %8.1f GB/s\n" % (n, size, spread(flat), gbs(statistics.median(flat))))
    for off, what in ((0, "src = dst (mod 16)"), (1, "src one byte off  ")):
        table = (hipapi.Copy * n)()
        for i in range(n):
            table[i].src, table[i].dst, table[i].len = src.data_ptr() + off + i * size, dst.data_ptr() + i * size, size
        dst.zero_()
        call = event_ms(torch, codec.stream, lambda: codec.ctx.copy_many(table), inner, repeats)
        ok = torch.equal(dst[:total], src[off:off + total])
        kern = []
        for r in range(repeats + 1):
            codec.ctx.set_profiling(True)
            codec.ctx.copy_many(table)
            ms = [t for name, t, _ in codec.ctx.kernel_times() if name == "k_copy_many"]
            codec.ctx.set_profiling(False)
            if r:
                kern.append(ms[0])
        out.write("%5d x %8d B  copy_many, %s, call  : %s  %8.1f GB/s  %s\n" % (n, size, what, spread(call), gbs(statistics.median(call)), "ok" if ok else "WRONG"))
        out.write("%5d x %8d B  copy_many, %s, kernel: %s  %8.1f GB/s\n" % (n, size, what, spread(kern), gbs(statistics.median(kern))))
        out.flush()
        if not ok:
            return False
    return True


def bench_codec(torch, kz, corpus, device, n, size, bs, transform, entropy, repeats, out):
    base = torch.frombuffer(bytearray(corpus.mixed(min(n * size, 16 << 20), 2)), dtype=torch.uint8).to(device)
    codec = kz.TensorCodec(device)
    if base.numel() >= n * size:
        tensors = [base[i * size:(i + 1) * size] for i in range(n)]
    else:                                      # large tensors: the same 16 MiB turned by a different amount each
        tensors = [torch.roll(base, 4099 * i) for i in range(n)]

    def device_route():
        blob, offsets = codec.compress(tensors, transform, entropy, bs)
        back = codec.decompress(blob, offsets)
        torch.cuda.synchronize()
        return blob.numel(), back

    def host_route():
        streams = kz.compress_many([t.cpu().numpy().tobytes() for t in tensors], transform, entropy, bs)
        back = [torch.frombuffer(bytearray(b), dtype=torch.uint8).to(device) for b in kz.decompress_many(streams)]
        torch.cuda.synchronize()
        return sum(len(s) for s in streams), back

    res = {}
    for name, fn in (("TensorCodec", device_route), ("through the host", host_route)):
        times = []
        for r in range(repeats + 1):
            t0 = time.perf_counter()
            nbytes, back = fn()
            if r:
                times.append(1e3 * (time.perf_counter() - t0))
        ok = len(back) == n and all(torch.equal(b, t) for b, t in zip(back, tensors))
        del back
        codec.close()                          # the workspaces of one route are gone before the other takes its own
        torch.cuda.empty_cache()
        res[name] = (statistics.median(times), nbytes, ok)
        out.write("%5d x %8d B  %-14s %-8s %-17s: %s  %8.1f MB/s  %d bytes  %s\n"
                  % (n, size, transform, entropy, name, spread(times), n * size / 1e3 / statistics.median(times), nbytes, "ok" if ok else "WRONG"))
        out.flush()
    out.write("%5d x %8d B  %-14s %-8s TensorCodec is x%.2f the host route; same bytes: %s\n"
              % (n, size, transform, entropy, res["through the host"][0] / res["TensorCodec"][0], res["TensorCodec"][1] == res["through the host"][1]))
    return all(v[2] for v in res.values()) and res["TensorCodec"][1] == res["through the host"][1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--only", choices=("copy", "codec"), default="")
    ap.add_argument("--shapes", choices=("small", "large", "both"), default="both")
    ap.add_argument("--chains", choices=("lz", "bwt", "both"), default="both")
    a = ap.parse_args()
    import torch
    hipapi, corpus, kz = load()
    out = open(a.out, "w") if a.out else sys.stdout
    shapes = [SHAPES[k] for k in (("small", "large") if a.shapes == "both" else (a.shapes,))]
    ok = True
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream), kz.TensorCodec() as codec:
        out.write("median of %d runs after a warm-up (fastest - slowest); copies: device events around %d calls in a row\n" % (a.repeats, a.inner))
        if a.only != "codec":
            for n, size, _ in shapes:
                ok &= bench_copy(torch, hipapi, codec, n, size, a.inner, a.repeats, out)
        if a.only != "copy":
            for n, size, bs in shapes:
                for key, transform, entropy in (("lz", "LZ", "HUFFMAN"), ("bwt", "BWT+RANK+ZRLT", "ANS0")):
                    if a.chains in (key, "both"):
                        ok &= bench_codec(torch, kz, corpus, codec.device, n, size, bs, transform, entropy, a.repeats, out)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
