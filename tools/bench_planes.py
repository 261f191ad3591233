"""Byte planes on the GPU: (a) the kernels of knz_hip_split_many / knz_hip_join_many for elements of 2 and 4 bytes beside knz_hip_copy_many
of the same bytes (one read and one write per byte in all three) and beside torch's own transpose of the bytes,
t.view(n, -1, w).transpose(1, 2).contiguous(); (b) what kanzi.TensorCodec.compress(planes=True) makes of bf16 and fp32 weights.

(a) one entry of 256 MiB and 4,096 entries of 64 KiB, sources and destinations at multiples of 16. Per call: device events on the codec's
    stream around `inner` calls in a row (the table upload of every call included); the kernel alone: knz_hip_get_kernel_times, in runs of
    their own. The variants take turns inside every one of the --repeats rounds (after a warm-up round); every figure is the median with
    the fastest and the slowest beside it. GB/s counts the payload once (the memory moves twice as many bytes). Every result is compared
    with torch's.
(b) 1 Mi values of N(0, 0.02) as bf16 and as fp32 under NONE / HUFFMAN, NONE / ANS0 and BWT+RANK+ZRLT / ANS0 in blocks of --block bytes:
    the stream's bytes as the values lie and as planes, and that both come back.

    python tools/bench_planes.py [--out FILE] [--repeats N] [--inner N] [--only kernels|sizes] [--shapes one|many|both] [--block BYTES]
"""
import argparse
import importlib
import importlib.util
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "kanzi-cpp_amd")
SHAPES = {"one": (1, 256 << 20), "many": (4096, 65536)}           # entries, bytes each
CHAINS = [("NONE", "HUFFMAN"), ("NONE", "ANS0"), ("BWT+RANK+ZRLT", "ANS0")]
KERNELS = {"copy": "k_copy_many", "split": "k_split_many", "join": "k_join_many"}


def load():
    if "kanzi_amd" not in sys.modules:
        spec = importlib.util.spec_from_file_location("kanzi_amd", os.path.join(PKG, "__init__.py"), submodule_search_locations=[PKG])
        mod = importlib.util.module_from_spec(spec)
        sys.modules["kanzi_amd"] = mod
        spec.loader.exec_module(mod)
    return [importlib.import_module("kanzi_amd." + m) for m in ("hipapi", "kanzi")]


def spread(times):
    return "%8.3f ms (%.3f - %.3f)" % (statistics.median(times), min(times), max(times))


def event_ms(torch, stream, fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    for _ in range(inner):
        fn()
    b.record(stream)
    b.synchronize()
    return a.elapsed_time(b) / inner


def kernel_ms(ctx, fn, name):
    ctx.set_profiling(True)
    fn()
    ms = [t for k, t, _ in ctx.kernel_times() if k == name]
    ctx.set_profiling(False)
    return ms[0]


def bench_kernels(torch, hipapi, codec, n, size, inner, repeats, out):
    total = n * size
    src = torch.randint(0, 256, (total,), dtype=torch.uint8, device=codec.device)
    dst = torch.empty(total, dtype=torch.uint8, device=codec.device)
    assert src.data_ptr() % 16 == 0 and dst.data_ptr() % 16 == 0
    ctx = codec.ctx
    copies = (hipapi.Copy * n)()
    for i in range(n):
        copies[i].src, copies[i].dst, copies[i].len = src.data_ptr() + i * size, dst.data_ptr() + i * size, size
    variants = [("copy", 0, lambda: ctx.copy_many(copies), None)]
    for w in (2, 4):
        table = (hipapi.PlaneCopy * n)()
        for i in range(n):
            table[i].src, table[i].dst, table[i].len, table[i].elem = src.data_ptr() + i * size, dst.data_ptr() + i * size, size, w
        variants.append(("split", w, lambda table=table: ctx.split_many(table), None))
        variants.append(("join", w, lambda table=table: ctx.join_many(table), None))
        variants.append(("torch", w, None, lambda w=w: src.view(n, size // w, w).transpose(1, 2).contiguous()))
        variants.append(("torch back", w, None, lambda w=w: src.view(n, w, size // w).transpose(1, 2).contiguous()))
    # every variant's result against torch's, once
    ok = True
    for name, w, call, _ in variants:
        if call is not None:
            dst.zero_()
            call()
            want = src if name == "copy" else src.view(n, size // w, w).transpose(1, 2) if name == "split" else src.view(n, w, size // w).transpose(1, 2)
            good = torch.equal(dst.view(want.shape), want)
            ok &= good
            if not good:
                out.write("%5d x %9d B  %s, width %d: WRONG\n" % (n, size, name, w))
    if not ok:
        return False
    calls, kerns = {}, {}
    for r in range(repeats + 1):
        for name, w, call, op in variants:
            ms = event_ms(torch, codec.stream, call or op, inner)
            if r:
                calls.setdefault((name, w), []).append(ms)
        for name, w, call, _ in variants:
            if call is not None:
                ms = kernel_ms(ctx, call, KERNELS[name])
                if r:
                    kerns.setdefault((name, w), []).append(ms)
    gbs = lambda times: total / 1e6 / statistics.median(times)
    base_call, base_kern = gbs(calls[("copy", 0)]), gbs(kerns[("copy", 0)])
    for name, w, call, _ in variants:
        what = "%-10s %s" % (name, "width %d" % w if w else "       ")
        out.write("%5d x %9d B  %s  call  : %s  %7.1f GB/s  x%.2f of copy_many\n" % (n, size, what, spread(calls[(name, w)]), gbs(calls[(name, w)]), gbs(calls[(name, w)]) / base_call))
        if call is not None:
            out.write("%5d x %9d B  %s  kernel: %s  %7.1f GB/s  x%.2f of copy_many\n" % (n, size, what, spread(kerns[(name, w)]), gbs(kerns[(name, w)]), gbs(kerns[(name, w)]) / base_kern))
    out.flush()
    return True


def bench_sizes(torch, codec, block, out):
    g = torch.Generator().manual_seed(5)
    values = torch.randn(1 << 20, generator=g) * 0.02
    ok = True
    for dtype in (torch.bfloat16, torch.float32):
        t = values.to(dtype).to(codec.device)
        nbytes = t.numel() * t.element_size()
        for transform, entropy in CHAINS:
            sizes = []
            for planes in (False, True):
                blob, offsets = codec.compress([t], transform, entropy, block, planes=planes)
                back = codec.decompress(blob, offsets, planes=[t.element_size()] if planes else None)
                ok &= torch.equal(back[0].view(dtype).view(torch.uint8), t.view(torch.uint8))
                sizes.append(offsets[1])
            out.write("%-9s %8d B  %-14s %-8s as they lie %8d B (%.3f bits/byte)  planes %8d B (%.3f bits/byte)  x%.3f\n"
                      % (str(dtype).replace("torch.", ""), nbytes, transform, entropy, sizes[0], 8 * sizes[0] / nbytes, sizes[1], 8 * sizes[1] / nbytes, sizes[1] / sizes[0]))
            out.flush()
    return ok


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--only", choices=("kernels", "sizes"), default="")
    ap.add_argument("--shapes", choices=("one", "many", "both"), default="both")
    ap.add_argument("--block", type=int, default=65536)
    a = ap.parse_args()
    import torch
    hipapi, kz = load()
    out = open(a.out, "w") if a.out else sys.stdout
    ok = True
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream), kz.TensorCodec() as codec:
        if a.only != "sizes":
            out.write("median of %d rounds after a warm-up (fastest - slowest); calls: device events around %d calls in a row\n" % (a.repeats, a.inner))
            for key in (("one", "many") if a.shapes == "both" else (a.shapes,)):
                ok &= bench_kernels(torch, hipapi, codec, *SHAPES[key], a.inner, a.repeats, out)
        if a.only != "kernels":
            ok &= bench_sizes(torch, codec, a.block, out)
    out.write("ok\n" if ok else "WRONG\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
