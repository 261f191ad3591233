"""Times MM (FSDCodec) forward and inverse on N blocks of 4 MiB: WAV-like data (XOR mode, distance 4) and a byte walk with 1 % escapes
(delta mode, distance 1), one batch through knz_hip_encode_blocks / _decode_blocks with NONE entropy. Beside each:
  (a) a device-to-device copy of the same bytes (hipMemcpyAsync between HIP events): the floor of a stage that reads N and writes N bytes,
  (b) PACK on the same batch (wall clock of the whole call, next to MM's wall clock and that of the chain NONE: all include block
      framing, so a stage is its call minus NONE's),
  (c) the reference's FSDCodec from oracle/_ref on the host, one thread per block (wall clock; skipped where the build is absent).
MM's own figure is the sum of its kernels' HIP-event times (knz_hip_set_profiling), warm, the median of --steps runs.
The encoder never writes an all-escape block and the batch entry points only decode what an encoder wrote, so the all-escape inverse
(mode 0, distance 1, 2 Mi escape pairs) goes through the per-stage entry point, one block, beside the walk's forward output through
the same entry point: kernel HIP-event sums again.
    python tools/gpu_mm_time.py [--blocks 64] [--steps 7]
For per-kernel times: rocprofv3 --kernel-trace --stats -d OUT -o run -- python tools/gpu_mm_time.py --steps 2
"""
import argparse
import os
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import knzlib  # noqa: E402
import mm_cases  # noqa: E402
import pack_cases  # noqa: E402

BS = 4 << 20


def kernel_ms(ctx, prefix):
    return sum(ms for name, ms, _ in ctx.kernel_times() if name.startswith(prefix))


def med(v):
    return statistics.median(v)


def copy_ms(ctx, n, steps):
    """hipMemcpyAsync device to device between two events on the null stream, through the HIP runtime the library itself uses."""
    import ctypes as C
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    hip.hipEventRecord.argtypes = [C.c_void_p, C.c_void_p]
    hip.hipEventSynchronize.argtypes = [C.c_void_p]
    hip.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]
    a, b = ctx.malloc(n), ctx.malloc(n)
    e0, e1 = C.c_void_p(), C.c_void_p()
    assert hip.hipEventCreate(C.byref(e0)) == 0 and hip.hipEventCreate(C.byref(e1)) == 0
    out = []
    for i in range(steps + 2):
        assert hip.hipEventRecord(e0, None) == 0
        assert hip.hipMemcpyAsync(b, a, n, 3, None) == 0            # hipMemcpyDeviceToDevice
        assert hip.hipEventRecord(e1, None) == 0
        assert hip.hipEventSynchronize(e1) == 0
        ms = C.c_float(0)
        assert hip.hipEventElapsedTime(C.byref(ms), e0, e1) == 0
        if i >= 2:
            out.append(ms.value)
    hip.hipEventDestroy.argtypes = [C.c_void_p]
    hip.hipEventDestroy(e0)
    hip.hipEventDestroy(e1)
    ctx.free(a)
    ctx.free(b)
    return med(out)


def batch(ctx, chain, d_in, n, steps):
    """(wall encode ms, wall decode ms, MM kernels forward ms, MM kernels inverse ms, ratio) of one batch."""
    p = ctx.params(chain, "NONE", BS)
    cap = ctx.encode_bound(p, n)
    d_out, d_dec = ctx.malloc(cap), ctx.malloc(n + BS + 64)
    te, td, kf, ki = [], [], [], []
    for prof in (False, True):
        ctx.set_profiling(prof)
        for i in range(steps + 2):
            t0 = time.perf_counter()
            bits = ctx.encode_blocks(p, d_in, n, d_out, cap)
            t1 = time.perf_counter()
            f = kernel_ms(ctx, "k_mm_f_") if prof else 0.0
            t2 = time.perf_counter()
            ob, _, _ = ctx.decode_blocks(p, d_out, bits, 0, d_dec, n + BS)
            t3 = time.perf_counter()
            assert ob == n
            if i < 2:
                continue
            if prof:
                kf.append(f)
                ki.append(kernel_ms(ctx, "k_mm_i_"))
            else:
                te.append(1e3 * (t1 - t0))
                td.append(1e3 * (t3 - t2))
    ctx.set_profiling(False)
    ctx.free(d_out)
    ctx.free(d_dec)
    return med(te), med(td), med(kf), med(ki), (bits / 8) / n


def reference_ms(block, nblocks):
    try:
        ref = knzlib.Ref()
    except Exception:
        return None
    cap = mm_cases.max_encoded(len(block))
    ok, fwd, _ = ref.forward("MM", block, cap)
    assert ok == 1
    with ThreadPoolExecutor(nblocks) as pool:
        t0 = time.perf_counter()
        list(pool.map(lambda _: ref.forward("MM", block, cap), range(nblocks)))
        t1 = time.perf_counter()
        list(pool.map(lambda _: ref.inverse("MM", fwd, cap), range(nblocks)))
        t2 = time.perf_counter()
    return 1e3 * (t1 - t0), 1e3 * (t2 - t1)


def stage_inverse_ms(ctx, data, cap, steps):
    out = []
    ctx.set_profiling(True)
    for i in range(steps + 2):
        ok, _ = ctx.transform_inverse("MM", data, cap)
        assert ok
        if i >= 2:
            out.append(kernel_ms(ctx, "k_mm_i_"))
    ctx.set_profiling(False)
    return med(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=64)
    ap.add_argument("--steps", type=int, default=7)
    a = ap.parse_args()
    assert a.steps >= 5, "the median of at least 5 runs"
    knzlib.load_pkg()
    import importlib
    hipapi = importlib.import_module("kanzi_amd.hipapi")
    ctx = hipapi.Context(0)
    n = BS * a.blocks
    print("device-to-device copy of %d x 4 MiB: %.3f ms" % (a.blocks, copy_ms(ctx, n, a.steps)), flush=True)
    walk = mm_cases.walk(BS, 7, 1, 0.01)
    for kind, block in (("wav", pack_cases.wav(BS, 7)), ("walk 1% escapes", walk)):
        d_in = ctx.malloc(n + 64)
        ctx.h2d(d_in, block * a.blocks)
        te, td, kf, ki, ratio = batch(ctx, "MM", d_in, n, a.steps)
        print("%-16s MM   kernels forward %8.3f ms  inverse %8.3f ms | whole call encode %8.2f ms  decode %8.2f ms  ratio %.4f" %
              (kind, kf, ki, te, td, ratio), flush=True)
        te, td, _, _, ratio = batch(ctx, "PACK", d_in, n, a.steps)
        print("%-16s PACK                                                  | whole call encode %8.2f ms  decode %8.2f ms  ratio %.4f" %
              (kind, te, td, ratio), flush=True)
        te, td, _, _, _ = batch(ctx, "NONE", d_in, n, a.steps)
        print("%-16s NONE (framing alone)                                  | whole call encode %8.2f ms  decode %8.2f ms" % (kind, te, td), flush=True)
        ctx.free(d_in)
        r = reference_ms(block, a.blocks)
        if r:
            print("%-16s reference FSDCodec, %d host threads: forward %8.2f ms  inverse %8.2f ms" % (kind, a.blocks, r[0], r[1]), flush=True)
        else:
            print("%-16s reference build not available" % kind, flush=True)
    ok, fwd = ctx.transform_forward("MM", walk, mm_cases.max_encoded(BS))
    assert ok
    esc = bytes([0, 1, 100]) + bytes([255, 3]) * (BS // 2)
    friendly = stage_inverse_ms(ctx, fwd, mm_cases.max_encoded(BS), a.steps)
    hostile = stage_inverse_ms(ctx, esc, BS, a.steps)
    print("one block, per-stage inverse kernels: walk %.3f ms (%d bytes in)  all-escape %.3f ms (%d bytes in)  ratio %.2f" %
          (friendly, len(fwd), hostile, len(esc), hostile / friendly), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
