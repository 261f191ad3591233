"""knz_hip_copy_many (csrc/copy_many.hip) on the device through hipapi.Context.copy_many: every pair of source and destination alignment
at lengths around 0, 16 and the tile size in ONE launch, with guard bytes around every destination; many one-byte copies; the empty
call; the limits of a call, each refused by name with the context usable afterwards. The kernel's logic with a small tile and under
AddressSanitizer: tests/test_emu_copy_many.py."""
import importlib

import numpy as np
import pytest

import knzlib

pytestmark = pytest.mark.gpu

TILE = 16384                # CM_TILE of csrc/copy_many.hip
GUARD = 32
FILL = 0xA5


def hipapi():
    knzlib.load_pkg()
    return importlib.import_module("kanzi_amd.hipapi")


def run_copies(hip, src, plan, dst_bytes):
    """plan: (source offset, destination offset, length) each, inside a source buffer holding `src` and a destination buffer of dst_bytes
    filled with FILL. One launch; returns (the destination buffer afterwards, what it has to be)."""
    d_src, d_dst = hip.malloc(len(src) + 16), hip.malloc(dst_bytes + 16)
    try:
        hip.h2d(d_src, src.tobytes())
        hip.h2d(d_dst, bytes([FILL]) * dst_bytes)
        hip.copy_many([(d_src + s, d_dst + d, n) for s, d, n in plan])
        got = np.frombuffer(hip.d2h(d_dst, dst_bytes), dtype=np.uint8)
    finally:
        hip.free(d_src)
        hip.free(d_dst)
    want = np.full(dst_bytes, FILL, dtype=np.uint8)
    for s, d, n in plan:
        want[d:d + n] = src[s:s + n]
    return got, want


def test_every_alignment_pair_and_length_in_one_launch(hip):
    lens = [0, 1, 15, 16, 17, 31, 33, TILE - 1, TILE, TILE + 1, 2 * TILE + 5]
    plan, s_at, d_at = [], 0, 0
    for smod in range(16):
        for dmod in range(16):
            for n in lens:
                s = ((s_at + 15) & ~15) + smod
                d = ((d_at + 15) & ~15) + GUARD + dmod
                plan.append((s, d, n))
                s_at, d_at = s + n, d + n + GUARD
    assert len(plan) == 256 * 11
    src = np.random.default_rng(1).integers(0, 256, size=s_at, dtype=np.uint8)
    got, want = run_copies(hip, src, plan, d_at)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, "first wrong byte at %d of the destination buffer" % bad[0]


def test_many_copies_of_one_byte(hip):
    n = 65536
    src = np.random.default_rng(2).integers(0, 256, size=n, dtype=np.uint8)
    order = np.random.default_rng(3).permutation(n)
    got, want = run_copies(hip, src, [(int(order[i]), 3 * i + 1, 1) for i in range(n)], 3 * n)
    assert (got == want).all()
    assert (want[1::3] == src[order]).all() and (want[0::3] == FILL).all()


def test_empty_call_and_limits(hip):
    api = hipapi()
    hip.copy_many([])
    d = hip.malloc(4096)
    try:
        hip.h2d(d, bytes(range(256)) * 16)
        with pytest.raises(api.KnzError, match="fewer than 2\\^32") as e:
            hip.copy_many([(d, d + 2048, 16), (d, d + 1024, 1 << 32)])
        assert e.value.code == 18
        with pytest.raises(api.KnzError, match="too many copies") as e:
            hip.copy_many((api.Copy * (api.COPY_MAX_COPIES + 1))())
        assert e.value.code == 18
        assert hip.d2h(d, 4096) == bytes(range(256)) * 16, "a refused call has copied something"
        # the context is as usable as before
        hip.copy_many([(d + 3, d + 2048 + 5, 100), (d, d + 4000, 0)])
        back = hip.d2h(d, 4096)
        assert back[2048 + 5:2048 + 105] == (bytes(range(256)) * 16)[3:103] and back[:2048] == (bytes(range(256)) * 16)[:2048]
    finally:
        hip.free(d)


def test_kernel_is_timed_when_profiling(hip):
    d = hip.malloc(4096)
    try:
        hip.set_profiling(True)
        hip.copy_many([(d, d + 2048, 1000)])
        hip.sync()
        names = [name for name, _, launches in hip.kernel_times() if launches]
    finally:
        hip.set_profiling(False)
        hip.free(d)
    assert "k_copy_many" in names
