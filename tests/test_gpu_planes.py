"""knz_hip_split_many / knz_hip_join_many (csrc/planes.hip) on the device through hipapi.Context.split_many / join_many, against
kanzi.split_bytes / join_bytes: every element width with every pair of source and destination alignment at lengths around 0, 16 elements
and the tile in ONE launch per direction, with guard bytes around every destination; the way there and back; many one-element entries;
the empty call; every refusal by name with the buffers untouched and the context usable afterwards. The kernels' logic with small tiles
and under AddressSanitizer: tests/test_emu_planes.py."""
import importlib

import numpy as np
import pytest

import knzlib

pytestmark = pytest.mark.gpu

TILE = 16384                # PL_TILE of csrc/planes.hip
GUARD = 32
FILL = 0xA5
WIDTHS = (1, 2, 4, 8)


def mods():
    knzlib.load_pkg()
    return importlib.import_module("kanzi_amd.hipapi"), importlib.import_module("kanzi_amd.kanzi")


def run_entries(hip, call, host, src, plan, dst_bytes):
    """plan: (source offset, destination offset, length, width) each, inside a source buffer holding `src` and a destination buffer of
    dst_bytes filled with FILL. One launch of `call`; returns (the destination buffer afterwards, what it has to be by `host`)."""
    d_src, d_dst = hip.malloc(len(src) + 16), hip.malloc(dst_bytes + 16)
    try:
        hip.h2d(d_src, src.tobytes())
        hip.h2d(d_dst, bytes([FILL]) * dst_bytes)
        call([(d_src + s, d_dst + d, n, w) for s, d, n, w in plan])
        got = np.frombuffer(hip.d2h(d_dst, dst_bytes), dtype=np.uint8)
    finally:
        hip.free(d_src)
        hip.free(d_dst)
    want = np.full(dst_bytes, FILL, dtype=np.uint8)
    for s, d, n, w in plan:
        want[d:d + n] = np.frombuffer(host(src[s:s + n], w), dtype=np.uint8)
    return got, want


@pytest.mark.parametrize("direction", ["split", "join"])
def test_every_width_alignment_pair_and_length_in_one_launch(hip, direction):
    _, kz = mods()
    plan, s_at, d_at = [], 0, 0
    for smod in range(16):
        for dmod in range(16):
            for w in WIDTHS:
                for n in (0, w, 15 * w, 16 * w, 17 * w, TILE - w, TILE, TILE + w, 2 * TILE + 5 * w):
                    s = ((s_at + 15) & ~15) + smod
                    d = ((d_at + 15) & ~15) + GUARD + dmod
                    plan.append((s, d, n, w))
                    s_at, d_at = s + n, d + n + GUARD
    assert len(plan) == 256 * 4 * 9
    src = np.random.default_rng(1).integers(0, 256, size=s_at, dtype=np.uint8)
    call, host = (hip.split_many, kz.split_bytes) if direction == "split" else (hip.join_many, kz.join_bytes)
    got, want = run_entries(hip, call, host, src, plan, d_at)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, "first wrong byte at %d of the destination buffer" % bad[0]


def test_join_of_split_gives_the_bytes_back(hip):
    sizes = [(w, m) for w in WIDTHS for m in (1, 16, 4097, 100003)]
    total = sum(w * m for w, m in sizes)
    src = np.random.default_rng(4).integers(0, 256, size=total, dtype=np.uint8)
    d_src, d_mid, d_back = hip.malloc(total + 16), hip.malloc(total + 16), hip.malloc(total + 16)
    try:
        hip.h2d(d_src, src.tobytes())
        there, back, at = [], [], 0
        for w, m in sizes:
            there.append((d_src + at, d_mid + at, w * m, w))
            back.append((d_mid + at, d_back + at, w * m, w))
            at += w * m
        hip.split_many(there)
        hip.join_many(back)
        mid, got = hip.d2h(d_mid, total), hip.d2h(d_back, total)
    finally:
        for d in (d_src, d_mid, d_back):
            hip.free(d)
    assert got == src.tobytes()
    assert mid != got and sorted(mid[-800024:]) == sorted(got[-800024:])          # (the last entry: a permutation of its bytes)


@pytest.mark.parametrize("direction", ["split", "join"])
def test_many_entries_of_one_element(hip, direction):
    n = 65536
    widths = [WIDTHS[i % 4] for i in range(n)]
    s_off = np.concatenate([[0], np.cumsum(widths)])
    src = np.random.default_rng(2).integers(0, 256, size=int(s_off[-1]), dtype=np.uint8)
    order = np.random.default_rng(3).permutation(n)
    plan = [(int(s_off[order[i]]), 10 * i + 1, widths[order[i]], widths[order[i]]) for i in range(n)]
    got, want = run_entries(hip, hip.split_many if direction == "split" else hip.join_many, lambda b, w: b.tobytes(), src, plan, 10 * n)
    assert (got == want).all()
    assert (want[0::10] == FILL).all() and (want[1::10] == src[s_off[order]]).all()


def test_empty_calls(hip):
    hip.split_many([])
    hip.join_many([])
    d = hip.malloc(64)
    try:
        hip.h2d(d, bytes(range(64)))
        hip.split_many([(d, d + 32, 0, 2), (d, d + 32, 0, 8)])
        hip.join_many([(d, d + 32, 0, 1)])
        assert hip.d2h(d, 64) == bytes(range(64))
    finally:
        hip.free(d)


@pytest.mark.parametrize("direction", ["split", "join"])
def test_refusals_leave_the_buffers_alone_and_the_context_usable(hip, direction):
    api, kz = mods()
    call = hip.split_many if direction == "split" else hip.join_many
    image = bytes(range(256)) * 16
    d = hip.malloc(4096)
    good = (d, d + 2048, 16, 2)
    reserved = (api.PlaneCopy * 2)()
    for e, (src, dst, n, w) in zip(reserved, [good, (d, d + 1024, 16, 4)]):
        e.src, e.dst, e.len, e.elem = src, dst, n, w
    reserved[1].reserved = 7
    many_tiles = [(d, d, (1 << 32) - 8, 8)] * 8192              # 8192 * 2^18 tiles = 2^31 (refused before any address is used)
    try:
        hip.h2d(d, image)
        for entries, message in [([good, (d, d + 1024, 12, 3)], "entry 1: elements of 3 bytes"),
                                 ([good, good, (d, d + 1024, 0, 0)], "entry 2: elements of 0 bytes"),
                                 ([(d, d + 1024, 16, 16)], "entry 0: elements of 16 bytes"),
                                 (reserved, "entry 1: reserved is 7"),
                                 ([good, (d, d + 1024, 10, 4)], "entry 1: 10 bytes are no multiple of its 4-byte elements"),
                                 ([good, (d, d + 1024, 1 << 32, 8)], "entry 1: 4294967296 bytes, an entry takes fewer than 2\\^32"),
                                 ((api.PlaneCopy * (api.COPY_MAX_COPIES + 1))(), "too many entries"),
                                 (many_tiles, "2147483648 tiles of 16384 bytes in one call, fewer than 2\\^31")]:
            with pytest.raises(api.KnzError, match=message) as e:
                call(entries)
            assert e.value.code == 18
        assert hip.d2h(d, 4096) == image, "a refused call has moved something"
        # the context is as usable as before
        host = kz.split_bytes if direction == "split" else kz.join_bytes
        call([(d + 3, d + 2048 + 5, 96, 4), (d, d + 4000, 0, 2)])
        back = hip.d2h(d, 4096)
        assert back[2048 + 5:2048 + 101] == host(image[3:99], 4) and back[:2048] == image[:2048]
    finally:
        hip.free(d)


def test_kernels_are_timed_when_profiling(hip):
    d = hip.malloc(4096)
    try:
        hip.set_profiling(True)
        hip.split_many([(d, d + 2048, 1000, 2)])
        hip.join_many([(d, d + 2048, 1000, 4)])
        hip.sync()
        names = [name for name, _, launches in hip.kernel_times() if launches]
    finally:
        hip.set_profiling(False)
        hip.free(d)
    assert "k_split_many" in names and "k_join_many" in names
