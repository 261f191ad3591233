"""The device-wide primitives of csrc/prims.hpp by themselves on the GPU (knz_hip_prims_scan / knz_hip_prims_sort): the prefix scans and
the segmented stable LSD radix sort against plain numpy, exactly, at the sizes where the kernels change path. Every boundary is computed
from the constants the library reports (knz_hip_prims_info), so that a change of a tile size moves the cases with it. The emulator
(tests/test_emu_kernels.py) checks the same code where memory is sequentially consistent and workgroups never wait; here the look-back
of the one-read pass runs on the real memory system, the column scan runs over several groups, and the count + scatter path runs at all."""
import ctypes as C
import functools
import importlib

import numpy as np
import pytest

import knzlib
import vectors

pytestmark = pytest.mark.gpu

SENTINEL = 0xDEADBEEF
STALE = 0x12345678
OPS = (0, 1, 2)                      # exclusive sum, inclusive max, inclusive min


@functools.lru_cache(maxsize=None)
def info():
    knzlib.load_pkg()
    return importlib.import_module("kanzi_amd.hipapi").prims_info()      # (RS_TILE, RS_GROUP, SC_TILE, RS_MAXPASS)


class Dev:
    """Device arrays that live for one `with` block."""

    def __init__(self, hip):
        self.hip, self.ptrs = hip, []

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        for p in self.ptrs:
            self.hip.free(p)

    def alloc(self, nbytes):
        p = self.hip.malloc(max(nbytes, 16))
        self.ptrs.append(p)
        return p

    def put(self, p, arr):
        arr = np.ascontiguousarray(arr)
        if arr.nbytes:
            self.hip._chk(self.hip.L.knz_hip_memcpy_h2d(self.hip.h, C.c_void_p(p), arr.ctypes.data_as(C.c_char_p), arr.nbytes))

    def up(self, arr):
        p = self.alloc(arr.nbytes)
        self.put(p, arr)
        return p

    def down(self, p, n, dtype):
        out = np.empty(n, dtype)
        if out.nbytes:
            self.hip._chk(self.hip.L.knz_hip_memcpy_d2h(self.hip.h, C.c_void_p(out.ctypes.data), C.c_void_p(p), out.nbytes))
        return out


# ---------------------------------------------------------------------------------------------------------------------------------
# scans
# ---------------------------------------------------------------------------------------------------------------------------------
def scan_sizes():
    S = info()[2]
    # 4096 tiles: the last size with one trip of the loop in k_scan_carries (256 threads x 16 partials) and a grid that does not stride;
    # 4096 S + S + 1: the first with a second trip and with tiles that workgroups reach by striding
    return [1, 15, 16, 17, S - 1, S, S + 1, 3 * S + 5, 4096 * S - 1, 4096 * S, 4096 * S + S + 1]


def scan_input(kind, n):
    if kind == "random":                 # all 32 bits: the sum wraps, half the values have bit 31 set
        return np.random.default_rng(1000 + n % 997).integers(0, 1 << 32, n, dtype=np.uint32)
    if kind == "ones":
        return np.ones(n, dtype=np.uint32)
    if kind == "allbits":
        return np.full(n, 0xFFFFFFFF, dtype=np.uint32)
    assert kind == "ramp"                # descending from 2^32 - 1: every word is a new minimum, the first one the maximum
    return (np.uint64(0xFFFFFFFF) - np.arange(n, dtype=np.uint64)).astype(np.uint32)


@functools.lru_cache(maxsize=2)
def scan_case(kind, n):
    """(input, (exclusive sum, inclusive max, inclusive min), wrapped sum of all): the references, computed once per input. A scan of the
    first m words is the first m words of the scan, so the shorter runs share them."""
    x = scan_input(kind, n)
    incl = np.cumsum(x, dtype=np.uint64) & np.uint64(0xFFFFFFFF)
    excl = np.empty(n, dtype=np.uint32)
    excl[0] = 0
    excl[1:] = incl[:-1].astype(np.uint32)
    refs = (excl, np.maximum.accumulate(x), np.minimum.accumulate(x))
    for r in refs:
        r.setflags(write=False)
    x.setflags(write=False)
    return x, refs, int(incl[-1])


def run_scans(hip, kind, n, modes):
    """Every op, out of place and in place, for each (n_max, *d_n or None) of `modes`; all of them must scan exactly n words."""
    x, refs, total = scan_case(kind, n)
    pad = max(nm for nm, _ in modes) - n + 64
    host_in = np.concatenate([x, np.full(pad, SENTINEL, dtype=np.uint32)])
    sent = np.full(n + pad, SENTINEL, dtype=np.uint32)
    with Dev(hip) as d:
        d_in, d_out, d_buf = d.up(host_in), d.alloc(host_in.nbytes), d.alloc(host_in.nbytes)
        d_n, d_total = d.alloc(4), d.alloc(4)
        for n_max, ndev in modes:
            if ndev is not None:
                d.put(d_n, np.array([ndev], dtype=np.uint32))
            for op in OPS:
                for in_place in (False, True):
                    if in_place:
                        d.put(d_buf, host_in)
                    else:
                        d.put(d_out, sent)
                    d.put(d_total, np.array([STALE], dtype=np.uint32))
                    src, dst = (d_buf, d_buf) if in_place else (d_in, d_out)
                    hip.prims_scan(op, src, dst, n_max, d_n if ndev is not None else None, d_total if op == 0 else None)
                    got = d.down(dst, n + pad, np.uint32)
                    what = (kind, n, "op %d" % op, "in place" if in_place else "out of place", "n_max %d" % n_max, "*d_n %s" % ndev)
                    assert np.array_equal(got[:n], refs[op]), what + ("first difference at %d" % int(np.flatnonzero(got[:n] != refs[op])[0]),)
                    assert (got[n:] == SENTINEL).all(), what + ("words behind n were written",)
                    if op == 0:
                        assert int(d.down(d_total, 1, np.uint32)[0]) == total, what + ("total",)
            assert np.array_equal(d.down(d_in, n, np.uint32), x), (kind, n, n_max, ndev, "the input of the out-of-place runs changed")


@pytest.mark.parametrize("n", scan_sizes())
def test_scan_random_words(hip, n):
    """Sum (exclusive, wrapping), max and min (inclusive) of full 32-bit random words: the size given by the host, by a device word below
    n_max (n_max reaches one tile further than n, so the grid is larger than the data) and by a device word above n_max, which clamps."""
    S = info()[2]
    run_scans(hip, "random", n, [(n, None), (n + S + 3, n), (n, n + 1000)])


@pytest.mark.parametrize("kind", ["ones", "allbits", "ramp"])
def test_scan_patterns(hip, kind):
    """All ones (the exclusive sum is the index: a tile carry that is off by one tile shows), all bits set (the sum wraps at every step)
    and a descending ramp (min changes at every word, max never), at a few tiles and at the first size with a striding grid."""
    S = info()[2]
    for n in (3 * S + 5, 4096 * S + S + 1):
        run_scans(hip, kind, n, [(n, None), (n + 7, n)])


@pytest.mark.parametrize("n_max", [1, 17, "S+1", "4096S+S+1"])
def test_scan_of_no_words(hip, n_max):
    """*d_n == 0 under n_max > 0 (the suffix sort passes a device-side count that can be 0 and reads the total back): out is untouched
    and the total reads 0, not what the word held before."""
    S = info()[2]
    n_max = {"S+1": S + 1, "4096S+S+1": 4096 * S + S + 1}.get(n_max, n_max)
    host = np.full(n_max + 64, SENTINEL, dtype=np.uint32)
    with Dev(hip) as d:
        d_in, d_out = d.up(np.full(n_max + 64, 7, dtype=np.uint32)), d.alloc(host.nbytes)
        d_n, d_total = d.up(np.zeros(1, dtype=np.uint32)), d.alloc(4)
        for op in OPS:
            for in_place in (False, True):
                d.put(d_out, host)
                d.put(d_total, np.array([STALE], dtype=np.uint32))
                hip.prims_scan(op, d_out if in_place else d_in, d_out, n_max, d_n, d_total if op == 0 else None)
                assert (d.down(d_out, n_max + 64, np.uint32) == SENTINEL).all(), (n_max, op, in_place)
                if op == 0:
                    assert int(d.down(d_total, 1, np.uint32)[0]) == 0, (n_max, in_place)
        # n_max == 0 launches nothing: the total keeps what it held
        d.put(d_total, np.array([STALE], dtype=np.uint32))
        hip.prims_scan(0, d_in, d_out, 0, None, d_total)
        assert int(d.down(d_total, 1, np.uint32)[0]) == STALE


# ---------------------------------------------------------------------------------------------------------------------------------
# sorts
# ---------------------------------------------------------------------------------------------------------------------------------
# (key bytes, values, lo bit, hi bit, keep)
HARNESS_TYPES = [(8, False, 0, 64, 0), (8, True, 3, 45, 0), (4, True, 0, 21, 0), (4, False, 8, 32, 0)]       # the emulator harness's matrix
ALL_TYPES = HARNESS_TYPES + [(4, True, 0, 1, 0), (4, True, 0, 5, 0), (4, True, 0, 9, 0),                    # one bit; a masked digit; two passes, the last one bit
                             (4, True, 0, 21, 1)]                                                        # rs_sort_keep as the LZ candidate sort calls it
KINDS = ["random", "two bits", "zero", "high 16", "sorted", "reverse", "63 of 64", "one tile's digit"]


def type_id(t):
    return "u%d%s[%d,%d)%s" % (8 * t[0], "+v" if t[1] else "", t[2], t[3], "keep" if t[4] else "")


def field(keys, lo, hi):
    """The bits the sort looks at, in the narrowest type (numpy sorts 8- and 16-bit integers with a radix sort)."""
    nb = hi - lo
    f = keys >> keys.dtype.type(lo)
    if nb < 8 * keys.dtype.itemsize:
        f = f & keys.dtype.type((1 << nb) - 1)
    return f.astype(np.uint8 if nb <= 8 else np.uint16 if nb <= 16 else keys.dtype)


def make_keys(kind, seg_lens, key_bytes, lo, hi, seed):
    """Keys of all segments; the kinds that speak of rows and tiles are laid out per segment (a tile never straddles segments)."""
    T = info()[0]
    rng = np.random.default_rng(seed)
    dt = np.uint64 if key_bytes == 8 else np.uint32
    n = int(sum(seg_lens))
    r = rng.integers(0, 1 << 64, n, dtype=np.uint64).astype(dt)
    if kind == "random":
        return r
    if kind == "two bits":
        return r & dt(0x0303030303030303 & ((1 << (8 * key_bytes)) - 1))
    if kind == "zero":                   # every row shows one digit: the one-digit path of the ranking, and every tile waits on digit 0
        return np.zeros(n, dtype=dt)
    if kind == "high 16":
        return r | dt(0xFFFF << (8 * key_bytes - 16))
    out = r.copy()
    at = 0
    for ln in seg_lens:
        seg = out[at:at + ln]
        if kind in ("sorted", "reverse"):
            o = np.argsort(field(seg, lo, hi), kind="stable")
            seg[:] = seg[o] if kind == "sorted" else seg[o][::-1]
        elif kind == "63 of 64":         # rows of 64 keys: one lane (another one in every row) differs, so no row takes the one-digit path
            rows, lane = np.arange(ln) // 64, np.arange(ln) % 64
            same = dt(0x5A5A5A5A5A5A5A5A & ((1 << (8 * key_bytes)) - 1))
            seg[:] = np.where(lane == (rows * 7 + 3) % 64, same ^ dt(1 << lo), same)       # (bit lo is part of the first pass's digit)
        else:                            # the first pass's highest digit in ONE tile only (the second if there is one), and all over it:
            assert kind == "one tile's digit"                                   # that tile's status word carries a whole tile's count
            w = min(8, hi - lo)
            star = dt(((1 << w) - 1) << lo)
            seg[(seg & star) == star] ^= dt(1 << lo)
            t0 = T if ln > T else 0
            seg[t0:t0 + T] |= star
        at += ln
    return out


def sort_reference(keys, seg_lens, lo, hi):
    """For each segment np.argsort(field, kind="stable"), as global indices: the expected values; keys[order] are the expected keys."""
    order = np.empty(len(keys), dtype=np.int64)
    f = field(keys, lo, hi)
    starts = np.concatenate([[0], np.cumsum(seg_lens)])

    def one(g):
        a, b = int(starts[g]), int(starts[g + 1])
        order[a:b] = np.argsort(f[a:b], kind="stable") + a

    if len(seg_lens) < 16:
        for g in range(len(seg_lens)):
            one(g)
    else:                                # (thousands of segments: numpy sorts without the interpreter lock)
        from concurrent.futures import ThreadPoolExecutor
        with ThreadPoolExecutor(max_workers=8) as pool:
            list(pool.map(one, range(len(seg_lens)), chunksize=64))
    return order


class SortCase:
    """One input on the device, its numpy reference computed once, sorted by both paths."""

    def __init__(self, hip, typ, kind, seg_lens, seed=1):
        self.hip, self.typ, self.kind, self.seg_lens = hip, typ, kind, seg_lens
        key_bytes, has_val, lo, hi, keep = typ
        self.dt = np.uint64 if key_bytes == 8 else np.uint32
        self.keys = make_keys(kind, seg_lens, key_bytes, lo, hi, seed)
        self.n = len(self.keys)
        self.base = np.concatenate([[0], np.cumsum(np.asarray(seg_lens, dtype=np.uint64))]).astype(np.uint32)
        order = sort_reference(self.keys, seg_lens, lo, hi)
        self.want_keys = self.keys[order]
        self.want_vals = order.astype(np.uint32)

    def run(self, d, one_read):
        """Sorts on the device; returns (keys, values or None) and asserts that the caller's arrays are as they were."""
        key_bytes, has_val, lo, hi, keep = self.typ
        vals = np.arange(self.n, dtype=np.uint32)            # the global index: equal keys must keep their order
        d_k, d_v, d_b = d.up(self.keys), (d.up(vals) if has_val else None), d.up(self.base)
        d_ko, d_vo = d.alloc(self.keys.nbytes), (d.alloc(vals.nbytes) if has_val else None)
        self.hip.prims_sort(key_bytes, has_val, keep, one_read, d_k, d_v, d_b, len(self.seg_lens), max(max(self.seg_lens), 1), lo, hi, d_ko, d_vo)
        assert np.array_equal(d.down(d_k, self.n, self.dt), self.keys), self.what(one_read) + ("the input keys changed",)
        if has_val:
            assert np.array_equal(d.down(d_v, self.n, np.uint32), vals), self.what(one_read) + ("the input values changed",)
        return d.down(d_ko, self.n, self.dt), (d.down(d_vo, self.n, np.uint32) if has_val else None)

    def what(self, one_read):
        return (type_id(self.typ), self.kind, "%d segments, %d keys" % (len(self.seg_lens), self.n), "one-read" if one_read else "count + scatter")

    def check(self, paths=(1, 0)):
        for one_read in paths:
            with Dev(self.hip) as d:
                ko, vo = self.run(d, one_read)
            assert np.array_equal(ko, self.want_keys), self.what(one_read) + ("keys: first difference at %d" % int(np.flatnonzero(ko != self.want_keys)[0]),)
            if vo is not None:
                assert np.array_equal(vo, self.want_vals), self.what(one_read) + ("values (stability): first difference at %d" % int(np.flatnonzero(vo != self.want_vals)[0]),)


@pytest.mark.parametrize("size", ["1", "T-1", "T", "T+1"])
def test_sort_one_segment_around_a_tile(hip, size):
    """One key, and one tile and its neighbours: every key type, bit range and key kind, both paths."""
    T = info()[0]
    n = {"1": 1, "T-1": T - 1, "T": T, "T+1": T + 1}[size]
    for typ in ALL_TYPES:
        for kind in KINDS:
            SortCase(hip, typ, kind, [n]).check()


@pytest.mark.parametrize("size", ["GT-1", "GT", "GT+1", "3GT+T+1"])
def test_sort_across_groups_of_the_column_scan(hip, size):
    """RS_GROUP tiles and their neighbours (one, one and two groups) and four groups: k_rs_colscan1 over more than one group,
    k_rs_colscan2, the group carry in k_rs_scatter -- and, on the one-read path, look-back chains of that many tiles."""
    T, G = info()[0], info()[1]
    n = {"GT-1": G * T - 1, "GT": G * T, "GT+1": G * T + 1, "3GT+T+1": 3 * G * T + T + 1}[size]
    for typ in HARNESS_TYPES + ALL_TYPES[-1:]:
        for kind in ("random", "two bits"):
            SortCase(hip, typ, kind, [n]).check()


@pytest.mark.parametrize("typ,kind", [((8, False, 0, 64, 0), "random"), ((4, True, 0, 8, 0), "zero")], ids=["u64-random", "u32+v-zero"])
def test_sort_long_look_back(hip, typ, kind):
    """1,100 tiles and a few keys: far more tiles than compute units, so tiles of every XCD look back at each other's status words. With
    all-zero keys every tile waits for digit 0 of every tile in front of it."""
    T = info()[0]
    SortCase(hip, typ, kind, [1100 * T + 17]).check()


def ragged_layout():
    T, G = info()[0], info()[1]
    rng = np.random.default_rng(77)
    lens = rng.integers(0, 2 * T + 4, 3000)                       # 0 .. 2 T + 3
    lens[rng.random(3000) < 0.1] = 0
    lens[0] = lens[-1] = 0
    for at in (1, 1499, 2998):                                    # behind the empty first one, in the middle, in front of the empty last one
        lens[at] = G * T + 5
    return [int(x) for x in lens]


@pytest.mark.parametrize("typ", [(4, True, 0, 21, 0), (8, False, 3, 45, 0)], ids=type_id)
def test_sort_ragged_segments(hip, typ):
    """What a batch of small blocks looks like: 3,000 segments of 0 to 2 T + 3 keys, a tenth of them empty, the first and the last
    empty, and three segments of more than one group among them (tileOff and grpOff behind segments of every shape)."""
    lens = ragged_layout()
    assert len(lens) == 3000 and lens[0] == 0 and lens[-1] == 0 and 200 < lens.count(0) < 400
    SortCase(hip, typ, "random", lens).check()


def test_sort_above_the_grid_cap(hip):
    """Two segments, the first longer than the 2,048 tiles a grid row gets when there is more than one segment (rs_grid_x): k_rs_count
    and k_rs_scatter reach the tiles behind by striding."""
    T = info()[0]
    SortCase(hip, (4, False, 0, 8, 0), "random", [2048 * T + T + 9, 5]).check()


def test_sort_twice_gives_the_same_bytes(hip):
    """The same input sorted again, by the same path and by the other one in between: status words, ticket counters or histograms left
    from a sort must not reach the next one."""
    T, G = info()[0], info()[1]
    case = SortCase(hip, (4, True, 0, 21, 0), "random", [T + 1, G * T + 1, 3])
    outs = []
    with Dev(hip) as d:
        for one_read in (1, 1, 0, 1, 0, 0):
            ko, vo = case.run(d, one_read)
            outs.append(ko.tobytes() + vo.tobytes())
    assert all(o == outs[0] for o in outs)
    assert outs[0] == case.want_keys.tobytes() + case.want_vals.tobytes()


def test_sort_probe_refuses_a_bad_segment_table(hip):
    """The kernels trust the segment table; the probe checks it before it launches anything."""
    hipapi = importlib.import_module("kanzi_amd.hipapi")
    with Dev(hip) as d:
        d_k, d_o = d.up(np.zeros(64, dtype=np.uint32)), d.alloc(256)
        for base, max_len in (([1, 5], 8), ([0, 9, 5], 16), ([0, 40], 8)):
            with pytest.raises(hipapi.KnzError):
                hip.prims_sort(4, 0, 0, 1, d_k, None, d.up(np.array(base, dtype=np.uint32)), len(base) - 1, max_len, 0, 8, d_o, None)


def test_bwt_forward_on_the_count_and_scatter_path(hip, oracle):
    """The suffix sort with the knob "rs_onesweep" at 0: on a GPU its radix passes otherwise take the count + scatter kernels only where the
    library falls back by itself (segments of 2^30 keys, too many symbols). Three of the inputs of test_bwt_round0_key_shapes; the
    reference's bytes under both settings."""
    hipapi = importlib.import_module("kanzi_amd.hipapi")
    cases = [bytes(5000), vectors.make(("text", 8000, 3)), vectors.make(("mixed", 70000, 4))]
    try:
        for data in cases:
            ok1, o1 = oracle.forward("BWT", data, len(data) + 64, "ANS0")
            assert ok1
            for knob in (0, 1):
                assert hipapi.lib().knz_hip_tune(b"rs_onesweep", knob) == 0
                ok2, o2 = hip.transform_forward("BWT", data, len(data) + 64, "ANS0")
                assert ok2 and o1 == o2, (len(data), knob)
    finally:
        hipapi.lib().knz_hip_tune(b"rs_onesweep", 1)
