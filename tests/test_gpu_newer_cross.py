"""BWTS, PACK, MM, LZP, RANGE and CM across the paths that cut through all stages: decoding a batch as one, two or three block ranges,
sharded encoding and decoding, and damaged streams. Four chains over one input of 17 blocks of 16 KiB and a tail; expected lengths,
digests and the reference's verdicts on the damaged streams come from tests/golden/newer_cross.json (tools/make_newer_cross_golden.py)."""
import hashlib
import importlib
import json
import os

import pytest

import knzlib
import newer_cross_cases as cases

pytestmark = pytest.mark.gpu

GOLDEN = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "newer_cross.json")))
IDS = ["%s-%s" % (c[0], c[1]) for c in cases.CHAINS]
_data = []


def md5(b):
    return hashlib.md5(b).hexdigest()


def data():
    if not _data:
        d = cases.make_input()
        assert md5(d) == GOLDEN["input_md5"] and len(d) == GOLDEN["n"]
        _data.append(d)
    return _data[0]


def record(idx):
    rec = GOLDEN["chains"][idx]
    assert (rec["chain"], rec["entropy"], rec["checksum"], rec["jobs"]) == cases.CHAINS[idx]
    return rec


def encode(hip, d, rec):
    framing = importlib.import_module("kanzi_amd.framing")
    hipapi = importlib.import_module("kanzi_amd.hipapi")
    p = hip.params(rec["chain"], rec["entropy"], cases.BS, rec["checksum"], jobs=rec["jobs"])
    hdr, hb = framing.make_header(p.entropy_type, p.transform_type, cases.BS, rec["checksum"], len(d))
    cap = hip.encode_bound(p, len(d)) + 64
    if p.entropy_type == hipapi.E_CM:
        cap += 32 * len(d)                  # knz_hip_encode_bound is CM's first tier (include/knz_hip.h)
    d_in, d_out = hip.malloc(len(d) + 64), hip.malloc(cap)
    try:
        hip.h2d(d_in, d)
        bits = hip.encode_blocks(p, d_in, len(d), d_out, cap, prologue=hdr, prologue_bits=hb)
        return hip.d2h(d_out, (bits + 7) // 8), hb
    finally:
        hip.free(d_in)
        hip.free(d_out)


def decode(hip, enc, rec, start_bit, n):
    p = hip.params(rec["chain"], rec["entropy"], cases.BS, rec["checksum"], jobs=rec["jobs"])
    d_in, d_out = hip.malloc(len(enc) + 4096), hip.malloc(n + 2 * cases.BS + 64)
    try:
        hip.h2d(d_in, enc + bytes(64))
        ob, _, _ = hip.decode_blocks(p, d_in, 8 * len(enc), start_bit, d_out, n + cases.BS)
        return hip.d2h(d_out, ob)
    finally:
        hip.free(d_in)
        hip.free(d_out)


@pytest.mark.parametrize("idx", range(len(cases.CHAINS)), ids=IDS)
def test_decode_in_ranges(hip, idx):
    """The stream is the reference's, and decoding it as one, two and three block ranges side by side (knob dec_parts: every range a
    smaller decode with workspaces of its own, the per-lane scratch of PACK, MM and LZP among them) gives the input back each time."""
    L = importlib.import_module("kanzi_amd.hipapi").lib()
    rec, d = record(idx), data()
    enc, hb = encode(hip, d, rec)
    assert hb == rec["header_bits"] and len(enc) == rec["knz_len"] and md5(enc) == rec["knz_md5"]
    try:
        for parts in (1, 2, 3):
            assert L.knz_hip_tune(b"dec_parts", parts) == 0
            assert decode(hip, enc, rec, hb, len(d)) == d, parts
    finally:
        L.knz_hip_tune(b"dec_parts", 3)


def _sharded(rec, d):
    sh = importlib.import_module("kanzi_amd.sharded")
    enc = sh.DeviceRunEncoder(0, rec["chain"], rec["entropy"], cases.BS, jobs=rec["jobs"], orig_size=len(d), checksum=rec["checksum"])
    runs = []
    for r, (first, cnt) in enumerate(sh.block_ranges(len(d), cases.BS, 2)):
        assert cnt > 0 and (r == 0) == (first == 0)
        runs.append(enc(d[first * cases.BS:min(len(d), (first + cnt) * cases.BS)], first, r == 0, r == 1))
    got = sh.concat_bit_runs(runs)[0]
    assert len(got) == rec["knz_len"] and md5(got) == rec["knz_md5"]
    dec = sh.DeviceRunDecoder(0, jobs=rec["jobs"])
    world = 3
    parts = [None] * world
    for r in range(world):
        def gather(obj, r=r):
            parts[r] = obj
            return None
        sh.decompress_sharded(got, r, world, dec, gather)
    assert b"".join(parts) == d


@pytest.mark.parametrize("idx", range(len(cases.CHAINS)), ids=IDS)
def test_sharded_runs_and_ranges(hip, idx):
    """Two block ranges encoded as runs of their own (the second with its first block's id and the chain's jobs), concatenated on the host:
    the reference's whole stream; decoded as three ranks' ranges: the input."""
    _sharded(record(idx), data())


def test_sharded_cm_with_the_first_tier_lowered(hip, monkeypatch):
    """The CM chain again with KNZ_CM_TIER1_DIV=4 (tests/test_gpu_cm.py::test_second_tier_with_the_first_lowered): the run encoder's first
    staging of n / 4 is too small for the blocks of random bytes, so it takes its second tier, and the stream is still the reference's."""
    monkeypatch.setenv("KNZ_CM_TIER1_DIV", "4")
    idx = [c[1] for c in cases.CHAINS].index("CM")
    _sharded(record(idx), data())


@pytest.mark.parametrize("idx", range(len(cases.CHAINS)), ids=IDS)
def test_damaged_streams_get_the_reference_verdict(hip, idx):
    """Six seeded damaged copies of the reference's stream (byte flips, a 64-byte overwritten range, a cut; the header stays): the device
    raises KnzError or returns, and it may return only where the reference's decompressor accepted the same bytes, and then the
    same output. The context still round-trips afterwards."""
    hipapi = importlib.import_module("kanzi_amd.hipapi")
    rec, d = record(idx), data()
    enc, hb = encode(hip, d, rec)
    assert md5(enc) == rec["knz_md5"]
    for v, want in enumerate(rec["damaged"]):
        bad = cases.damage(enc, (hb + 7) // 8, idx, v)
        assert want["variant"] == v and len(bad) == want["input_len"] and md5(bad) == want["input_md5"]
        try:
            out = decode(hip, bad, rec, hb, len(d))
        except hipapi.KnzError:
            continue
        assert want["accepted"], ("the reference refuses this stream", rec["chain"], v)
        assert len(out) == want["out_len"] and md5(out) == want["out_md5"], (rec["chain"], v)
    assert decode(hip, enc, rec, hb, len(d)) == d
