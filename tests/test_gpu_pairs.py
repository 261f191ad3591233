"""Every ordered pair of the 14 device transforms through the code the stages share (api.hip, sequence.hip: the buffer stride and the
capacities a stage receives in second position, the skip-flag byte, the data type a stage leaves for the one behind it, the per-lane
scratch of the decode ranges): 196 chains over one input of nine blocks of 16 KiB and a copy block, in front of NONE (pass A) and in
front of a rotation of the eight coders, the checksum widths and three job counts (pass B). Expected lengths and digests are the
reference's, from tests/golden/pairs.json (tools/make_pair_golden.py, pinned by tests/test_pair_golden.py); the input makes every stage
that can refuse a block both take and refuse some. One test per first stage."""
import hashlib
import importlib
import json
import os
import time

import pytest

import knzlib
import pair_cases as cases

pytestmark = pytest.mark.gpu

GOLDEN = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pairs.json")))
KNZ_ERR_INVALID_CODEC = 3            # include/knz_hip.h
_data = []
_ref = []


def md5(b):
    return hashlib.md5(b).hexdigest()


def data():
    if not _data:
        d = cases.make_input()
        assert md5(d) == GOLDEN["input_md5"] and len(d) == GOLDEN["n"]
        _data.append(d)
    return _data[0]


def reference():
    """The reference build, for the streams the device refuses to write. Its absence is a failure, not a skip."""
    if not _ref:
        _ref.append(knzlib.Ref())
    return _ref[0]


def encode(hip, d, rec):
    framing = importlib.import_module("kanzi_amd.framing")
    hipapi = importlib.import_module("kanzi_amd.hipapi")
    p = hip.params(rec["chain"], rec["entropy"], cases.BS, rec["checksum"], jobs=rec["jobs"])
    hdr, hb = framing.make_header(p.entropy_type, p.transform_type, cases.BS, rec["checksum"], len(d))
    cap = hip.encode_bound(p, len(d)) + 64
    if p.entropy_type in hipapi.BINARY_CODERS:
        cap += 32 * len(d)                  # knz_hip_encode_bound is these coders' first tier (include/knz_hip.h)
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


def one_pair(hip, L, d, ps, i, j, rec):
    hipapi = importlib.import_module("kanzi_amd.hipapi")
    what = (ps, rec["chain"], rec["entropy"], rec["checksum"], rec["jobs"])
    if cases.refused_when_encoding(i, j):
        # the device LZ stages do not read the data type the first stage leaves, so the chain is refused rather than written differently
        # from the reference; the decoder needs no data type (the minimum match is in the block) and must read the reference's stream
        with pytest.raises(hipapi.KnzError) as ex:
            encode(hip, d, rec)
        assert ex.value.code == KNZ_ERR_INVALID_CODEC, what
        rc, enc = reference().compress(d, rec["chain"], rec["entropy"], cases.BS, jobs=rec["jobs"], checksum=rec["checksum"], orig_size=len(d))
        assert rc == 0, what
        hb = rec["header_bits"]
    else:
        enc, hb = encode(hip, d, rec)
        assert hb == rec["header_bits"], what
    assert (len(enc), md5(enc)) == (rec["knz_len"], rec["knz_md5"]), what
    for parts in (3, 1) if ps == "A" else (3,):
        assert L.knz_hip_tune(b"dec_parts", parts) == 0
        assert decode(hip, enc, rec, hb, len(d)) == d, what + (parts,)


@pytest.mark.parametrize("first", cases.T)
def test_every_second_stage_behind(hip, first):
    """`first` in front of each of the 14 stages, both passes: the device writes the reference's stream (for {PACK, MM, UTF, ROLZX} +
    {LZ, LZX} it refuses to, with the invalid-codec code, and is given the reference's) and reads it back as three block ranges, in
    pass A also as one. Cases the fixture leaves out (the reference cannot read, or does not repeat, its own stream) are not run.
    Afterwards the context still round-trips the headline chain."""
    L = importlib.import_module("kanzi_amd.hipapi").lib()
    d, i = data(), cases.T.index(first)
    try:
        for ps in cases.PASSES:
            recs = cases.records(GOLDEN, ps)
            t0, compared = time.time(), 0
            for j in range(14):
                rec = recs[14 * i + j]
                if "left_out" in rec:
                    continue
                one_pair(hip, L, d, ps, i, j, rec)
                compared += 1
            print("%s+*: pass %s, %d cases, %.2f s" % (first, ps, compared, time.time() - t0))
            assert compared >= 13, (first, ps, compared)
    finally:
        L.knz_hip_tune(b"dec_parts", 3)
    rec = {"chain": "BWT+MTFT+ZRLT", "entropy": "ANS0", "checksum": 0, "jobs": 1}
    enc, hb = encode(hip, d, rec)
    assert decode(hip, enc, rec, hb, len(d)) == d
