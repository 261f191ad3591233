"""The three LZ / LZX decoders of csrc/lz.hip on the device: the data-parallel one (k_lz_i_pparse parses a block by scans, k_lz_i_parse
takes the blocks it hands on token by token, then expand / pointer jumping / emit) and k_lz_inverse, one wave per block, which
lz_inverse() in csrc/api.hip uses alone when the 20-bytes-per-output-byte workspace cannot be had (1 GiB blocks, a 2 GiB batch, a failed
allocation, the KNZ_LZ_INV_SCRATCH_MAX budget) and which the knob lz_serial_decode selects. Its overlapping matches rest on a fence
between a wave's store and the next match's load, which no emulator of one lane at a time can show missing.

Inputs: tests/lz_decoder_cases.py. The oracle's blocks must decode to the input with the knob at 0 and at 1, in both token layouts
(bitstream versions 6 and 5), stage by stage and as a batch, whose kernel times say which decoder ran. Damaged blocks
(tests/golden/first_gen_damage.json: what the reference decides) must be accepted or refused alike by both, with the same length
and the same bytes."""
import hashlib
import importlib

import pytest

import first_gen_damage as fgd
import knzlib
import lz_decoder_cases as cases

pytestmark = pytest.mark.gpu


def lib():
    knzlib.load_pkg()
    return importlib.import_module("kanzi_amd.hipapi").lib()


@pytest.mark.parametrize("version", (6, 5))
@pytest.mark.parametrize("transform", cases.TRANSFORMS)
def test_blocks_decode_by_either_decoder(hip, oracle, transform, version):
    L = lib()
    enc = {}
    oracle.set_bs_version(version)
    try:
        for name, d in cases.blocks().items():
            ok, e = oracle.forward(transform, d, cases.forward_cap(len(d)))
            assert bool(ok) == (name != "tiny"), name
            if ok:
                enc[name] = e
                if version == 6:
                    cases.check(name, e)
        batch = cases.batch()
        rc, stream = oracle.compress(batch, transform, "NONE", cases.BATCH_BS, headerless=1)
        assert rc == 0
    finally:
        oracle.set_bs_version(6)
    if version == 6:                               # the device refuses the block below the codec's smallest too (it writes version 6 only)
        d = cases.blocks()["tiny"]
        assert hip.transform_forward(transform, d, cases.forward_cap(len(d)))[0] == 0
    p = hip.params(transform, "NONE", cases.BATCH_BS, bs_version=version)
    d_in, d_out = hip.malloc(len(stream) + 64), hip.malloc(len(batch) + cases.BATCH_BS + 64)
    hip.h2d(d_in, stream)
    try:
        for serial in (0, 1):
            assert L.knz_hip_tune(b"lz_serial_decode", serial) == 0
            for name, e in enc.items():
                d = cases.blocks()[name]
                ok, back = hip.transform_inverse(transform, e, len(d), bs_version=version)
                assert ok == 1 and back == d, (transform, version, serial, name)
            # the batch: five blocks of BATCH_BS bytes and the tiny one, which the stream carries as it is; with the timing of kernels on,
            # the names say which decoder the batch took
            hip.set_profiling(True)
            try:
                ob, eb, nb = hip.decode_blocks(p, d_in, 8 * len(stream), 0, d_out, len(batch) + cases.BATCH_BS)
                ran = {name: launches for name, ms, launches in hip.kernel_times()}
            finally:
                hip.set_profiling(False)
            assert nb == len(cases.blocks()) and hip.d2h(d_out, ob) == batch, (transform, version, serial)
            assert ran.get("k_lz_inverse", 0) > 0, ran
            assert (ran.get("k_lz_i_pparse", 0) > 0) == (serial == 0) and (ran.get("k_lz_i_emit", 0) > 0) == (serial == 0), (serial, ran)
    finally:
        L.knz_hip_tune(b"lz_serial_decode", 0)
        hip.free(d_in); hip.free(d_out)


@pytest.mark.parametrize("name", [n for n in cases.blocks() if n != "tiny"])
@pytest.mark.parametrize("transform", cases.TRANSFORMS)
def test_damaged_blocks_are_decided_as_the_reference_decides(hip, oracle, transform, name):
    """One to three bytes flipped or overwritten in one of the header's fields, the literals, the tokens or the length extensions, and the
    headers k_lz_i_pparse hands on to k_lz_i_parse by its own checks (no tokens, literals that end inside the header, distances a byte past
    the block), into destinations of n and n + 64 bytes: the data-parallel decoder and the one-wave one give the reference's decision and
    length, and its bytes where it accepts. (The distances are left alone, and a case in which the reference reads further behind the
    block than the two bytes it asks for is not in the fixture: its answer is not defined there.)"""
    L = lib()
    recs = [r for r in fgd.load()[0] if r["stage"] == "LZ" and r["transform"] == transform and r["input"][1] == name]
    assert len(recs) >= 40 and {r["cap"] - len(cases.blocks()[name]) for r in recs} == {0, 64}
    assert {"nTok=0", "litEnd=12", "nDist+1"} <= {r["case"] for r in recs}
    try:
        for serial in (0, 1):
            assert L.knz_hip_tune(b"lz_serial_decode", serial) == 0
            for r in recs:
                ok, out = hip.transform_inverse(transform, fgd.block(oracle, r), r["cap"])
                assert ok == r["ok"], (serial, r)
                if ok:
                    assert len(out) == r["len"], (serial, r)
                    if r["md5"] is not None:
                        assert hashlib.md5(out).hexdigest() == r["md5"], (serial, r)
    finally:
        L.knz_hip_tune(b"lz_serial_decode", 0)
