"""tests/rolzx_model.py -- ROLZX restated in plain Python -- pinned to the reference: the reference's per-stage entry point does not reach
ROLZCodec2, so the model's stage output is looked for, as a bit string, in the file `kanzi -c -t ROLZX -e NONE` writes (the block header
is not byte-aligned). The records of tests/golden/rolzx.json are the model's, and the paths the fixture takes are checked here."""
import collections
import hashlib
import json
import os
import subprocess

import pytest

import knzlib
import rolzx_cases
import rolzx_model

GOLDEN = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rolzx.json")))


def md5(b):
    return hashlib.md5(b).hexdigest()


def bits(b):
    return "".join(format(x, "08b") for x in b)


def test_model_output_is_in_the_reference_stream_and_decodes(tmp_path):
    """Every small recipe the stage accepts with the type a stream gives it (EXE behind the ELF magic, none otherwise): the model's
    forward output is in the reference's stream, and the model's inverse gives the input back."""
    if not os.path.exists(knzlib.REF_BIN):
        pytest.skip("the reference's command-line tool is not built (oracle/_ref/kanzi)")
    src, knz = str(tmp_path / "in.bin"), str(tmp_path / "out.knz")
    n = 0
    for r in rolzx_cases.STAGE:
        d = rolzx_cases.make(r)
        ok, out, _, _ = rolzx_model.forward(d, rolzx_cases.max_encoded(len(d)), 3 if r[0] == "elf" else 0)
        if not ok or not d:
            continue
        open(src, "wb").write(d)
        p = subprocess.run([knzlib.REF_BIN, "-c", "-i", src, "-o", knz, "-f", "-t", "ROLZX", "-e", "NONE", "-j", "1"], capture_output=True, text=True, timeout=120)
        assert p.returncode == 0, p.stdout + p.stderr
        assert bits(out) in bits(open(knz, "rb").read()), r
        iok, back, _ = rolzx_model.inverse(out, len(d))
        assert iok and back == d, r
        n += 1
    assert n >= 25


def test_model_reproduces_every_record_and_the_fixture_takes_every_path():
    fwd_paths, inv_paths = collections.Counter(), collections.Counter()
    outputs = {}
    for rec in GOLDEN["stage"]:
        d = rolzx_cases.make(rec["recipe"])
        assert md5(d) == rec["input_md5"], rec["recipe"]
        ok, out, dt, paths = rolzx_model.forward(d, rec["cap"], rec["dtype_in"])
        fwd_paths.update(paths.keys())
        assert int(ok) == rec["ok"] and dt == rec["dtype_out"], rec["recipe"]
        if ok and d:
            assert len(out) == rec["fwd_len"] and md5(out) == rec["fwd_md5"], rec["recipe"]
            if rec["dtype_in"] == 0:
                outputs[json.dumps(rec["recipe"])] = out
    d = rolzx_cases.make(rolzx_cases.SHORT_CAP)
    assert not rolzx_model.forward(d, rolzx_cases.max_encoded(len(d)) - 1)[0] and rolzx_model.forward(d, rolzx_cases.max_encoded(len(d)))[0]
    n_refused = 0
    for rec in GOLDEN["damaged"]:
        bad = rolzx_cases.damage(outputs[json.dumps(rec["recipe"])], rec["op"])
        assert md5(bad) == rec["input_md5"], (rec["recipe"], rec["op"])
        ok, out, paths = rolzx_model.inverse(bad, rec["cap"])
        inv_paths.update(paths.keys())
        assert int(ok) == rec["ok"], (rec["recipe"], rec["op"])
        assert ok or rec["op"][0] != "whole"
        n_refused += 0 if ok else 1
        if ok:
            assert md5(out) == rec["inv_md5"], (rec["recipe"], rec["op"])
    assert n_refused > 0
    want_fwd = ["refuse_early", "refuse_output_reaches_count", "dna", "exe", "no_room_for_a_match", "zero_entry_is_a_candidate",
                "length_overshoots", "equal_length_newer_stays", "scan_ends_at_exact_length", "longer_candidate_behind_exact",
                "counter_wraps", "match_of_min_match", "match_of_maximum", "match_index_nonzero", "below_min_match_6"]
    assert [p for p in want_fwd if p not in fwd_paths] == []
    want_inv = ["literal", "match", "copy_overlaps", "refuse_length_field", "refuse_short_read", "refuse_match_among_first_literals",
                "refuse_sanity_check", "refuse_input_not_used_up"]
    assert [p for p in want_inv if p not in inv_paths] == []
    assert "refuse_write_outside" not in inv_paths, "no record may rely on the reference writing outside its buffers"


def test_zero_entry_record_matches_position_zero():
    """The record built for it: a position whose hash32 is 0 while its key's ring holds only zero entries is coded as a match with
    position 0 (a kernel that took zero for `empty` would code literals)."""
    d = rolzx_cases.make(rolzx_cases._zero_entry())
    at = d.index(bytes.fromhex("f8f9")) + 2
    assert rolzx_model.hash32(d, at) == 0 and d[at:at + 13] == d[:13]
    _, out, _, _ = rolzx_model.forward(d, rolzx_cases.max_encoded(len(d)))
    alt = bytearray(d)
    alt[0] ^= 1                                   # position 0 no longer agrees: literals instead
    _, out2, _, _ = rolzx_model.forward(bytes(alt), rolzx_cases.max_encoded(len(d)))
    assert len(out) < len(out2)
