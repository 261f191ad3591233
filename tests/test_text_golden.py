"""tests/golden/text.json against the host code, against the reference and against what the TEXT tests need from it (CPU only). The
file is written by tools/make_text_golden.py; where the reference build exists (oracle/_ref) every record is derived again and compared."""
import importlib.util
import json
import os

import pytest

import knzlib
import text_cases

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "text.json")
GOLDEN = json.load(open(PATH))


def _tool():
    spec = importlib.util.spec_from_file_location("make_text_golden", os.path.join(knzlib.ROOT, "tools", "make_text_golden.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    return tool


def test_golden_file_holds_what_the_tests_need():
    """Every case for the three codecs and the three block sizes, in order; the verdicts the cases are there for; some block refused
    midway; indexes of every length; damaged records refused; no input bytes."""
    recs = GOLDEN["stage"]
    want = [(name, json.loads(json.dumps(r)), dt, codec, bs) for name, r, dt in text_cases.stage_cases() for codec in (1, 2, 3)
            for bs in text_cases.BLOCK_SIZES]
    assert [(r["name"], r["recipe"], r["dtype"], r["codec"], r["block_size"]) for r in recs] == want
    by = {(r["name"], r["codec"], r["block_size"]): r for r in recs}
    for codec in (1, 2, 3):
        for bs in text_cases.BLOCK_SIZES:
            assert not by[("plain 1023", codec, bs)]["ok"] and by[("plain 1024", codec, bs)]["ok"]
            assert by[("magic", codec, bs)]["ok"] == (codec != 2)
            assert (by[("overflow", codec, bs)]["ok"], by[("overflow", codec, bs)]["dtype_out"]) == (0, 1), "text, refused midway"
            for name in ("distinct words 128 KiB", "three letters behind 16384 entries", "wrap 4 MiB", "crlf", "xml", "escape bytes", "word lengths"):
                assert by[(name, codec, bs)]["ok"], name
            for dt in (2, 3, 4, 5, 6, 8, 9):
                assert (by[("preset %d" % dt, codec, bs)]["ok"], by[("preset %d" % dt, codec, bs)]["dtype_out"]) == (0, dt)
            for dt in (1, 7):
                assert (by[("preset %d" % dt, codec, bs)]["ok"], by[("preset %d" % dt, codec, bs)]["dtype_out"]) == (1, 1)
    verdicts = {r["dtype_out"] for r in recs if not r["ok"] and r["dtype"] == 0 and r["codec"] == 2}
    assert verdicts >= {0, 4, 5, 6, 7, 8, 9}, "UNDEFINED, NUMERIC, BASE64, DNA, BIN, UTF8 and SMALL_ALPHABET"
    assert {r["source"] for r in recs if r["block_size"] == 0 and (r["dtype"] == 0 or r["codec"] == 1)} == {"ref"}
    damaged = GOLDEN["damaged"]
    for codec in (1, 2, 3):
        names = [r["name"] for r in damaged if r["codec"] == codec]
        assert names == [n for n, _ in text_cases.damaged_cases(codec)] + ["whole", "capacity one short", "capacity 100 short"]
    assert all(r["ok"] == (r["name"] == "whole") for r in damaged)
    assert [(r["chain"], r["entropy"], r["checksum"]) for r in GOLDEN["streams"]] == [tuple(c) for c in text_cases.STREAM_CHAINS]
    assert [(r["chain"], r["entropy"], r["checksum"]) for r in GOLDEN["mixed"]] == [tuple(c) for c in text_cases.MIXED_CHAINS]
    assert [(r["chain"], r["entropy"], r["checksum"]) for r in GOLDEN["dna"]] == [tuple(c) for c in text_cases.DNA_CHAINS]
    assert [(r["chain"], r["entropy"], r["block_size"]) for r in GOLDEN["big"]] == [(c, e, text_cases.BIG_BS) for c, e, _ in text_cases.BIG_CHAINS]
    assert [r["level"] for r in GOLDEN["cli"]] == text_cases.CLI_LEVELS
    assert os.path.getsize(PATH) < 200000


def test_golden_file_is_what_the_host_code_gives():
    """Every stage and damaged record derived again from knz_host_text_forward / _inverse (which tests/test_host_text_utf.py pins to the
    reference)."""
    tool = _tool()
    host = tool.Host()
    stage, outputs = tool.stage_records(host, None, log=lambda *a: None)
    strip = lambda recs: [{k: v for k, v in r.items() if k != "source"} for r in recs]
    assert strip(json.loads(json.dumps(stage))) == strip(GOLDEN["stage"])
    assert json.loads(json.dumps(tool.damaged_records(host, outputs))) == GOLDEN["damaged"]


def test_golden_file_is_what_the_reference_gives():
    """Every record derived again with the reference at hand (tools/make_text_golden.py asserts that the reference and the host code agree
    wherever the reference's harness can be asked)."""
    if knzlib.ensure_ref() is None:
        pytest.skip("the reference build is not available (oracle/_ref: build() makes it where the reference's sources exist)")
    assert _tool().build_golden(log=lambda *a: None) == GOLDEN
