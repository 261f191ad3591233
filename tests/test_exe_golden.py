"""tests/golden/exe.json against the reference and against what the EXE tests need from it (CPU only). The file is written by
tools/make_exe_golden.py from the reference build in oracle/_ref; where that build exists every record is derived again and compared."""
import importlib.util
import json
import os

import pytest

import exe_cases
import knzlib

GOLDEN = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "exe.json")))


def test_golden_file_holds_what_the_tests_need():
    """Every stage case of exe_cases.STAGE in order, the verdicts of exe_cases.REQUIRED, every whole record accepted and given back, some
    damaged record refused, both special damages present, a first refused count of ARM64 escape pairs, and no input bytes."""
    recs = GOLDEN["stage"]
    assert [(r["recipe"], r["dtype"], r["name"]) for r in recs] == [(json.loads(json.dumps(r)), dt, name) for r, dt, name in exe_cases.STAGE]
    by_name = {r["name"]: r for r in recs}
    for name, (ok, dt) in exe_cases.REQUIRED.items():
        assert (by_name[name]["ok"], by_name[name]["dtype_out"]) == (ok, dt), name
    for r in recs:
        assert r["cap"] == exe_cases.max_encoded(r["recipe"][1])
        assert set(r) <= {"name", "recipe", "dtype", "input_md5", "cap", "ok", "dtype_out", "fwd_len", "fwd_md5", "mode", "inv_md5", "lossless"}
        if r["ok"]:
            assert r["dtype_out"] == exe_cases.EXE and 9 <= r["fwd_len"] - r["recipe"][1] <= r["recipe"][1] // 50
            assert r["lossless"] or r["name"] == "elf64 arm codeStart 4098"
    assert {by_name[n]["mode"] for n in exe_cases.DAMAGE_FROM} == {0x40, 0x20}
    below = [by_name[n] for _, _, n in exe_cases.STAGE if n.endswith("below 0")]
    assert below[0]["ok"] and not below[-1]["ok"]
    damaged = GOLDEN["damaged"]
    assert all(r["ok"] for r in damaged if r["op"] == "whole") and any(not r["ok"] for r in damaged)
    assert {"escend", "armhalf"} <= {r["op"] for r in damaged}
    for name in exe_cases.DAMAGE_FROM:
        assert {r["op"] for r in damaged if r["stage"] == name} >= set(exe_cases.DAMAGE) - {"escend", "armhalf", "cutprefix"}
    assert [(r["chain"], r["entropy"], r["checksum"]) for r in GOLDEN["streams"]] == [tuple(c) for c in exe_cases.STREAM_CHAINS]
    assert [r["jobs"] for r in GOLDEN["hosted"]] == [1, 3] * len(exe_cases.HOSTED)
    assert os.path.getsize(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "exe.json")) < 100000


def test_golden_file_is_what_the_reference_gives():
    """Every record derived again from the reference (tools/make_exe_golden.py, which also asserts the required verdicts)."""
    if knzlib.ensure_ref() is None:
        pytest.skip("the reference build is not available (oracle/_ref: build() makes it where the reference's sources exist)")
    spec = importlib.util.spec_from_file_location("make_exe_golden", os.path.join(knzlib.ROOT, "tools", "make_exe_golden.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    assert tool.build_golden(log=lambda *a: None) == GOLDEN
