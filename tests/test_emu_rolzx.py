"""ROLZX kernels on the CPU: kanzi-cpp_amd/csrc/rolzx.hip compiled as plain C++ against the fiber emulation in tools/hipemu, compared
with the records of tests/golden/rolzx.json (tools/make_rolzx_golden.py: the model's results, pinned to the reference by
tests/test_rolzx_model.py). Test infrastructure only: the product runs the real kernels (tests/test_gpu_rolzx.py)."""
import hashlib
import json
import os

import rolzx_cases
from test_emu_kernels import build
from test_emu_mm import run_cases

GOLDEN = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rolzx.json")))
TABLES = 8667136           # bytes of tables per block that runs at once (rolzx.hip)


def md5(b):
    return hashlib.md5(b).hexdigest()


def _stage_cases():
    recs = GOLDEN["stage"]
    blocks = [rolzx_cases.make(r["recipe"]) for r in recs]
    for r, b in zip(recs, blocks):
        assert md5(b) == r["input_md5"], r["recipe"]
    return recs, blocks


def _damaged_cases(outputs):
    cases = []
    for r in GOLDEN["damaged"]:
        d = rolzx_cases.damage(outputs[json.dumps(r["recipe"])], r["op"])
        assert md5(d) == r["input_md5"], (r["recipe"], r["op"])
        cases.append((0, r["cap"], 0, d))
    return cases


def _check_damaged(got):
    for r, (ok, _, out) in zip(GOLDEN["damaged"], got):
        assert ok == r["ok"], ("inverse ok", r["recipe"][:3], r["op"], r["cap"])
        if r["ok"]:
            assert md5(out) == r["inv_md5"], ("inverse bytes", r["recipe"][:3], r["op"], r["cap"])


def test_rolzx_every_record_emulated(tmp_path, monkeypatch):
    """Every stage record (preset types included, and one with a destination one byte below the bound) in one ragged forward batch, the
    inverse of every accepted output and every cut and damaged record in one ragged inverse batch, the tables limited to 5 blocks at a
    time so that the batches run in slices: the recorded verdict, bytes and data type, nothing written behind a capacity; workgroups
    dispatched in order and shuffled."""
    monkeypatch.setenv("KNZ_ROLZX_TABLES_MAX", str(5 * TABLES))
    recs, blocks = _stage_cases()
    short = rolzx_cases.make(rolzx_cases.SHORT_CAP)
    exe = build("rolzx_emu", tmp_path)
    for order in ("0", "2"):
        fwd = run_cases(exe, tmp_path, [(1, r["cap"], r["dtype_in"], b) for r, b in zip(recs, blocks)]
                        + [(1, rolzx_cases.max_encoded(len(short)) - 1, 0, short)], order)
        assert fwd[-1][0] == 0, "a destination below getMaxEncodedLength is refused (ROLZCodec.cpp:916)"
        outputs, cases, want = {}, [], []
        for r, b, (ok, dt, out) in zip(recs, blocks, fwd):
            if len(b) == 0:
                continue                                     # (takes no part in a batch)
            assert ok == r["ok"], ("ok", r["recipe"][:3], r["dtype_in"], order)
            assert dt == r["dtype_out"], ("data type", r["recipe"][:3], r["dtype_in"], order)
            if r["ok"]:
                assert len(out) == r["fwd_len"] and md5(out) == r["fwd_md5"], ("forward", r["recipe"][:3], r["dtype_in"], order)
                if r["dtype_in"] == 0:
                    outputs[json.dumps(r["recipe"])] = out
                cases.append((0, len(b), 0, out))
                want.append(b)
        got = run_cases(exe, tmp_path, cases + _damaged_cases(outputs), order)
        for b, (ok, _, out) in zip(want, got):
            assert ok and out == b, ("round trip", len(b), order)
        _check_damaged(got[len(want):])


def test_rolzx_damaged_input_and_block_ends_under_address_sanitizer(tmp_path, monkeypatch):
    """The cut and damaged inverse records, and the forward of the records that end inside a match or in the tail, in a host build of
    the kernels under AddressSanitizer, as a program of its own: the recorded verdict, nothing read or written out of bounds."""
    monkeypatch.setenv("KNZ_ROLZX_TABLES_MAX", str(5 * TABLES))
    exe = build("rolzx_emu", tmp_path, extra=["-fsanitize=address", "-g", "-fno-omit-frame-pointer"])
    recs = [r for r in GOLDEN["stage"] if r["ok"] and r["dtype_in"] == 0 and 0 < r["recipe"][1] <= 5000]
    fwd = run_cases(exe, tmp_path, [(1, r["cap"], 0, rolzx_cases.make(r["recipe"])) for r in recs], "0")
    outputs = {}
    for r, (ok, _, out) in zip(recs, fwd):
        assert ok and md5(out) == r["fwd_md5"], r["recipe"][:3]
        outputs[json.dumps(r["recipe"])] = out
    _check_damaged(run_cases(exe, tmp_path, _damaged_cases(outputs), "2"))
