"""TEXT kernels on the CPU: kanzi-cpp_amd/csrc/text.hip compiled as plain C++ against the fiber emulation in tools/hipemu, compared with
the results recorded in tests/golden/text.json (tools/make_text_golden.py). Test infrastructure only: the product runs the real kernels
(tests/test_gpu_text.py)."""
import hashlib
import json
import os
import struct
import subprocess

import pytest

import text_cases
from test_emu_kernels import build

GOLDEN = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "text.json")))
EMU_MAX = 1 << 20          # the recipes below 1 MiB


def md5(b):
    return hashlib.md5(b).hexdigest()


def run_cases(exe, tmp_path, cases, codec, block_size, order, env=None):
    """cases: (forward, cap, data type, bytes); returns (ok, data type afterwards, bytes) per case."""
    case, res = str(tmp_path / "case.bin"), str(tmp_path / "res.bin")
    with open(case, "wb") as f:
        f.write(struct.pack("<I", len(cases)))
        for fwd, cap, dt, d in cases:
            f.write(struct.pack("<IIII", fwd, cap, dt, len(d)))
            f.write(d)
    r = subprocess.run([exe, case, res, str(text_cases.ENTROPY_ID[codec]), str(block_size)], capture_output=True, text=True, timeout=1800,
                       env=dict(os.environ, HIPEMU_ORDER=order, **(env or {})))
    assert r.returncode == 0, (order, r.stdout[-2000:] + r.stderr[-2000:])
    d = open(res, "rb").read()
    o, out = 0, []
    for _ in cases:
        ok, dt, n = struct.unpack_from("<III", d, o)
        o += 12
        out.append((ok, dt, d[o:o + n]))
        o += n
    return out


@pytest.fixture(scope="module")
def blocks():
    out = {}
    for r in GOLDEN["stage"]:
        if r["recipe"][1] < EMU_MAX and r["name"] not in out:
            out[r["name"]] = text_cases.make(r["recipe"])
            assert md5(out[r["name"]]) == r["input_md5"], r["name"]
    return out


def _check(exe, tmp_path, blocks, codec, bs, order, limit=EMU_MAX, env=None):
    recs = [r for r in GOLDEN["stage"] if r["codec"] == codec and r["block_size"] == bs and r["recipe"][1] < limit]
    assert len(recs) >= 30 or limit < EMU_MAX
    fwd = run_cases(exe, tmp_path, [(1, len(blocks[r["name"]]), r["dtype"], blocks[r["name"]]) for r in recs] + [(1, 100, 0, b"")], codec, bs, order, env)
    assert fwd[-1][0] == 1 and fwd[-1][2] == b"", "an empty block passes"
    outputs = {}
    for r, (ok, dt, out) in zip(recs, fwd):
        assert ok == r["ok"], ("ok", r["name"], codec, bs, order)
        assert dt == r["dtype_out"], ("data type", r["name"], codec, bs, order)
        if r["ok"]:
            assert len(out) == r["fwd_len"] and md5(out) == r["fwd_md5"], ("forward", r["name"], codec, bs, order)
            outputs[r["name"]] = out
    assert len(outputs) >= 10
    cases = [((0, len(blocks[name]), 0, out), name) for name, out in outputs.items()]
    damaged = [r for r in GOLDEN["damaged"] if r["codec"] == codec] if bs == 0 and text_cases.DAMAGE_FROM in outputs else []
    for r in damaged:
        bad = text_cases.damage(outputs[text_cases.DAMAGE_FROM], r["op"], codec)
        assert md5(bad) == r["input_md5"], r["name"]
        cases.append(((0, r["cap"], 0, bad), r))
    got = run_cases(exe, tmp_path, [c for c, _ in cases], codec, bs, order, env)
    n_refused = 0
    for (c, what), (ok, _, out) in zip(cases, got):
        if isinstance(what, str):
            assert ok == 1 and out == blocks[what], ("round trip", what, codec, bs, order)
        else:
            assert ok == what["ok"], ("damaged", what["name"], codec, order)
            n_refused += 1 - ok
            if what["ok"]:
                assert len(out) == what["inv_len"] and md5(out) == what["inv_md5"], ("damaged", what["name"], codec, order)
    assert n_refused > 0 or not damaged


@pytest.mark.parametrize("codec", (1, 2, 3))
def test_text_every_record_emulated(tmp_path, blocks, codec):
    """Every stage record below 1 MiB in one ragged forward batch per stream block size (with an empty block), every accepted output
    and, at block size 0, every damaged record in one ragged inverse batch: the recorded verdict, bytes and data type, the input back,
    nothing written behind a capacity; workgroups dispatched in order and, at block size 0, shuffled."""
    exe = build("text_emu", tmp_path)
    for bs in text_cases.BLOCK_SIZES:
        for order in (("0", "2") if bs == 0 else ("0",)):
            _check(exe, tmp_path, blocks, codec, bs, order)


def test_text_batches_run_in_slices(tmp_path, blocks):
    """KNZ_TEXT_TABLES_MAX below the scratch of two blocks: the batches run one block at a time, with the same results."""
    exe = build("text_emu", tmp_path)
    _check(exe, tmp_path, blocks, 1, 0, "0", limit=10000, env={"KNZ_TEXT_TABLES_MAX": "1"})


def test_text_under_address_sanitizer(tmp_path, blocks):
    """The stage records up to 10,000 bytes, their round trips and the damaged records in a host build of the kernels under
    AddressSanitizer, for both encodings: the recorded results, nothing read or written out of bounds (the blocks come without slack)."""
    exe = build("text_emu", tmp_path, extra=["-fsanitize=address", "-g", "-fno-omit-frame-pointer"])
    for codec in (1, 2):
        _check(exe, tmp_path, blocks, codec, 0, "0", limit=10000)
