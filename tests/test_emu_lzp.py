"""LZP kernels on the CPU: kanzi-cpp_amd/csrc/lzp.hip compiled as plain C++ against the fiber emulation in tools/hipemu, compared with
the reference's results recorded in tests/golden/lzp.json (tools/make_lzp_golden.py). Test infrastructure only: the product runs the
real kernels (tests/test_gpu_lzp.py)."""
import hashlib
import json
import os

import lzp_cases
from test_emu_kernels import build
from test_emu_mm import run_cases

GOLDEN = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lzp.json")))


def md5(b):
    return hashlib.md5(b).hexdigest()


def test_lzp_every_record_emulated(tmp_path):
    """Every stage record (and one with a destination one byte below the bound) in one ragged forward batch, every inverse and cut record
    and the inverse of every accepted output in one ragged inverse batch: the reference's verdict and bytes, nothing written behind a
    capacity; workgroups dispatched in order and shuffled."""
    recs = GOLDEN["stage"]
    blocks = [lzp_cases.make(r["recipe"]) for r in recs]
    for r, b in zip(recs, blocks):
        assert md5(b) == r["input_md5"], r["recipe"]
    short = lzp_cases.make(lzp_cases.SHORT_CAP)
    exe = build("lzp_emu", tmp_path)
    for order in ("0", "2"):
        fwd = run_cases(exe, tmp_path, [(1, r["cap"], 0, b) for r, b in zip(recs, blocks)]
                        + [(1, lzp_cases.max_encoded(len(short)) - 1, 0, short)], order)
        assert fwd[-1][0] == 0, "a destination below getMaxEncodedLength is refused (LZCodec.cpp:788)"
        outputs = {}
        for r, b, (ok, _, out) in zip(recs, blocks, fwd):
            if len(b) == 0:
                continue                                     # (takes no part in a batch)
            assert ok == r["ok"], ("ok", r["recipe"], order)
            if r["ok"]:
                assert len(out) == r["fwd_len"] and md5(out) == r["fwd_md5"], ("forward", r["recipe"], order)
                outputs[json.dumps(r["recipe"])] = (out, b)
        cases, want = [], []
        for out, b in outputs.values():
            cases.append((0, len(b), 0, out))
            want.append((1, md5(b)))
        for r in GOLDEN["inverse"] + GOLDEN["cut"]:
            d = outputs[json.dumps(r["recipe"])][0][:r["cut"]] if "cut" in r else lzp_cases.make(r["recipe"])
            assert md5(d) == r["input_md5"], r["recipe"]
            cases.append((0, r["cap"], 0, d))
            want.append((r["ok"], r["inv_md5"]))
        got = run_cases(exe, tmp_path, cases, order)
        for (c, (wok, wmd5), (ok, _, out)) in zip(cases, want, got):
            assert ok == wok, ("inverse ok", len(c[3]), c[1], order)
            if wok:
                assert md5(out) == wmd5, ("inverse bytes", len(c[3]), c[1], order)


def test_lzp_damaged_inverse_input_under_address_sanitizer(tmp_path):
    """The inverse and cut records, and the forward of the records that end in a match or in the tail loop, in a host build of the kernels
    under AddressSanitizer: the reference's verdict, nothing read or written out of bounds."""
    exe = build("lzp_emu", tmp_path, extra=["-fsanitize=address", "-g", "-fno-omit-frame-pointer"])
    recs = [r for r in GOLDEN["stage"] if r["ok"] and len(lzp_cases.make(r["recipe"])) < 70000]
    fwd = run_cases(exe, tmp_path, [(1, r["cap"], 0, lzp_cases.make(r["recipe"])) for r in recs], "0")
    outputs = {json.dumps(r["recipe"]): out for r, (ok, _, out) in zip(recs, fwd) if ok}
    assert len(outputs) == len(recs)
    cases, want = [], []
    for r in GOLDEN["inverse"] + GOLDEN["cut"]:
        d = outputs[json.dumps(r["recipe"])][:r["cut"]] if "cut" in r else lzp_cases.make(r["recipe"])
        assert md5(d) == r["input_md5"], r["recipe"]
        cases.append((0, r["cap"], 0, d))
        want.append(r)
    got = run_cases(exe, tmp_path, cases, "2")
    for r, (ok, _, out) in zip(want, got):
        assert ok == r["ok"], ("ok", r["recipe"], r["cap"], r.get("where"))
        if r["ok"]:
            assert md5(out) == r["inv_md5"], ("inverse", r["recipe"], r["cap"])
