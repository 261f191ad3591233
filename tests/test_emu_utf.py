"""UTF kernels on the CPU: kanzi-cpp_amd/csrc/utf.hip compiled as plain C++ against the fiber emulation in tools/hipemu, compared with
the reference's results recorded in tests/golden/utf.json (tools/make_utf_golden.py). Test infrastructure only: the product runs the
real kernels (tests/test_gpu_utf.py)."""
import hashlib
import json
import os

import utf_cases
from test_emu_kernels import build
from test_emu_mm import run_cases

GOLDEN = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "utf.json")))


def md5(b):
    return hashlib.md5(b).hexdigest()


def _blocks(recs):
    blocks = [utf_cases.make(r["recipe"]) for r in recs]
    for r, b in zip(recs, blocks):
        assert md5(b) == r["input_md5"], r["recipe"]
    return blocks


def inverse_cases(outputs):
    """(case, expected record) of every inverse and damaged record; outputs: the forward output by stage index (records of stages that
    are not in it are left out)."""
    cases = []
    for r in GOLDEN["inverse"] + GOLDEN["damaged"]:
        if "stage" in r and r["stage"] not in outputs:
            continue
        if "op" in r:
            d = utf_cases.damage(outputs[r["stage"]], r["op"])
        elif "stage" in r:
            d = outputs[r["stage"]]
        else:
            d = utf_cases.make(r["recipe"])
        assert md5(d) == r["input_md5"], r
        cases.append(((0, r["cap"], 0, d), r))
    return cases


def check_inverse(cases, got, order):
    n_ok = 0
    for ((_, cap, _, d), r), (ok, _, out) in zip(cases, got):
        assert ok == r["ok"], ("inverse ok", r.get("stage"), r.get("op"), r.get("recipe"), cap, order)
        if r["ok"]:
            n_ok += 1
            assert len(out) == r["inv_len"] and md5(out) == r["inv_md5"], ("inverse bytes", r.get("stage"), r.get("op"), cap, order)
    assert 3 * n_ok >= len(cases)


def test_utf_every_record_emulated(tmp_path):
    """Every stage record with its data type in one ragged forward batch (and one block with a destination one byte below the bound, one at
    the bound), every inverse and damaged record in one ragged inverse batch: the reference's verdict, bytes and data type, nothing
    written behind a capacity; workgroups dispatched in order and shuffled."""
    recs = GOLDEN["stage"]
    blocks = _blocks(recs)
    capd = utf_cases.make(utf_cases.CAP_CASE)
    exe = build("utf_emu", tmp_path)
    for order in ("0", "2"):
        fwd = run_cases(exe, tmp_path, [(1, r["cap"], r["dtype"], b) for r, b in zip(recs, blocks)]
                        + [(1, len(capd) + 8191, 0, capd), (1, len(capd) + 8192, 0, capd)], order)
        assert fwd[-2][0] == 0 and fwd[-2][1] == 0, "a destination below getMaxEncodedLength is refused, the type untouched (UTFCodec.cpp:62)"
        assert fwd[-1][0] == 1 and fwd[-1][1] == 8
        outputs = {}
        for i, (r, b, (ok, dt, out)) in enumerate(zip(recs, blocks, fwd)):
            if len(b) == 0:
                continue                                     # (takes no part in a batch)
            assert ok == r["ok"], ("ok", r["recipe"], r["dtype"], order)
            assert dt == r["dtype_out"], ("data type", r["recipe"], r["dtype"], order)
            if r["ok"]:
                assert len(out) == r["fwd_len"] and md5(out) == r["fwd_md5"], ("forward", r["recipe"], order)
                if "fwd_hex" in r:
                    assert out.hex() == r["fwd_hex"]
                outputs[i] = out
        cases = inverse_cases(outputs)
        assert len(cases) == len(GOLDEN["inverse"]) + len(GOLDEN["damaged"])
        got = run_cases(exe, tmp_path, [c for c, _ in cases], order)
        check_inverse(cases, got, order)


def test_utf_damaged_inverse_input_under_address_sanitizer(tmp_path):
    """The inverse and damaged records, and the forward of the records they come from, in a host build of the kernels under
    AddressSanitizer: the reference's verdict, nothing read or written out of bounds."""
    exe = build("utf_emu", tmp_path, extra=["-fsanitize=address", "-g", "-fno-omit-frame-pointer"])
    idx = [i for i, r in enumerate(GOLDEN["stage"]) if r["ok"] and 0 < r["fwd_len"] < 70000]
    recs = [GOLDEN["stage"][i] for i in idx]
    fwd = run_cases(exe, tmp_path, [(1, r["cap"], r["dtype"], b) for r, b in zip(recs, _blocks(recs))], "0")
    outputs = {i: out for i, (ok, _, out) in zip(idx, fwd) if ok}
    assert len(outputs) == len(recs)
    cases = inverse_cases(outputs)
    assert len(cases) >= len(GOLDEN["damaged"])
    got = run_cases(exe, tmp_path, [c for c, _ in cases], "2")
    check_inverse(cases, got, "2")
