"""EXE kernels on the CPU: kanzi-cpp_amd/csrc/exe.hip compiled as plain C++ against the fiber emulation in tools/hipemu, compared with
the reference's results recorded in tests/golden/exe.json (tools/make_exe_golden.py). Test infrastructure only: the product runs the
real kernels (tests/test_gpu_exe.py)."""
import hashlib
import json
import os

import exe_cases
from test_emu_kernels import build
from test_emu_mm import run_cases

GOLDEN = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "exe.json")))


def md5(b):
    return hashlib.md5(b).hexdigest()


def _blocks(recs):
    blocks = [exe_cases.make(r["recipe"]) for r in recs]
    for r, b in zip(recs, blocks):
        assert md5(b) == r["input_md5"], r["name"]
    return blocks


def check_forward(recs, blocks, got, order):
    """The reference's verdict, data type and bytes; returns the accepted outputs by name."""
    outputs = {}
    for r, b, (ok, dt, out) in zip(recs, blocks, got):
        assert ok == r["ok"], ("ok", r["name"], order)
        assert dt == r["dtype_out"], ("data type", r["name"], order)
        if r["ok"]:
            assert len(out) == r["fwd_len"] and md5(out) == r["fwd_md5"], ("forward", r["name"], order)
            outputs[r["name"]] = out
    return outputs


def inverse_cases(outputs):
    cases = []
    for r in GOLDEN["damaged"]:
        if r["stage"] not in outputs:
            continue
        d = exe_cases.damage(outputs[r["stage"]], r["op"])
        assert md5(d) == r["input_md5"], r
        cases.append(((0, r["cap"], 0, d), r))
    return cases


def check_inverse(cases, got, order):
    n_refused = 0
    for ((_, cap, _, _), r), (ok, _, out) in zip(cases, got):
        assert ok == r["ok"], ("inverse ok", r["stage"], r["op"], cap, order)
        n_refused += 1 - ok
        if r["ok"]:
            assert len(out) == r["inv_len"] and md5(out) == r["inv_md5"], ("inverse bytes", r["stage"], r["op"], cap, order)
    assert n_refused > 0


def test_exe_every_record_emulated(tmp_path):
    """Every stage record with its data type in one ragged forward batch (with one block whose destination is one byte below the bound and
    an empty block), every accepted output and every damaged record in one ragged inverse batch: the reference's verdict, bytes and data
    type, nothing written behind a capacity; workgroups dispatched in order and shuffled."""
    recs = GOLDEN["stage"]
    blocks = _blocks(recs)
    short = blocks[[r["name"] for r in recs].index("x86 8192")]
    exe = build("exe_emu", tmp_path)
    for order in ("0", "2"):
        fwd = run_cases(exe, tmp_path, [(1, r["cap"], r["dtype"], b) for r, b in zip(recs, blocks)]
                        + [(1, exe_cases.max_encoded(len(short)) - 1, 0, short), (1, 100, 0, b"")], order)
        assert fwd[-2][0] == 0 and fwd[-2][1] == 0, "a destination below getMaxEncodedLength is refused, the type untouched (EXECodec.cpp:77)"
        assert fwd[-1][0] == 1 and fwd[-1][2] == b""
        outputs = check_forward(recs, blocks, fwd, order)
        back = {r["name"]: (len(b), r["inv_md5"]) for r, b in zip(recs, blocks) if r["ok"]}
        whole = [(0, back[name][0], 0, out) for name, out in outputs.items()]               # (the destination is smaller than the input)
        cases = inverse_cases(outputs)
        assert len(cases) == len(GOLDEN["damaged"])
        got = run_cases(exe, tmp_path, whole + [c for c, _ in cases], order)
        for (name, _), (ok, _, out) in zip(outputs.items(), got):
            assert ok == 1 and (len(out), md5(out)) == back[name], ("round trip", name, order)
        check_inverse(cases, got[len(whole):], order)


def test_exe_under_address_sanitizer(tmp_path):
    """The stage records up to 70,000 bytes, their round trips and the damaged records in a host build of the kernels under
    AddressSanitizer: the reference's results, nothing read or written out of bounds."""
    exe = build("exe_emu", tmp_path, extra=["-fsanitize=address", "-g", "-fno-omit-frame-pointer"])
    recs = [r for r in GOLDEN["stage"] if r["recipe"][1] <= 70000]
    blocks = _blocks(recs)
    fwd = run_cases(exe, tmp_path, [(1, r["cap"], r["dtype"], b) for r, b in zip(recs, blocks)], "0")
    outputs = check_forward(recs, blocks, fwd, "asan")
    cases = inverse_cases(outputs)
    assert len(cases) == len(GOLDEN["damaged"])
    got = run_cases(exe, tmp_path, [c for c, _ in cases], "2")
    check_inverse(cases, got, "asan")
