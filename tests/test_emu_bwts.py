"""BWTS kernels on the CPU: kanzi-cpp_amd/csrc/bwts.hip (with the suffix sort of bwt_fwd.hip it starts from) compiled as plain C++
against the fiber emulation in tools/hipemu, compared with the reference's outputs recorded in tests/golden/bwts.json
(tools/make_bwts_golden.py). Test infrastructure only: the product runs the real kernels (tests/test_gpu_bwts.py)."""
import hashlib
import json
import os
import struct
import subprocess

import bwts_cases
from test_emu_kernels import build, write_case

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bwts.json")


def read_results(path, nBlocks):
    d = open(path, "rb").read()
    o, res = 0, []
    for _ in range(nBlocks):
        pair = []
        for _ in range(2):
            n = struct.unpack_from("<I", d, o)[0]
            o += 4
            pair.append(d[o:o + n])
            o += n
        res.append(pair)
    return res


def test_bwts_kernels_emulated(tmp_path):
    """Forward and inverse of every small fixture case in one ragged batch per direction (sizes 0, 1, 2, the reference's TestBWT
    strings, all bytes equal, strictly decreasing, abab..., a^k b, random, text, zero runs), forward output and inverse of the raw
    bytes equal to the reference's, round trip checked inside the harness; workgroups dispatched in order and shuffled."""
    golden = json.load(open(GOLDEN))
    recs = golden["stage"]
    blocks = [bwts_cases.make(r["recipe"]) for r in recs]
    for r, b in zip(recs, blocks):
        assert hashlib.md5(b).hexdigest() == r["input_md5"], r["recipe"]
    exe = build("bwts_emu", tmp_path)
    case, res = str(tmp_path / "case.bin"), str(tmp_path / "res.bin")
    write_case(case, blocks)
    for order in ("0", "2"):
        r = subprocess.run([exe, case, res], capture_output=True, text=True, timeout=900, env=dict(os.environ, HIPEMU_ORDER=order))
        assert r.returncode == 0, (order, r.stdout[-2000:] + r.stderr[-2000:])
        for rec, (fwd, inv) in zip(recs, read_results(res, len(blocks))):
            assert hashlib.md5(fwd).hexdigest() == rec["fwd_md5"], ("forward", rec["recipe"], order)
            assert hashlib.md5(inv).hexdigest() == rec["inv_md5"], ("inverse", rec["recipe"], order)
            if "fwd_hex" in rec:
                assert fwd.hex() == rec["fwd_hex"] and inv.hex() == rec["inv_hex"], rec["recipe"]
