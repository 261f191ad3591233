"""kanzi.TensorCodec with byte planes on the device: the cases are in tests/tensor_planes_cases.py and run there, all in ONE child process
started once (as tests/test_gpu_tensors.py does, and for its reason). Every case is a test of its own here and shows the child's traceback
when it failed."""
import json
import os
import re
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = re.findall(r"^def (case_\w+)\(", open(os.path.join(HERE, "tensor_planes_cases.py")).read(), re.M)
_results = {}


def results():
    """The child's verdicts, from one run: a child that ends badly is not started again."""
    if not _results:
        r = subprocess.run([sys.executable, os.path.join(HERE, "tensor_planes_cases.py")], capture_output=True, text=True, timeout=600)
        lines = [l for l in r.stdout.splitlines() if l.startswith("RESULTS ")]
        if r.returncode == 0 and lines:
            _results.update(json.loads(lines[-1][len("RESULTS "):]))
        else:
            _results["child"] = "the child ended with %d\n%s\n%s" % (r.returncode, r.stdout[-3000:], r.stderr[-3000:])
    assert "child" not in _results, _results["child"]
    return _results


def test_the_cases_are_all_here():
    assert len(CASES) == 7 and sorted(results()) == sorted(CASES)


@pytest.mark.parametrize("case", CASES)
def test_tensor_codec_planes(case):
    assert results().get(case) == "ok", results().get(case)
