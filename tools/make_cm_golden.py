"""Writes tests/golden/cm.json from the reference's command line (oracle/_ref/kanzi, which build() makes where the reference sources
exist): for every case of tests/cm_cases.py the input recipe, the stream header and the length and md5 of what
`kanzi -c -t CHAIN -e CM -b SIZE -j 1` writes, from a file (the header carries the input's size) and from standard input (it carries
none: what a writer that cannot know the size, such as the C API's compressor, has to produce). The tests read only this file.
    python tools/make_cm_golden.py
"""
import hashlib
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import knzlib  # noqa: E402
import cm_cases  # noqa: E402
import cm_model  # noqa: E402


def md5(b):
    return hashlib.md5(b).hexdigest()


def ref_cli(data, chain, bs, checksum, from_stdin=False):
    with tempfile.TemporaryDirectory() as tmp:
        src, dst = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.knz")
        with open(src, "wb") as f:
            f.write(data)
        cmd = [knzlib.REF_BIN, "-c", "-i", "STDIN" if from_stdin else src, "-o", dst, "-f", "-t", chain, "-e", "CM", "-b", str(bs), "-j", "1"]
        if checksum:
            cmd.append("-x%d" % checksum)
        with open(src, "rb") as f:
            subprocess.run(cmd, check=True, stdin=f if from_stdin else subprocess.DEVNULL, stdout=subprocess.DEVNULL)
        return open(dst, "rb").read()


def record(name, chain, recipe, bs, checksum):
    knzlib.load_pkg()
    import importlib
    framing = importlib.import_module("kanzi_amd.framing")
    d = cm_cases.make(recipe)
    enc = ref_cli(d, chain, bs, checksum)
    h = framing.parse_header(enc)
    assert h["etype"] == 6 and h["block_size"] == bs and h["checksum_bits"] == checksum, name
    unsized = ref_cli(d, chain, bs, checksum, from_stdin=True)
    h0 = framing.parse_header(unsized)
    assert h0["orig_size"] == 0 and h0["etype"] == 6 and h0["block_size"] == bs and h0["checksum_bits"] == checksum, name
    assert h["bits"] % 8 == 0 and h0["bits"] % 8 == 0 and unsized[h0["bits"] // 8:] == enc[h["bits"] // 8:], name    # only the header differs
    return {"name": name, "chain": chain, "recipe": recipe, "block_size": bs, "checksum": checksum, "n": len(d), "input_md5": md5(d),
            "orig_size": h["orig_size"], "header_bits": h["bits"], "knz_len": len(enc), "knz_md5": md5(enc),
            "unsized_len": len(unsized), "unsized_md5": md5(unsized)}


def adversary_record():
    """Whether the reference's payload for the adversary block exceeds n + n / 8, the encoder's first staging: measured on the
    reference's own stream (block payload = stream minus header, block framing and end marker), asserted equal to the model's."""
    d = cm_cases.make(cm_cases.ADVERSARY)
    sizes = []
    enc, bits = cm_model.encode(d, payloads=sizes)
    rec = next(r for r in cm_cases.STREAMS if r[0] == "adversary")
    ref = ref_cli(d, "NONE", rec[2], 0)
    knzlib.load_pkg()
    import importlib
    framing = importlib.import_module("kanzi_amd.framing")
    h = framing.parse_header(ref)
    assert cm_model.stream(ref[:(h["bits"] + 7) // 8], h["bits"], d, rec[2]) == ref       # the payload size below is the reference's
    n = len(d)
    return {"n": n, "payload_bytes": sizes[0], "first_staging": n + n // 8, "exceeds_first_staging": sizes[0] > n + n // 8}


def main():
    if not os.path.exists(knzlib.REF_BIN):
        knzlib.ensure_ref()
    out = {"streams": [record(n, "NONE", r, bs, ck) for n, r, bs, ck in cm_cases.STREAMS],
           "chains": [record(c, c, r, bs, ck) for c, r, bs, ck in cm_cases.CHAINS],
           "hosted": [record(c, c, r, bs, ck) for c, r, bs, ck in cm_cases.HOSTED],
           "adversary": adversary_record()}
    path = os.path.join(ROOT, "tests", "golden", "cm.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", path)


if __name__ == "__main__":
    main()
