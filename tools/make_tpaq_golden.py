"""Writes tests/golden/tpaq.json from the reference's command line (oracle/_ref/kanzi, which build() makes where the reference sources
exist): for every case of tests/tpaq_cases.py and both coders the input recipe, the stream header and the length and md5 of what
`kanzi -c -t CHAIN -e TPAQ|TPAQX -b SIZE -j 1` writes, from a file (the header carries the input's size) and from standard input (it
carries none: what a writer that cannot know the size has to produce). The reference's decoder is run on each stream as well, so a
record is a stream the reference itself reads back (this matters at `-b 10000`, whose masks are not 2^k - 1). The tests read only this
file.
    python tools/make_tpaq_golden.py
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
import tpaq_cases  # noqa: E402


def md5(b):
    return hashlib.md5(b).hexdigest()


def ref_cli(data, chain, coder, bs, checksum, from_stdin=False):
    with tempfile.TemporaryDirectory() as tmp:
        src, dst, back = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.knz"), os.path.join(tmp, "back.bin")
        with open(src, "wb") as f:
            f.write(data)
        cmd = [knzlib.REF_BIN, "-c", "-i", "STDIN" if from_stdin else src, "-o", dst, "-f", "-t", chain, "-e", coder, "-b", str(bs), "-j", "1"]
        if checksum:
            cmd.append("-x%d" % checksum)
        with open(src, "rb") as f:
            subprocess.run(cmd, check=True, stdin=f if from_stdin else subprocess.DEVNULL, stdout=subprocess.DEVNULL)
        if not from_stdin:
            subprocess.run([knzlib.REF_BIN, "-d", "-i", dst, "-o", back, "-f", "-j", "1"], check=True, stdin=subprocess.DEVNULL, stdout=subprocess.DEVNULL)
            assert open(back, "rb").read() == data, (chain, coder, bs)
        return open(dst, "rb").read()


def record(name, chain, coder, recipe, bs, checksum):
    knzlib.load_pkg()
    import importlib
    framing = importlib.import_module("kanzi_amd.framing")
    d = tpaq_cases.make(recipe)
    enc = ref_cli(d, chain, coder, bs, checksum)
    h = framing.parse_header(enc)
    eid = tpaq_cases.ENTROPY_ID[coder]
    assert h["etype"] == eid and h["block_size"] == bs and h["checksum_bits"] == checksum, name
    unsized = ref_cli(d, chain, coder, bs, checksum, from_stdin=True)
    h0 = framing.parse_header(unsized)
    assert h0["orig_size"] == 0 and h0["etype"] == eid and h0["block_size"] == bs and h0["checksum_bits"] == checksum, name
    assert h["bits"] % 8 == 0 and h0["bits"] % 8 == 0 and unsized[h0["bits"] // 8:] == enc[h["bits"] // 8:], name    # only the header differs
    return {"name": name, "chain": chain, "coder": coder, "recipe": recipe, "block_size": bs, "checksum": checksum, "n": len(d),
            "input_md5": md5(d), "orig_size": h["orig_size"], "header_bits": h["bits"], "header_hex": enc[:(h["bits"] + 7) // 8].hex(),
            "knz_len": len(enc), "knz_md5": md5(enc), "unsized_len": len(unsized), "unsized_md5": md5(unsized)}


def main():
    if not os.path.exists(knzlib.REF_BIN):
        knzlib.ensure_ref()
    both = tpaq_cases.CODERS
    out = {"streams": [record(n, "NONE", c, r, bs, ck) for n, r, bs, ck in tpaq_cases.STREAMS for c in both],
           "chains": [record(t, t, c, r, bs, ck) for t, r, bs, ck in tpaq_cases.CHAINS for c in both],
           "hosted": [record(t, t, c, r, bs, ck) for t, r, bs, ck in tpaq_cases.HOSTED for c in both]}
    path = os.path.join(ROOT, "tests", "golden", "tpaq.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", path)


if __name__ == "__main__":
    main()
