"""Writes tests/golden/range.json from the reference's command line (oracle/_ref/kanzi, which build() makes where the reference
sources exist): for every case of tests/range_cases.py the input recipe, the stream header and the length and md5 of what
`kanzi -c -t CHAIN -e RANGE -b SIZE -j 1` writes, from a file (the header carries the input's size) and from standard input (it
carries none: what a writer that cannot know the size, such as the C API's compressor, has to produce).
The `wide` section holds the chunks with a wrapped frequency (range_cases.WIDE, WIDE_STREAMS), per stage and framed, from the
reference build's library (knzlib.Ref). The tests read only this file.
    python tools/make_range_golden.py [--find-underflow]
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
import range_cases  # noqa: E402
import range_model  # noqa: E402


def md5(b):
    return hashlib.md5(b).hexdigest()


def ref_cli(data, chain, bs, checksum, from_stdin=False):
    with tempfile.TemporaryDirectory() as tmp:
        src, dst = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.knz")
        with open(src, "wb") as f:
            f.write(data)
        cmd = [knzlib.REF_BIN, "-c", "-i", "STDIN" if from_stdin else src, "-o", dst, "-f", "-t", chain, "-e", "RANGE", "-b", str(bs), "-j", "1"]
        if checksum:
            cmd.append("-x%d" % checksum)
        with open(src, "rb") as f:
            subprocess.run(cmd, check=True, stdin=f if from_stdin else subprocess.DEVNULL, stdout=subprocess.DEVNULL)
        return open(dst, "rb").read()


def record(name, chain, recipe, bs, checksum):
    knzlib.load_pkg()
    import importlib
    framing = importlib.import_module("kanzi_amd.framing")
    d = range_cases.make(recipe)
    enc = ref_cli(d, chain, bs, checksum)
    h = framing.parse_header(enc)
    assert h["etype"] == 4 and h["block_size"] == bs and h["checksum_bits"] == checksum, name
    unsized = ref_cli(d, chain, bs, checksum, from_stdin=True)
    h0 = framing.parse_header(unsized)
    assert h0["orig_size"] == 0 and h0["etype"] == 4 and h0["block_size"] == bs and h0["checksum_bits"] == checksum, name
    assert h["bits"] % 8 == 0 and h0["bits"] % 8 == 0 and unsized[h0["bits"] // 8:] == enc[h["bits"] // 8:], name    # only the header differs
    return {"name": name, "chain": chain, "recipe": recipe, "block_size": bs, "checksum": checksum, "n": len(d), "input_md5": md5(d),
            "orig_size": h["orig_size"], "header_bits": h["bits"], "knz_len": len(enc), "knz_md5": md5(enc),
            "unsized_len": len(unsized), "unsized_md5": md5(unsized)}


def wide_records():
    """The chunks with a wrapped frequency (range_cases.WIDE, WIDE_STREAMS) from the reference build's library: per stage, and framed."""
    ref = knzlib.Ref()
    stage, streams = [], []
    for r in range_cases.WIDE:
        d = range_cases.make(r)
        enc, bits = ref.entropy_encode("RANGE", d)
        rc, back = ref.entropy_decode("RANGE", enc, len(d))
        stage.append({"recipe": r, "n": len(d), "input_md5": md5(d), "bits": bits, "enc_md5": md5(enc), "ref_decodes": int(rc >= 0 and back == d)})
    for r, bs, ck, jobs in range_cases.WIDE_STREAMS:
        d = range_cases.make(r)
        rc, enc = ref.compress(d, "NONE", "RANGE", bs, jobs=jobs, checksum=ck, headerless=1)
        assert rc == 0, r
        rc1, full = ref.compress(d, "NONE", "RANGE", bs, jobs=jobs, checksum=ck, orig_size=len(d))
        rc2, back = ref.decompress(full, len(d) + bs, jobs=jobs)
        streams.append({"recipe": r, "block_size": bs, "checksum": ck, "jobs": jobs, "n": len(d), "input_md5": md5(d),
                        "stream_len": len(enc), "stream_md5": md5(enc), "ref_decodes": int(rc1 == 0 and rc2 == 0 and back == d)})
    return {"stage": stage, "streams": streams}


def find_underflow():
    for seed in range(1, 200):
        st = range_model.Stats()
        range_model.encode(range_cases.make(["rand", 32768, seed]), st)
        if st.underflows:
            print("UNDERFLOW =", ["rand", 32768, seed], "taken", st.underflows, "times")
            return
    print("none found")


def main():
    if "--find-underflow" in sys.argv:
        return find_underflow()
    if not os.path.exists(knzlib.REF_BIN):
        knzlib.ensure_ref()
    out = {"streams": [record(n, "NONE", r, bs, ck) for n, r, bs, ck in range_cases.STREAMS],
           "chains": [record(c, c, r, bs, ck) for c, r, bs, ck in range_cases.CHAINS],
           "hosted": [record(c, c, r, bs, ck) for c, r, bs, ck in range_cases.HOSTED],
           "wide": wide_records()}
    path = os.path.join(ROOT, "tests", "golden", "range.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", path)


if __name__ == "__main__":
    main()
