"""Writes tests/golden/text.json from the reference build in oracle/_ref (build() makes it where the reference sources exist).

Stage records, one per case of tests/text_cases.py, codec (1: entropy FPAQ, 2: ANS0, 3: TPAQX) and stream block size: the recipe, the data
type the block comes with, the forward result (ok flag, data type afterwards, length, md5) and "source". The reference's per-stage
harness (oracle/ref_harness.cpp) has no "blockSize" entry in its Context and takes either an entropy name or a data type, so:
  block size 0, data type 0     ok and bytes are the reference's for all three codecs (source "ref"); the data type afterwards is the
                                reference's for codec 1, the host code's (host/text_codec.cpp) for codecs 2 and 3
  block size 0, preset types    the reference's for codec 1 (ok, bytes, type), the host code's for codecs 2 and 3 (source "host")
  other block sizes             the host code's (source "host"); the "big" stream records below are the reference's streams of 4 MiB
                                blocks over the two largest recipes, which pins the maps of 2^19 (codec 1) and 2^17 slots (codec 2) to it;
                                the doubled map of TPAQX at 4 MiB (2^20 slots) has the host code's values only
and wherever both exist this tool asserts that they agree. Every accepted output goes back through the host inverse, and for codec 1
at block size 0 through the reference's. Damaged records: outputs of text_cases.DAMAGE_FROM damaged in the ways of
text_cases.damaged_cases, and whole into capacities that are too short: the verdict and bytes of knz_host_text_inverse (the
reference reads out of bounds on some of them, text_codec.cpp:449-451). Stream records: the md5 of the reference's headerless stream
for each chain of text_cases.STREAM_CHAINS, MIXED_CHAINS, DNA_CHAINS (an ACGT block that DNA takes and a text block it refuses) and
BIG_CHAINS (blocks of 4 MiB; the tool asserts that the host code's TEXT output for those blocks is what the reference's stream holds). CLI records: length and md5 of what the reference's tool writes for
text_cases.STREAM with -l N -b 64k -j 1, for the levels of text_cases.CLI_LEVELS. No input bytes are stored; the tests read only this file.
    python tools/make_text_golden.py
"""
import ctypes as C
import hashlib
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import knzlib  # noqa: E402
import text_cases  # noqa: E402


def md5(b):
    return hashlib.md5(b).hexdigest()


class Host:
    """knz_host_text_forward / _inverse of libkanzi_amd.so"""

    def __init__(self):
        L = self.L = C.CDLL(os.path.join(knzlib.PKG, "libkanzi_amd.so"))
        u8p = C.POINTER(C.c_uint8)
        L.knz_host_text_forward.argtypes = [C.c_int, u8p, C.c_int, u8p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]
        L.knz_host_text_inverse.argtypes = [C.c_int, u8p, C.c_int, u8p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int)]

    def forward(self, codec, d, block_size, data_type):
        out = (C.c_uint8 * (len(d) + 64))()
        dt, ol = C.c_int(data_type), C.c_int(0)
        ok = self.L.knz_host_text_forward(codec, knzlib._buf(d), len(d), out, len(d), block_size, 6, C.byref(dt), C.byref(ol))
        return ok, C.string_at(out, ol.value) if ok else b"", dt.value

    def inverse(self, codec, e, cap, block_size):
        out = (C.c_uint8 * (cap + 64))()
        ol = C.c_int(0)
        ok = self.L.knz_host_text_inverse(codec, knzlib._buf(e), len(e), out, cap, block_size, 6, C.byref(ol))
        return ok, C.string_at(out, ol.value) if ok else b""


def stage_records(host, ref=None, log=print):
    recs, outputs = [], {}
    for name, recipe, dt in text_cases.stage_cases():
        d = text_cases.make(recipe)
        for codec in (1, 2, 3):
            for bs in text_cases.BLOCK_SIZES:
                ok, fwd, dt_out = host.forward(codec, d, bs, dt)
                source = "host"
                if ref is not None and bs == 0 and dt == 0:
                    rok, rfwd, _ = ref.forward("TEXT", d, len(d), text_cases.ENTROPY[codec])
                    assert (int(rok == 1), rfwd if rok == 1 else b"") == (ok, fwd), ("the host code differs from the reference", name, codec)
                    source = "ref"
                if ref is not None and bs == 0 and codec == 1:
                    rok, rfwd, rdt = ref.forward_dt("TEXT", d, len(d), dt)
                    assert (int(rok == 1), rfwd if rok == 1 else b"", rdt) == (ok, fwd, dt_out), ("the host code differs from the reference", name, dt)
                    source = "ref"
                rec = {"name": name, "recipe": recipe, "dtype": dt, "codec": codec, "block_size": bs, "input_md5": md5(d), "ok": ok,
                       "dtype_out": dt_out, "source": source}
                if ok:
                    ok2, back = host.inverse(codec, fwd, len(d), bs)
                    assert ok2 == 1 and back == d, ("no round trip", name, codec, bs)
                    if ref is not None and bs == 0 and codec == 1:
                        ok2, back = ref.inverse("TEXT", fwd, len(d))
                        assert ok2 == 1 and back == d, ("the reference does not give the block back", name)
                    rec.update({"fwd_len": len(fwd), "fwd_md5": md5(fwd)})
                    outputs[(name, codec, bs)] = fwd
                recs.append(rec)
        log("%-40s %s" % (name, [(r["codec"], r["ok"], r["dtype_out"], r.get("fwd_len")) for r in recs[-9::3]]))
    return recs, outputs


def damaged_records(host, outputs):
    recs = []
    n = text_cases.stage_cases()[[c[0] for c in text_cases.stage_cases()].index(text_cases.DAMAGE_FROM)][1][1]
    for codec in (1, 2, 3):
        fwd = outputs[(text_cases.DAMAGE_FROM, codec, 0)]
        cases = [(name, op, n) for name, op in text_cases.damaged_cases(codec)]
        cases += [("whole", ["append", []], n), ("capacity one short", ["append", []], n - 1), ("capacity 100 short", ["append", []], n - 100)]
        for name, op, cap in cases:
            bad = text_cases.damage(fwd, op, codec)
            ok, inv = host.inverse(codec, bad, cap, 0)
            assert (name == "whole") == (ok == 1), (name, codec, ok)
            recs.append({"name": name, "codec": codec, "op": op, "cap": cap, "input_md5": md5(bad), "ok": ok,
                         "inv_len": len(inv) if ok else None, "inv_md5": md5(inv) if ok else None})
    return recs


def stream_records(ref, log=print):
    out = {"streams": [], "mixed": [], "dna": [], "big": []}
    d = text_cases.make(text_cases.STREAM)
    plain = {}
    for chain, entropy, ck in text_cases.STREAM_CHAINS:
        rc, enc = ref.compress(d, chain, entropy, text_cases.STREAM_BS, headerless=1, checksum=ck)
        assert rc == 0, chain
        without = "+".join(t for t in chain.split("+") if t != "TEXT") or "NONE"
        rc, other = ref.compress(d, without, entropy, text_cases.STREAM_BS, headerless=1, checksum=ck)
        assert rc == 0
        if other == enc:
            log("TEXT takes no block of", chain)
        rc, back = ref.decompress(ref.compress(d, chain, entropy, text_cases.STREAM_BS, checksum=ck)[1], len(d) + text_cases.STREAM_BS)
        assert rc == 0 and back == d, chain
        log(chain, entropy, len(enc))
        out["streams"].append({"chain": chain, "entropy": entropy, "block_size": text_cases.STREAM_BS, "checksum": ck, "input_md5": md5(d),
                               "stream_len": len(enc), "stream_md5": md5(enc)})
    d = text_cases.mixed()
    for chain, entropy, ck in text_cases.MIXED_CHAINS:
        rc, enc = ref.compress(d, chain, entropy, text_cases.STREAM_BS, headerless=1, checksum=ck)
        assert rc == 0, chain
        out["mixed"].append({"chain": chain, "entropy": entropy, "block_size": text_cases.STREAM_BS, "checksum": ck, "input_md5": md5(d),
                             "stream_len": len(enc), "stream_md5": md5(enc)})
    d = text_cases.dna_blocks()
    for chain, entropy, ck in text_cases.DNA_CHAINS:
        rc, enc = ref.compress(d, chain, entropy, text_cases.STREAM_BS, headerless=1, checksum=ck)
        assert rc == 0, chain
        rc, half = ref.compress(d[text_cases.STREAM_BS:], chain, entropy, text_cases.STREAM_BS, headerless=1, checksum=ck)
        rc2, none = ref.compress(d[text_cases.STREAM_BS:], chain.replace("DNA+", "").replace("DNA", "NONE"), entropy, text_cases.STREAM_BS, headerless=1, checksum=ck)
        assert rc == 0 and rc2 == 0 and len(half) == len(none), "DNA takes the text block"
        rc, none = ref.compress(d[:text_cases.STREAM_BS], chain.replace("DNA+", "").replace("DNA", "NONE"), entropy, text_cases.STREAM_BS, headerless=1, checksum=ck)
        rc2, half = ref.compress(d[:text_cases.STREAM_BS], chain, entropy, text_cases.STREAM_BS, headerless=1, checksum=ck)
        assert rc == 0 and rc2 == 0 and half != none and (entropy != "NONE" or len(half) < len(none) * 3 // 4), "DNA does not take the ACGT block"
        out["dna"].append({"chain": chain, "entropy": entropy, "block_size": text_cases.STREAM_BS, "checksum": ck, "input_md5": md5(d),
                           "stream_len": len(enc), "stream_md5": md5(enc)})
    d = text_cases.big_blocks()
    for chain, entropy, ck in text_cases.BIG_CHAINS:
        rc, enc = ref.compress(d, chain, entropy, text_cases.BIG_BS, headerless=1, checksum=ck)
        assert rc == 0, chain
        if entropy == "NONE":
            # the stream holds the TEXT output byte for byte: the host code's, at this map size
            # (a block starts at any bit of the stream)
            host, bits = Host(), int.from_bytes(enc, "big")
            shifted = [((bits << sh) & ((1 << (8 * len(enc))) - 1)).to_bytes(len(enc), "big") for sh in range(8)]
            for off in range(0, len(d), text_cases.BIG_BS):
                ok, fwd, _ = host.forward(2, d[off:off + text_cases.BIG_BS], text_cases.BIG_BS, 0)
                assert ok and any(fwd in e for e in shifted), "the host code differs from the reference at 4 MiB blocks"
        out["big"].append({"chain": chain, "entropy": entropy, "block_size": text_cases.BIG_BS, "checksum": ck, "input_md5": md5(d),
                           "stream_len": len(enc), "stream_md5": md5(enc)})
    return out


def cli_records():
    out = []
    d = text_cases.make(text_cases.STREAM)
    with tempfile.TemporaryDirectory() as tmp:
        src, dst = os.path.join(tmp, "in.txt"), os.path.join(tmp, "out.knz")
        open(src, "wb").write(d)
        for level in text_cases.CLI_LEVELS:
            subprocess.check_call([knzlib.REF_BIN, "-c", "-i", src, "-o", dst, "-f", "-j", "1", "-l", str(level), "-b", "64k"], stdout=subprocess.DEVNULL)
            enc = open(dst, "rb").read()
            out.append({"level": level, "input_md5": md5(d), "knz_len": len(enc), "knz_md5": md5(enc)})
    return out


def build_golden(log=print):
    """Every record (tests/test_text_golden.py compares the stored file with this)."""
    ref, host = knzlib.Ref(), Host()
    stage, outputs = stage_records(host, ref, log)
    out = {"stage": stage, "damaged": damaged_records(host, outputs)}
    out.update(stream_records(ref, log))
    out["cli"] = cli_records()
    return json.loads(json.dumps(out))


def main():
    out = build_golden()
    path = os.path.join(ROOT, "tests", "golden", "text.json")
    with open(path, "w") as f:
        json.dump(out, f, separators=(",", ":"))
        f.write("\n")
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
