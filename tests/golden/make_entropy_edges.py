#!/usr/bin/env python3
"""Writes tests/golden/entropy_edges.json: what the UNMODIFIED reference compiled into oracle/_ref/ (build container only) writes for
the inputs of tests/entropy_edge_cases.py:   make -C oracle ref && python tests/golden/make_entropy_edges.py

Per stage case and coder (ANS0, ANS1, HUFFMAN, FPAQ): bit count, byte length and md5 of the entropy stage's output. Per batch case:
byte length and md5 of the headerless stream (transform NONE). Per input: its md5. Digests only, never bytes. The reference must
decode everything it wrote here: a case it cannot read back is no edge case but a quirk, and is to be replaced, not exempted."""
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import knzlib  # noqa: E402
import entropy_edge_cases as eec  # noqa: E402

PATH = os.path.join(HERE, "entropy_edges.json")


def md5(b):
    return hashlib.md5(b).hexdigest()


def main():
    R = knzlib.Ref()
    inputs, stage, batch = {}, {}, {}
    for name, data, prop in eec.stage_cases():
        inputs[name] = md5(data)
        stage[name] = {}
        for coder in eec.CODERS:
            enc, bits = R.entropy_encode(coder, data)
            assert enc is not None, (name, coder, bits)
            r, back = R.entropy_decode(coder, enc, len(data))
            assert r == len(data) and back == data, ("the reference cannot read what it wrote", name, coder, r)
            stage[name][coder] = [bits, len(enc), md5(enc)]
    for name, bs, data in eec.batch_inputs():
        inputs[name] = md5(data)
        for coder in eec.CODERS:
            for ck in eec.BATCH_CHECKSUMS:
                rc, enc = R.compress(data, "NONE", coder, bs, jobs=1, checksum=ck, headerless=1)
                assert rc == 0, (name, coder, ck, rc)
                batch[eec.batch_key(name, coder, ck)] = [len(enc), md5(enc)]
    with open(PATH, "w") as f:
        f.write('{"inputs": {\n' + ",\n".join("%s: %s" % (json.dumps(k), json.dumps(v)) for k, v in inputs.items()) + '\n},\n"stage": {\n' +
                ",\n".join("%s: %s" % (json.dumps(k), json.dumps(v)) for k, v in stage.items()) + '\n},\n"batch": {\n' +
                ",\n".join("%s: %s" % (json.dumps(k), json.dumps(v)) for k, v in batch.items()) + "\n}}\n")
    print("%d stage cases x %d coders, %d batch streams" % (len(stage), len(eec.CODERS), len(batch)))


if __name__ == "__main__":
    main()
