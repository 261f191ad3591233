"""Writes tests/golden/streams.json: length and md5 of the file the reference CLI (oracle/_ref/kanzi, built by
__graft_entry__.build() where the reference's sources exist) writes for every file of the tree of tests/stream_tree.py, under each of
its option sets. The directory-mode tests of kanzi_amd_cli compare with it, so that they hold on a machine without oracle/_ref as well.
Runs on the CPU:  python tools/make_streams_golden.py"""
import hashlib
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import knzlib          # noqa: E402
import stream_tree     # noqa: E402


def main():
    if knzlib.ensure_ref() is None or not os.path.exists(knzlib.REF_BIN):
        raise SystemExit("oracle/_ref/kanzi is not built")
    out = {"args": stream_tree.CLI_ARGS, "files": {}}
    with tempfile.TemporaryDirectory() as tmp:
        stream_tree.write(tmp)
        for rel, data in sorted(stream_tree.files().items()):
            recs = []
            for args in stream_tree.CLI_ARGS:
                knz = os.path.join(tmp, "out.knz")
                subprocess.check_call([knzlib.REF_BIN, "-c", "-i", os.path.join(tmp, rel), "-o", knz, "-f", "-j", "1", "-v", "0"] + args)
                enc = open(knz, "rb").read()
                recs.append({"len": len(enc), "md5": hashlib.md5(enc).hexdigest()})
            out["files"][rel] = {"n": len(data), "md5": hashlib.md5(data).hexdigest(), "knz": recs}
    path = os.path.join(ROOT, "tests", "golden", "streams.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", path, len(out["files"]), "files")


if __name__ == "__main__":
    main()
