"""The tree of small files that the directory mode of kanzi_amd_cli is tested on (tests/test_host_streams_stub.py on the CPU with the
stand-in device, tests/test_gpu_streams_cli.py on the device), and the CLI options it goes through. tools/make_streams_golden.py
records what the reference CLI writes for every file of it in tests/golden/streams.json."""
import os

import vectors

# the options of every run (reference and product take the same): chains the CPU stand-in of the device runs as well
CLI_ARGS = [["-t", "BWT+RANK+ZRLT", "-e", "ANS0", "-b", "64k", "-x32"], ["-t", "LZX", "-e", "HUFFMAN", "-b", "16k"]]


def files():
    """{relative path: bytes}: 30 files in three directories -- an empty one, copy-block sizes, sizes around the block sizes above, one
    of more than two blocks of 64 KiB, text, mixed, runs and random bytes."""
    out = {}
    sizes = [0, 1, 15, 16, 700, 1023, 1024, 5000, 16383, 16384, 16385, 40000, 65535, 65536, 65537, 2 * 65536 + 4321, 90000, 3, 2000, 33333,
             100, 8192, 12345, 70000, 131072, 17, 255, 256, 60000, 4096]
    kinds = ("text", "mixed", "runs", "rand")
    for i, n in enumerate(sizes):
        kind = kinds[i % 4]
        data = vectors.make({"text": ("text", n, 20 + i), "mixed": ("mixedslice", 300000, 3, i * 1000, i * 1000 + n), "runs": ("runs", 50, 8000),
                             "rand": ("rand", n, 40 + i)}[kind])[:n]
        assert len(data) == n
        sub = ("", "docs", os.path.join("docs", "deep"), "data")[i % 4 if i % 4 != 0 else (0 if i % 8 == 0 else 3)]
        out[os.path.join(sub, "f%02d_%s.%s" % (i, kind, "txt" if kind == "text" else "bin"))] = data
    assert len(out) == 30
    return out


def write(root):
    for rel, data in files().items():
        path = os.path.join(root, rel)
        os.makedirs(os.path.dirname(path), exist_ok=True)
        with open(path, "wb") as f:
            f.write(data)


def read(root, suffix=""):
    """{relative path without suffix: bytes} of every regular file under root whose name ends with suffix."""
    out = {}
    for d, _, names in os.walk(root):
        for nm in names:
            if nm.endswith(suffix):
                p = os.path.join(d, nm)
                rel = os.path.relpath(p, root)
                out[rel[:len(rel) - len(suffix)] if suffix else rel] = open(p, "rb").read()
    return out


def check_directory_mode(cli, tmp_path, ref_bin=None, env=None):
    """-c -i DIR -o OUT, then -d, with the binary `cli`, under every option set: every .knz is the reference CLI's file (by the digests of
    tests/golden/streams.json, and byte for byte where ref_bin is given) and what the same binary writes for that file alone, the tree comes
    back, and a file that cannot be written is reported by name while the others are. Then once without -o: F.knz beside F."""
    import hashlib
    import json
    import shutil
    import subprocess
    golden = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "streams.json")))
    assert golden["args"] == CLI_ARGS
    tree = files()
    assert {k: [len(v), hashlib.md5(v).hexdigest()] for k, v in tree.items()} == {k: [r["n"], r["md5"]] for k, r in golden["files"].items()}
    victim = sorted(k for k in tree if k.startswith(os.path.join("docs", "deep")))[1]
    for k, args in enumerate(CLI_ARGS):
        src, out, back = str(tmp_path / ("tree%d" % k)), str(tmp_path / ("out%d" % k)), str(tmp_path / ("back%d" % k))
        write(src)
        os.makedirs(os.path.join(out, victim + ".knz"))             # a directory where one file's output belongs: that file cannot be written
        r = subprocess.run([cli, "-c", "-i", src, "-o", out, "-j", "1", "-f"] + args, capture_output=True, text=True, env=env, timeout=600)
        assert r.returncode == 8, r.stderr[-2000:]                  # ERR_CREATE_FILE, the first (and only) failure
        assert os.path.join(src, victim) in r.stderr and "29 of 30" in r.stderr, r.stderr[-2000:]
        os.rmdir(os.path.join(out, victim + ".knz"))
        got = read(out, ".knz")
        assert set(got) == set(tree) - {victim}
        for rel, enc in got.items():
            rec = golden["files"][rel]["knz"][k]
            assert (len(enc), hashlib.md5(enc).hexdigest()) == (rec["len"], rec["md5"]), (args, rel)
        one = str(tmp_path / "one.knz")
        for rel, enc in sorted(got.items()):
            if ref_bin:
                subprocess.check_call([ref_bin, "-c", "-i", os.path.join(src, rel), "-o", one, "-f", "-j", "1", "-v", "0"] + args)
                assert open(one, "rb").read() == enc, (args, rel)
        # ... and what the same binary writes for each file alone: every file through a stream class of its own (KNZ_STREAMS_BATCH=0, one
        # process -- a process per file would spend its time starting the device), and three of them as the only file of a run
        alone = str(tmp_path / ("alone%d" % k))
        r = subprocess.run([cli, "-c", "-i", src, "-o", alone, "-j", "1"] + args, capture_output=True, text=True, timeout=600,
                           env=dict(os.environ if env is None else env, KNZ_STREAMS_BATCH="0"))
        assert r.returncode == 0 and "30 of 30" in r.stderr, r.stderr[-2000:]
        assert {rel: enc for rel, enc in read(alone, ".knz").items() if rel != victim} == got
        shutil.rmtree(alone)
        by_size = sorted(got, key=lambda rel: len(tree[rel]))
        for rel in (by_size[0], by_size[len(by_size) // 2], by_size[-1]) if k == 0 else ():
            subprocess.check_call([cli, "-c", "-i", os.path.join(src, rel), "-o", one, "-f", "-j", "1"] + args, stderr=subprocess.DEVNULL, env=env)
            assert open(one, "rb").read() == got[rel], (args, rel)
        if k == 0:
            # a second run without -f refuses to overwrite what is there, and writes the one file that is not
            r = subprocess.run([cli, "-c", "-i", src, "-o", out, "-j", "1"] + args, capture_output=True, text=True, env=env, timeout=600)
            assert r.returncode == 7 and "1 of 30" in r.stderr, r.stderr[-2000:]
        r = subprocess.run([cli, "-d", "-i", out, "-o", back], capture_output=True, text=True, env=env, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        assert read(back) == (tree if k == 0 else {rel: v for rel, v in tree.items() if rel != victim})
        if k == 1:
            # a damaged file among them: reported, the rest comes back
            bad = os.path.join(out, sorted(tree)[5] + ".knz")
            blob = bytearray(open(bad, "rb").read())
            blob[len(blob) // 2] ^= 0x10
            open(bad, "wb").write(bytes(blob[:len(blob) - 3]))
            r = subprocess.run([cli, "-d", "-i", out, "-o", back, "-f"], capture_output=True, text=True, env=env, timeout=600)
            assert r.returncode != 0 and bad in r.stderr and "28 of 29" in r.stderr, r.stderr[-2000:]
        shutil.rmtree(out)
        shutil.rmtree(back)
    # an input that cannot be read: reported by name with ERR_OPEN_FILE, the others are written. (A process with the rights of root reads
    # a file of mode 000 like any other, and a path that is no regular file is not listed at all: there the case cannot be arranged and
    # is left out; the checks of this repository run as an ordinary user.)
    locked = str(tmp_path / "locked")
    os.makedirs(os.path.join(locked, "sub"))
    for nm, data in (("a.txt", b"first " * 50), (os.path.join("sub", "b.bin"), b"second " * 70), ("c.txt", b"third " * 90)):
        open(os.path.join(locked, nm), "wb").write(data)
    os.chmod(os.path.join(locked, "sub", "b.bin"), 0)
    if not os.access(os.path.join(locked, "sub", "b.bin"), os.R_OK):
        r = subprocess.run([cli, "-c", "-i", locked, "-o", str(tmp_path / "locked_out"), "-j", "1"] + CLI_ARGS[-1], capture_output=True, text=True, env=env, timeout=600)
        assert r.returncode == 10 and os.path.join(locked, "sub", "b.bin") in r.stderr and "2 of 3" in r.stderr, r.stderr[-2000:]
        assert set(read(str(tmp_path / "locked_out"), ".knz")) == {"a.txt", "c.txt"}
    os.chmod(os.path.join(locked, "sub", "b.bin"), 0o600)
    # beside the files: DIR/F.knz, and back after the originals are gone
    r = subprocess.run([cli, "-c", "-i", src, "-j", "1"] + CLI_ARGS[-1], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert {k: v for k, v in read(src, ".knz").items()}.keys() == tree.keys()
    for rel in tree:
        os.remove(os.path.join(src, rel))
    r = subprocess.run([cli, "-d", "-i", src], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert {k: v for k, v in read(src).items() if not k.endswith(".knz")} == tree
