"""The CLI's directory mode and the C++ batch pair against the real device library: the checks of tests/test_host_streams_stub.py, where
the pair now reaches the device many files per call."""
import os
import subprocess

import pytest

import knzlib
import stream_tree

pytestmark = pytest.mark.gpu


def test_directory_mode_on_the_device(tmp_path):
    cli = os.environ.get("KNZ_TEST_CLI", os.path.join(knzlib.PKG, "kanzi_amd_cli"))
    assert os.path.exists(cli), "run __graft_entry__.build() first"
    ref = knzlib.REF_BIN if os.path.exists(knzlib.REF_BIN) else None
    stream_tree.check_directory_mode(cli, tmp_path, ref)


def test_pair_batches_on_the_device(tmp_path):
    exe = str(tmp_path / "streams_pair_test")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-I" + os.path.join(knzlib.ROOT, "include"), "-o", exe,
                           os.path.join(knzlib.ROOT, "tests", "cpp", "streams_pair_test.cpp"), "-L" + knzlib.PKG, "-lkanzi_amd", "-lknz_hip",
                           "-Wl,-rpath," + knzlib.PKG])
    for args in (["BWT+RANK+ZRLT", "ANS0", "4096", "32"], ["LZX", "HUFFMAN", "1024", "0"], ["LZP", "CM", "1024", "0"]):
        r = subprocess.run([exe] + args, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and "OK 40" in r.stdout and "batched 1" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


def test_directory_of_many_small_files_with_the_default_block_size(tmp_path):
    """650 files of at most 2,000 bytes through -c -i DIR and -d -i DIR with the default -b (4 MiB): a tree that one device call
    compresses must be a tree that one device call gives back, whatever the block size of the streams' format is."""
    import hashlib
    import numpy as np
    import vectors
    cli = os.environ.get("KNZ_TEST_CLI", os.path.join(knzlib.PKG, "kanzi_amd_cli"))
    src, out, back = str(tmp_path / "src"), str(tmp_path / "out"), str(tmp_path / "back")
    rng = np.random.default_rng(17)
    pool = vectors.make(("mixed", 300000, 5))
    tree = {}
    for i in range(650):
        n = int(rng.integers(0, 2001))
        at = int(rng.integers(0, len(pool) - n))
        tree[os.path.join("d%02d" % (i % 13), "f%03d.bin" % i)] = pool[at:at + n]
    for rel, data in tree.items():
        os.makedirs(os.path.dirname(os.path.join(src, rel)), exist_ok=True)
        open(os.path.join(src, rel), "wb").write(data)
    args = ["-t", "LZX", "-e", "HUFFMAN"]
    r = subprocess.run([cli, "-c", "-i", src, "-o", out, "-j", "1"] + args, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "650 of 650" in r.stderr, r.stderr[-2000:]
    r = subprocess.run([cli, "-d", "-i", out, "-o", back], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "650 of 650" in r.stderr, r.stderr[-2000:]
    assert stream_tree.read(back) == tree
    if os.path.exists(knzlib.REF_BIN):
        one = str(tmp_path / "one.knz")
        for rel in sorted(tree)[::130]:
            subprocess.check_call([knzlib.REF_BIN, "-c", "-i", os.path.join(src, rel), "-o", one, "-f", "-j", "1", "-v", "0"] + args)
            assert hashlib.md5(open(one, "rb").read()).digest() == hashlib.md5(open(os.path.join(out, rel + ".knz"), "rb").read()).digest(), rel
    # --from / --to belong to one file
    r = subprocess.run([cli, "-d", "-i", out, "-o", back, "-f", "--from=2"], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "not with a directory" in r.stderr
