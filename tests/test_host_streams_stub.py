"""The host layer's batch pair and the CLI's directory mode on the CPU, against the stand-in device library (tests/stub/knz_hip_stub.c),
which has no knz_hip_encode_streams / knz_hip_decode_streams: the pair takes its fall-back -- one stream class per item -- and has to
write the same bytes. tests/test_gpu_streams_cli.py runs the same checks against the real device library."""
import os
import subprocess

import knzlib
import stream_tree
from test_host_stub import build_stub

ROOT = knzlib.ROOT
_built = {}


def stub(tmp_path_factory):
    if not _built:
        tmp = tmp_path_factory.mktemp("streams_stub")
        lib, _, cli = build_stub(tmp)
        _built.update(lib=lib, cli=cli, tmp=tmp)
    return _built


def test_directory_mode_against_stub(tmp_path, tmp_path_factory):
    s = stub(tmp_path_factory)
    ref = knzlib.REF_BIN if knzlib.ensure_ref() is not None and os.path.exists(knzlib.REF_BIN) else None
    stream_tree.check_directory_mode(s["cli"], tmp_path, ref)


def test_pair_falls_back_against_stub(tmp_path, tmp_path_factory):
    s = stub(tmp_path_factory)
    ora = os.path.join(ROOT, "oracle")
    exe = str(tmp_path / "streams_pair_test_stub")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-I" + os.path.join(ROOT, "include"), "-o", exe, os.path.join(ROOT, "tests", "cpp", "streams_pair_test.cpp"),
                           s["lib"], "-Wl,-rpath," + str(s["tmp"]), "-L" + ora, "-lknz_oracle", "-Wl,-rpath," + ora])
    for args in (["BWT+RANK+ZRLT", "ANS0", "4096", "32"], ["LZX", "HUFFMAN", "1024", "0"]):
        r = subprocess.run([exe] + args, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0 and "OK 40" in r.stdout and "batched 0" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
