"""The stage cases of tests/entropy_edge_cases.py of at most 2 * 16 KiB + 1 bytes on the kernels themselves, compiled as plain C++
against the fiber emulation (tests/test_emu_kernels.py): the decoders of ANS0, HUFFMAN and ANS1 on the oracle's streams, the
encoders with the bit assembly bit for bit against the oracle, and FPAQ both ways with sub-chunks of 4 KiB, so that their borders
fall inside these sizes. What the oracle writes for these inputs is the reference's (tests/test_entropy_edges.py)."""
import os
import subprocess

import pytest

import entropy_edge_cases as eec
import knzlib
from test_emu_kernels import EMU, ROOT, build, write_case


def blocks(keep=lambda name: True):
    return [data for name, data, prop in eec.stage_cases() if len(data) <= eec.EMU_MAX and keep(name)]


def run(exe, path, timeout=1500):
    r = subprocess.run([exe, path], capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]


def fewer_placements(name):
    """Of the alphabet placements the drawn one, with the lowest and the highest byte values for the sizes around the change of the
    frequency groups and the only one there is at 256 symbols."""
    p = name.split(":")
    return p[0] != "asz" or p[2] == "random" or p[1] in ("63", "64", "65", "256")


@pytest.mark.parametrize("harness", ["ans0_emu", "ans0_enc_emu", "huff_emu", "huff_enc_emu"])
def test_order0_and_huffman_kernels_on_the_edge_cases_emulated(tmp_path, harness):
    """The decoders take every placement of every alphabet size; the encoders, which cost the emulator more per chunk, fewer."""
    exe = build(harness, tmp_path)
    path = str(tmp_path / "edges.bin")
    write_case(path, blocks(fewer_placements if harness == "ans0_enc_emu" else lambda name: True))
    run(exe, path)


@pytest.mark.parametrize("harness", ["ans1_emu", "ans1_enc_emu"])
def test_order1_kernels_on_the_edge_cases_emulated(tmp_path, harness):
    """Fewer placements: an order-1 chunk costs the emulator 256 contexts whatever its length. The encoder takes the blocks of 4 MiB
    + 1, + 2 and + 3 bytes as well, whatever their size: an order-1 chunk of fewer than 4 bytes exists only behind a chunk of 4 MiB.
    (What these found: k_ans1_encode left the four states of such a chunk at their start value, where the reference codes the byte in
    front of the chunk once into each.)"""
    exe = build(harness, tmp_path)
    path = str(tmp_path / "edges.bin")
    write_case(path, blocks(fewer_placements))
    run(exe, path)
    if harness == "ans1_enc_emu":
        write_case(path, [data for name, data, prop in eec.stage_cases() if name in ["m4:%d" % (eec.M4 + k) for k in (1, 2, 3)]])
        run(exe, path)


def test_fpaq_kernels_on_the_edge_cases_emulated(tmp_path):
    """Kernels and a private copy of the oracle's sources built with sub-chunks of 4 KiB instead of 4 MiB: the lengths around 4,096
    and 16,384 are lengths around one and four sub-chunks. FPAQ does not look at the alphabet: the length cases only, in three
    runs, because the harness sizes its staging area by blocks times the sub-chunks of the longest block."""
    objs = []
    for src in sorted(os.listdir(os.path.join(ROOT, "oracle"))):
        if src.endswith(".c"):
            obj = str(tmp_path / (src[:-2] + ".o"))
            subprocess.check_call(["gcc", "-O2", "-std=c99", "-fPIC", "-DFPAQ_CHUNK=4096u", "-c", os.path.join(ROOT, "oracle", src), "-o", obj])
            objs.append(obj)
    exe = str(tmp_path / "fpaq_emu_small")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-x", "c++", "-DKNZ_EMU_FPAQ_CHUNK=4096u", "-I" + os.path.join(ROOT, "tools", "hipemu"),
                           "-I" + os.path.join(ROOT, "include"), "-Wno-unused-value", "-Wno-attributes", "-Wno-format-extra-args",
                           os.path.join(EMU, "fpaq_emu.cpp"), os.path.join(ROOT, "tools", "hipemu", "hipemu.cpp"), "-x", "none"] + objs + ["-o", exe])
    lens = blocks(lambda name: name.startswith("len:"))
    for i, group in enumerate(([d for d in lens if len(d) <= 4097], [d for d in lens if 4097 < len(d) <= eec.CH + 33], [d for d in lens if len(d) > eec.CH + 33])):
        assert group
        path = str(tmp_path / ("edges%d.bin" % i))
        write_case(path, group)
        run(exe, path)
