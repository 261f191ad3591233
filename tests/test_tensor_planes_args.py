"""kanzi.split_bytes / join_bytes, the host form and the specification of the byte-plane kernels, against an example written out by hand
and as inverses of each other; and the ValueErrors of the `planes` argument of kanzi.compress_tensors, by index and before the device
library is loaded."""
import importlib

import numpy as np
import pytest

import knzlib


def kanzi():
    knzlib.load_pkg()
    return importlib.import_module("kanzi_amd.kanzi")


def test_split_and_join_a_hand_written_example():
    kz = kanzi()
    data = bytes([0x10, 0x11, 0x12, 0x13, 0x20, 0x21, 0x22, 0x23, 0x30, 0x31, 0x32, 0x33, 0x40, 0x41, 0x42, 0x43])
    assert kz.split_bytes(data, 1) == data
    assert kz.split_bytes(data, 2) == bytes([0x10, 0x12, 0x20, 0x22, 0x30, 0x32, 0x40, 0x42, 0x11, 0x13, 0x21, 0x23, 0x31, 0x33, 0x41, 0x43])
    assert kz.split_bytes(data, 4) == bytes([0x10, 0x20, 0x30, 0x40, 0x11, 0x21, 0x31, 0x41, 0x12, 0x22, 0x32, 0x42, 0x13, 0x23, 0x33, 0x43])
    assert kz.split_bytes(data, 8) == bytes([0x10, 0x30, 0x11, 0x31, 0x12, 0x32, 0x13, 0x33, 0x20, 0x40, 0x21, 0x41, 0x22, 0x42, 0x23, 0x43])
    assert kz.join_bytes(bytes([1, 2, 3, 0xA, 0xB, 0xC]), 2) == bytes([1, 0xA, 2, 0xB, 3, 0xC])
    # the definition, index by index
    data = bytes(range(200, 224))
    for w in (1, 2, 4, 8):
        m, s = len(data) // w, kz.split_bytes(data, w)
        assert all(s[k * m + i] == data[i * w + k] for i in range(m) for k in range(w))


@pytest.mark.parametrize("width", [1, 2, 4, 8])
def test_split_and_join_are_inverses(width):
    kz = kanzi()
    rng = np.random.default_rng(width)
    for m in (0, 1, 2, 15, 16, 17, 1000):
        data = rng.integers(0, 256, size=m * width, dtype=np.uint8).tobytes()
        s = kz.split_bytes(data, width)
        assert isinstance(s, bytes) and len(s) == len(data)
        assert kz.join_bytes(s, width) == data and kz.split_bytes(kz.join_bytes(data, width), width) == data
        assert kz.split_bytes(bytearray(data), width) == s and kz.split_bytes(np.frombuffer(data, dtype=np.uint8), width) == s


def test_split_and_join_refuse_other_widths_and_ragged_lengths():
    kz = kanzi()
    for f in (kz.split_bytes, kz.join_bytes):
        for width in (0, 3, 16, -2):
            with pytest.raises(ValueError, match="width"):
                f(bytes(48), width)
        with pytest.raises(ValueError, match="7 bytes are no multiple of the width 2"):
            f(bytes(7), 2)


def test_planes_argument_is_checked_by_index_before_the_device_library_loads(monkeypatch):
    import torch
    kz, hipapi = kanzi(), importlib.import_module("kanzi_amd.hipapi")
    monkeypatch.setattr(hipapi, "lib", lambda: pytest.fail("the device library was asked for"))
    monkeypatch.setattr(hipapi.Context, "__init__", lambda self, *a, **k: pytest.fail("a device context was made"))
    raw = torch.zeros(24, dtype=torch.uint8)
    odd = torch.zeros(7, dtype=torch.uint8)
    with pytest.raises(ValueError, match="planes holds 1 widths for 2 tensors"):
        kz.compress_tensors([raw, raw], "NONE", "HUFFMAN", 65536, planes=[2])
    with pytest.raises(ValueError, match="tensor 1: width 3,"):
        kz.compress_tensors([raw, raw], "NONE", "HUFFMAN", 65536, planes=[2, 3])
    with pytest.raises(ValueError, match="tensor 0: width 16,"):
        kz.compress_tensors([raw, raw], "NONE", "HUFFMAN", 65536, planes=[16, 2])
    with pytest.raises(ValueError, match="tensor 1: width True,"):
        kz.compress_tensors([raw, raw], "NONE", "HUFFMAN", 65536, planes=[1, True])
    with pytest.raises(ValueError, match="tensor 2: 7 bytes are no multiple of the width 2"):
        kz.compress_tensors([raw, odd, odd], "NONE", "HUFFMAN", 65536, planes=[8, 1, 2])
    # what is no tensor, or not contiguous, is still named first; valid widths get as far as the tensors' place
    with pytest.raises(ValueError, match="tensor 1 is no torch.Tensor"):
        kz.compress_tensors([raw, b"x"], "NONE", "HUFFMAN", 65536, planes=True)
    for planes in (True, [4, 8], (w for w in (2, 1)), False):
        with pytest.raises(ValueError, match="tensor 0 is on cpu"):
            kz.compress_tensors([raw, raw], "NONE", "HUFFMAN", 65536, planes=planes)


def test_widths_come_from_the_dtype():
    import torch
    kz = kanzi()
    dtypes = [torch.bfloat16, torch.float16, torch.float32, torch.float64, torch.int8, torch.bool, torch.complex64, torch.complex128, torch.int64]
    assert kz._plane_widths([torch.zeros(3, dtype=d) for d in dtypes], True) == [2, 2, 4, 8, 1, 1, 4, 8, 8]
    assert kz._plane_widths([torch.zeros(3)], False) is None and kz._plane_widths([torch.zeros(3)], None) is None
