"""kanzi.compress_tensors refuses what it will not silently repair -- a tensor on the CPU, one that is not contiguous, something that is no
tensor -- by index and before the device library is loaded; and kanzi.py itself needs no torch to be imported."""
import importlib
import sys

import pytest

import knzlib


def test_bad_tensors_are_refused_by_index_before_the_device_library_loads(monkeypatch):
    import torch
    knzlib.load_pkg()
    kz, hipapi = importlib.import_module("kanzi_amd.kanzi"), importlib.import_module("kanzi_amd.hipapi")
    monkeypatch.setattr(hipapi, "lib", lambda: pytest.fail("the device library was asked for"))
    monkeypatch.setattr(hipapi.Context, "__init__", lambda self, *a, **k: pytest.fail("a device context was made"))
    good = torch.zeros(16, dtype=torch.uint8)
    with pytest.raises(ValueError, match="tensor 0 is on cpu"):
        kz.compress_tensors([good], "LZ", "HUFFMAN", 65536)
    with pytest.raises(ValueError, match="tensor 1 is not contiguous"):
        kz.compress_tensors([good, torch.zeros(4, 4).t()], "LZ", "HUFFMAN", 65536)
    with pytest.raises(ValueError, match="tensor 2 is no torch.Tensor but bytes"):
        kz.compress_tensors([good, good, b"bytes"], "LZ", "HUFFMAN", 65536)
    with pytest.raises(ValueError, match="tensor 0 is no torch.Tensor but ndarray"):
        kz.compress_tensors([good.numpy()], "LZ", "HUFFMAN", 65536)


def test_kanzi_module_imports_without_torch(monkeypatch):
    knzlib.load_pkg()
    for name in [m for m in sys.modules if m == "torch" or m.startswith("torch.")]:
        monkeypatch.delitem(sys.modules, name)
    monkeypatch.setitem(sys.modules, "torch", None)              # `import torch` now raises ImportError
    monkeypatch.delitem(sys.modules, "kanzi_amd.kanzi", raising=False)
    with pytest.raises(ImportError):
        importlib.import_module("torch")
    kz = importlib.import_module("kanzi_amd.kanzi")
    assert hasattr(kz, "TensorCodec") and hasattr(kz, "compress_many")
    with pytest.raises(ImportError):
        kz.compress_tensors([], "LZ", "HUFFMAN", 65536)
