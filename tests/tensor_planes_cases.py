"""The cases of tests/test_gpu_tensor_planes.py, which runs this file as a program in a process of its own for the reason given in
tests/tensor_cases.py (torch's HIP runtime has to be loaded before the device library). Every case_* function is one test; main() runs
them up to the first that fails and prints one JSON object {case: "ok" or the traceback}.

kanzi.TensorCodec with byte planes: compress(planes=...) must give, byte for byte, compress_many's stream for kanzi.split_bytes of the
tensor's bytes (split_bytes is plain numpy, compress_many is tied to the unmodified reference by tests/test_gpu_streams.py), and
decompress(planes=widths) must give the tensor's bytes back."""
import importlib
import json
import os
import sys
import traceback

import torch                # first: see above

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import pytest

import knzlib

COUNTS = [0, 1, 7, 4099]
CHAINS = [("NONE", "HUFFMAN", 65536), ("BWT+RANK+ZRLT", "ANS0", 65536)]
_cache = {}


def mods():
    knzlib.load_pkg()
    return importlib.import_module("kanzi_amd.kanzi"), importlib.import_module("kanzi_amd.hipapi")


def raw(t):
    """The tensor's bytes in memory order."""
    return t.contiguous().view(-1).view(torch.uint8).cpu().numpy().tobytes() if t.numel() else b""


def corpus():
    """(tensors on the GPU, their bytes, their widths): seven dtypes at every count of COUNTS, each also as the contiguous slice [1:] of a
    tensor one element longer, whose storage starts one element (1 to 8 bytes) off the allocation's boundary; some NaNs and infinities
    among the floating-point values. Made once, on the CPU from a seed."""
    if "corpus" not in _cache:
        g = torch.Generator().manual_seed(20)
        tensors, widths = [], []
        for dtype, width in [(torch.bfloat16, 2), (torch.float16, 2), (torch.float32, 4), (torch.float64, 8), (torch.int8, 1), (torch.bool, 1), (torch.complex64, 4)]:
            for n in COUNTS:
                for sliced in (False, True):
                    k = n + 1 if sliced else n
                    if dtype == torch.int8:
                        t = torch.randint(-128, 128, (k,), generator=g, dtype=torch.int8)
                    elif dtype == torch.bool:
                        t = torch.rand(k, generator=g) < 0.3
                    elif dtype == torch.complex64:
                        t = torch.complex(torch.randn(k, generator=g) * 0.02, torch.randn(k, generator=g))
                    else:
                        t = torch.randn(k, generator=g, dtype=torch.float64) * 0.02
                        if k > 5:
                            t[2], t[3], t[5] = float("nan"), float("inf"), -float("nan")
                        t = t.to(dtype)
                    t = t.cuda()
                    if sliced:
                        t = t[1:]
                        assert t.is_contiguous() and (t.data_ptr() % 16 == t.element_size() or n == 0)
                    assert t.numel() == n
                    tensors.append(t)
                    widths.append(width)
        _cache["corpus"] = (tensors, [raw(t) for t in tensors], widths)
    return _cache["corpus"]


def expected(chain, split):
    """compress_many's streams for the corpus's bytes, split into planes on the host or as they are: computed once, never changed."""
    if (chain, split) not in _cache:
        kz, _ = mods()
        _, host, widths = corpus()
        _cache[(chain, split)] = kz.compress_many([kz.split_bytes(b, w) if split else b for b, w in zip(host, widths)], *chain)
    return _cache[(chain, split)]


def streams_of(blob, offsets):
    data = blob.cpu().numpy().tobytes()
    return [data[offsets[k]:offsets[k + 1]] for k in range(len(offsets) - 1)]


def case_planes_streams_equal_compress_many_of_split_bytes_none_huffman():
    planes_streams_equal_compress_many_of_split_bytes(CHAINS[0])


def case_planes_streams_equal_compress_many_of_split_bytes_bwt_ans0():
    planes_streams_equal_compress_many_of_split_bytes(CHAINS[1])


def planes_streams_equal_compress_many_of_split_bytes(chain):
    kz, _ = mods()
    tensors, host, widths = corpus()
    with kz.TensorCodec() as codec:
        blob, offsets = codec.compress(tensors, *chain, planes=True)
        assert len(offsets) == len(tensors) + 1 and offsets[-1] == blob.numel()
        got, want = streams_of(blob, offsets), expected(chain, True)
        for k, t in enumerate(tensors):
            assert got[k] == want[k], "stream %d (%s, %d elements) differs from compress_many's of the split bytes" % (k, t.dtype, t.numel())
        back = codec.decompress(blob, offsets, planes=widths)
        # without the widths the streams decode to the planes
        flat = codec.decompress(blob, offsets)
    assert len(back) == len(tensors)
    for k, t in enumerate(tensors):
        assert back[k].dtype == torch.uint8 and back[k].is_cuda and back[k].data_ptr() % 16 == 0, k
        assert back[k].cpu().numpy().tobytes() == host[k], "tensor %d (%s, %d elements) does not come back" % (k, t.dtype, t.numel())       # (as bytes: NaNs count)
        assert flat[k].cpu().numpy().tobytes() == kz.split_bytes(host[k], widths[k]), k
        if t.numel():
            assert torch.equal(back[k].view(t.dtype).view(torch.uint8), t.view(torch.uint8))
    # the one-shot wrappers pass the arguments through
    blob2, offsets2 = kz.compress_tensors(tensors[:16], *chain, planes=True)
    assert streams_of(blob2, offsets2) == want[:16]
    assert [t.cpu().numpy().tobytes() for t in kz.decompress_tensors(blob2, offsets2, planes=widths[:16])] == host[:16]


def case_without_planes_nothing_changes():
    kz, _ = mods()
    tensors, host, widths = corpus()
    with kz.TensorCodec() as codec:
        for chain in CHAINS:
            blob, offsets = codec.compress(tensors, *chain)
            assert streams_of(blob, offsets) == expected(chain, False)
            for planes in (False, None, [1] * len(tensors)):                # (planes of one byte are the bytes themselves)
                blob2, offsets2 = codec.compress(tensors, *chain, planes=planes)
                assert offsets2 == offsets and torch.equal(blob2, blob), planes
            assert expected(chain, False) != expected(chain, True)
        back = codec.decompress(blob, offsets, planes=None)
        ones = codec.decompress(blob, offsets, planes=[1] * len(tensors))
    assert [t.cpu().numpy().tobytes() for t in back] == host and [t.cpu().numpy().tobytes() for t in ones] == host


def case_explicit_widths_on_uint8_tensors():
    kz, _ = mods()
    tensors, host, widths = corpus()
    chain = CHAINS[0]
    as_bytes = [t.view(-1).view(torch.uint8) if t.numel() else torch.empty(0, dtype=torch.uint8, device="cuda") for t in tensors]
    assert all(t.dtype == torch.uint8 for t in as_bytes)
    with kz.TensorCodec() as codec:
        blob, offsets = codec.compress(as_bytes, *chain, planes=widths)
        assert streams_of(blob, offsets) == expected(chain, True)
        # other widths than the dtype's: bf16 pairs as 4-byte elements
        k = next(k for k, t in enumerate(tensors) if t.dtype == torch.bfloat16 and t.numel() == 4099)
        pair = tensors[k][1:]                                              # 4098 values, 8196 bytes
        blob4, offsets4 = codec.compress([pair, pair], *chain, planes=[4, 2])
        assert streams_of(blob4, offsets4) == kz.compress_many([kz.split_bytes(raw(pair), 4), kz.split_bytes(raw(pair), 2)], *chain)
        back = codec.decompress(blob4, offsets4, planes=(4, 2))
    assert torch.equal(back[0].view(torch.bfloat16).view(torch.uint8), pair.view(torch.uint8)) and torch.equal(back[0], back[1])


def case_a_width_that_does_not_divide_the_length_is_refused_on_both_sides():
    kz, _ = mods()
    seven = torch.arange(7, dtype=torch.uint8, device="cuda")
    six = torch.arange(6, dtype=torch.uint8, device="cuda")
    with kz.TensorCodec() as codec:
        with pytest.raises(ValueError, match="tensor 1: 7 bytes are no multiple of the width 2"):
            codec.compress([six, seven], "NONE", "HUFFMAN", 65536, planes=[2, 2])
        with pytest.raises(ValueError, match="tensor 0: width 3"):
            codec.compress([six, seven], "NONE", "HUFFMAN", 65536, planes=[3, 1])
        blob, offsets = codec.compress([six, seven], "NONE", "HUFFMAN", 65536)
        with pytest.raises(ValueError, match="stream 1: 7 decoded bytes are no multiple of the width 4"):
            codec.decompress(blob, offsets, planes=[2, 4])
        with pytest.raises(ValueError, match="stream 0: width 5"):
            codec.decompress(blob, offsets, planes=[5, 1])
        with pytest.raises(ValueError, match="planes holds 1 widths for 2 streams"):
            codec.decompress(blob, offsets, planes=[2])
        # the codec is as usable as before
        back = codec.decompress(blob, offsets, planes=[2, 1])
    assert back[0].cpu().numpy().tobytes() == kz.join_bytes(bytes(range(6)), 2) and back[1].cpu().numpy().tobytes() == bytes(range(7))


def case_split_bf16_weights_are_smaller_under_huffman():
    """65,536 bf16 values of N(0, 0.02) under NONE / HUFFMAN: as they lie, the order-0 entropy of their bytes is 6.21 bits per byte, which
    no order-0 code gets below; split, the two planes fall into separate 16 KiB chunks with tables of their own, 7.97 and 2.68 bits per
    byte, and a Huffman code is within one bit of the entropy: at most (8 + 2.68 + 1) / 2 = 5.85 bits per byte and the tables."""
    kz, _ = mods()
    g = torch.Generator().manual_seed(21)
    t = (torch.randn(65536, generator=g) * 0.02).to(torch.bfloat16).cuda()
    with kz.TensorCodec() as codec:
        _, plain = codec.compress([t], "NONE", "HUFFMAN", 65536)
        blob, split = codec.compress([t], "NONE", "HUFFMAN", 65536, planes=True)
        back = codec.decompress(blob, split, planes=[2])
    print("bf16 N(0, 0.02), 131072 bytes, NONE / HUFFMAN: %d bytes as they lie, %d bytes as planes" % (plain[1], split[1]))
    assert split[1] < plain[1]
    assert torch.equal(back[0].view(torch.bfloat16).view(torch.uint8), t.view(torch.uint8))


def case_z_streams_that_go_through_the_host_are_joined_too():
    with pytest.MonkeyPatch.context() as monkeypatch:
        _streams_that_go_through_the_host_are_joined_too(monkeypatch)


def _streams_that_go_through_the_host_are_joined_too(monkeypatch):
    kz, _ = mods()
    tensors, host, widths = corpus()
    chain = CHAINS[0]
    with kz.TensorCodec() as codec:
        blob, offsets = codec.compress(tensors, *chain, planes=True)
        real, asked = kz._fits_one_call, []
        # every stream of more than 1000 bytes is taken for one that a device call does not hold
        monkeypatch.setattr(kz, "_fits_one_call", lambda n, bs, hipapi: (asked.append(n), n <= 1000 and real(n, bs, hipapi))[1])
        back = codec.decompress(blob, offsets, planes=widths)
        assert any(n > 1000 for n in asked)
        with pytest.raises(ValueError, match="stream 0: 8198 decoded bytes are no multiple of the width 4"):
            k = next(k for k, t in enumerate(tensors) if t.dtype == torch.bfloat16 and t.numel() == 4099)
            codec.decompress(blob[offsets[k]:offsets[k + 1]].clone(), [0, offsets[k + 1] - offsets[k]], planes=[4])
    for k, t in enumerate(tensors):
        assert back[k].data_ptr() % 16 == 0 and back[k].cpu().numpy().tobytes() == host[k], "tensor %d (%s, %d elements) does not come back" % (k, t.dtype, t.numel())


CASES = sorted(k for k in globals() if k.startswith("case_"))


def main():
    res, failed = {}, None
    for name in CASES:
        if failed:                                 # (nothing more is started on a device that may have faulted)
            res[name] = "not run: %s failed before" % failed
            continue
        try:
            globals()[name]()
            res[name] = "ok"
        except BaseException:
            res[name], failed = traceback.format_exc(), name
    print("RESULTS " + json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
