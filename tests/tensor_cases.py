"""The cases of tests/test_gpu_tensors.py, which runs this file as a program in a process of its own: torch comes with a HIP runtime of its
own, which a process has to load before the device library, and a pytest process that has run other GPU tests has loaded the library
long ago. Every case_* function is one test; main() runs them up to the first that fails and prints one JSON object {case: "ok" or the
traceback}.

kanzi.TensorCodec: compress / decompress of tensors that live on the GPU. Every stream must be, byte for byte, what compress_many returns
for the tensor's bytes (which tests/test_gpu_streams.py ties to the unmodified reference), the way back must give the bytes, and nothing
of the payload's size may cross the bus in either direction."""
import importlib
import json
import os
import sys
import traceback

import torch                # first: see above

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np
import pytest

import knzlib
import vectors

LENGTHS = [0, 1, 15, 16, 17, 1023, 1024, 4096, 65535, 65536, 65537, 200000]
N_TENSORS = 300
CHAINS = [("BWT+RANK+ZRLT", "ANS0", 65536, 0), ("LZ", "HUFFMAN", 65536, 32)]
_cache = {}


def mods():
    import torch
    knzlib.load_pkg()
    return torch, importlib.import_module("kanzi_amd.kanzi"), importlib.import_module("kanzi_amd.hipapi")


def upload(torch, data):
    return torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda() if data else torch.empty(0, dtype=torch.uint8, device="cuda")


def corpus():
    """(host bytes, tensors): N_TENSORS tensors whose byte lengths go round LENGTHS, of four dtypes (where the length is a multiple of the
    element size), every seventh a uint8 view at an odd offset of a larger tensor; text-like, random and constant content. Made once."""
    if "corpus" not in _cache:
        torch, _, _ = mods()
        pools = [vectors.make(("text", 300000, 1)), vectors.make(("rand", 300000, 7)), b"\x07" * 300000]
        dtypes = [torch.uint8, torch.float16, torch.float32, torch.int64]
        rng = np.random.default_rng(12)
        host, tensors = [], []
        for i in range(N_TENSORS):
            n = LENGTHS[i % len(LENGTHS)]
            pool = pools[(i // len(LENGTHS)) % 3]
            at = int(rng.integers(0, len(pool) - n))
            data = pool[at:at + n]
            if i % 7 == 3:
                off = 2 * int(rng.integers(0, 50)) + 1
                t = upload(torch, bytes(off) + data + bytes(9))[off:off + n]
                assert n == 0 or t.data_ptr() % 2 == 1
            else:
                dt = dtypes[(i // 5) % 4]
                t = upload(torch, data)
                if n and n % dt.itemsize == 0:
                    t = t.view(dt)
            assert t.is_contiguous() and t.numel() * t.element_size() == n
            host.append(data)
            tensors.append(t)
        assert {t.dtype for t in tensors} == set(dtypes)
        _cache["corpus"] = (host, tensors)
    return _cache["corpus"]


def expected(chain):
    """compress_many's streams for the corpus: computed once per chain, never changed."""
    if chain not in _cache:
        _, kz, _ = mods()
        transform, entropy, bs, ck = chain
        _cache[chain] = kz.compress_many(corpus()[0], transform, entropy, bs, checksum=ck)
    return _cache[chain]


def streams_of(blob, offsets):
    raw = blob.cpu().numpy().tobytes()
    return [raw[offsets[k]:offsets[k + 1]] for k in range(len(offsets) - 1)]


def case_streams_equal_compress_many_and_come_back_bwt_ans0():
    streams_equal_compress_many_and_come_back(CHAINS[0])


def case_streams_equal_compress_many_and_come_back_lz_huffman():
    streams_equal_compress_many_and_come_back(CHAINS[1])


def streams_equal_compress_many_and_come_back(chain):
    torch, kz, _ = mods()
    host, tensors = corpus()
    transform, entropy, bs, ck = chain
    with kz.TensorCodec() as codec:
        blob, offsets = codec.compress(tensors, transform, entropy, bs, checksum=ck)
        assert blob.dtype == torch.uint8 and blob.dim() == 1 and blob.is_cuda
        assert len(offsets) == len(tensors) + 1 and offsets[0] == 0 and offsets[-1] == blob.numel()
        got, want = streams_of(blob, offsets), expected(chain)
        for k in range(len(tensors)):
            assert got[k] == want[k], "stream %d (%d bytes) differs from compress_many's" % (k, len(host[k]))
        back = codec.decompress(blob, offsets)
    assert len(back) == len(tensors)
    for k, t in enumerate(back):
        assert t.dtype == torch.uint8 and t.is_cuda and t.data_ptr() % 16 == 0, k
        assert t.cpu().numpy().tobytes() == host[k], k
    k = next(k for k, t in enumerate(tensors) if t.dtype == torch.float32)
    assert torch.equal(back[k].view(torch.float32).view(torch.uint8), tensors[k].view(torch.uint8))
    # the one-shot wrappers
    blob2, offsets2 = kz.compress_tensors(tensors[:20], transform, entropy, bs, checksum=ck)
    assert streams_of(blob2, offsets2) == want[:20]
    assert [t.cpu().numpy().tobytes() for t in kz.decompress_tensors(blob2, offsets2)] == host[:20]


def case_empty_list():
    torch, kz, _ = mods()
    with kz.TensorCodec() as codec:
        blob, offsets = codec.compress([], "LZ", "HUFFMAN", 65536)
        assert blob.numel() == 0 and blob.dtype == torch.uint8 and blob.is_cuda and offsets == [0]
        assert codec.decompress(blob, offsets) == []


def case_several_device_calls_give_the_same_blob():
    with pytest.MonkeyPatch.context() as monkeypatch:
        _several_device_calls_give_the_same_blob(monkeypatch)


def _several_device_calls_give_the_same_blob(monkeypatch):
    torch, kz, hipapi = mods()
    _, tensors = corpus()
    transform, entropy, bs, ck = CHAINS[1]
    calls = []
    real = hipapi.Context.encode_streams
    monkeypatch.setattr(hipapi.Context, "encode_streams", lambda self, p, d_in, items, *a, **k: (calls.append(len(items)), real(self, p, d_in, items, *a, **k))[1])
    with kz.TensorCodec() as codec:
        blob, offsets = codec.compress(tensors, transform, entropy, bs, checksum=ck)
        assert calls == [N_TENSORS]
        del calls[:]
        monkeypatch.setattr(hipapi, "STREAMS_MAX_ITEMS", 64)
        blob5, offsets5 = codec.compress(tensors, transform, entropy, bs, checksum=ck)
        assert calls == [64, 64, 64, 64, N_TENSORS - 256]
        assert offsets5 == offsets and torch.equal(blob5, blob)
        back = codec.decompress(blob5, offsets5)
    assert all(torch.equal(b, t.view(torch.uint8).reshape(-1)) for b, t in zip(back, tensors))


def case_nothing_of_the_payloads_size_crosses_the_bus():
    with pytest.MonkeyPatch.context() as monkeypatch:
        _nothing_of_the_payloads_size_crosses_the_bus(monkeypatch)


def _nothing_of_the_payloads_size_crosses_the_bus(monkeypatch):
    torch, kz, hipapi = mods()
    _, tensors = corpus()
    moved = {"h2d": 0, "d2h": 0}
    real_h2d, real_d2h = hipapi.Context.h2d, hipapi.Context.d2h
    monkeypatch.setattr(hipapi.Context, "h2d", lambda self, dptr, data: (moved.__setitem__("h2d", moved["h2d"] + len(data)), real_h2d(self, dptr, data))[1])
    monkeypatch.setattr(hipapi.Context, "d2h", lambda self, dptr, n: (moved.__setitem__("d2h", moved["d2h"] + n), real_d2h(self, dptr, n))[1])
    transform, entropy, bs, ck = CHAINS[0]
    with kz.TensorCodec() as codec:
        blob, offsets = codec.compress(tensors, transform, entropy, bs, checksum=ck)
        assert moved == {"h2d": 0, "d2h": 0}
        back = codec.decompress(blob, offsets)
        assert moved["h2d"] == 0 and 0 < moved["d2h"] <= 32 * len(tensors)
    assert sum(t.numel() for t in back) == sum(t.numel() * t.element_size() for t in tensors) > 32 * len(tensors)


def case_streams_of_different_headers_in_one_call():
    torch, kz, _ = mods()
    host, tensors = corpus()
    picks = [k for k, h in enumerate(host) if 0 < len(h) <= 4096][:24]
    with kz.TensorCodec() as codec:
        parts = []                                   # (stream bytes, the bytes it stands for)
        for j, (transform, entropy, bs) in enumerate((("LZ", "HUFFMAN", 65536), ("BWT+RANK+ZRLT", "ANS0", 65536), ("LZ", "HUFFMAN", 1024), ("BWT+RANK+ZRLT", "ANS0", 1024))):
            mine = picks[j::4]
            blob, offsets = codec.compress([tensors[k] for k in mine], transform, entropy, bs)
            parts.append(list(zip(streams_of(blob, offsets), [host[k] for k in mine])))
        mixed = [parts[j][i] for i in range(6) for j in range(4)]                # interleaved
        mixed.insert(5, (kz.compress_many([host[picks[0]]], "RLT", "FPAQ", 4096)[0], host[picks[0]]))      # written on the host
        blob = upload(torch, b"".join(s for s, _ in mixed))
        offsets = [0]
        for s, _ in mixed:
            offsets.append(offsets[-1] + len(s))
        back = codec.decompress(blob, offsets)
    assert [t.cpu().numpy().tobytes() for t in back] == [d for _, d in mixed]
    assert all(t.data_ptr() % 16 == 0 for t in back)


def case_a_damaged_stream_is_named():
    torch, kz, _ = mods()
    host, tensors = corpus()
    picks = [k for k, h in enumerate(host) if len(h) == 1024][:8]          # one block each: the middle of a stream is payload
    with kz.TensorCodec() as codec:
        blob, offsets = codec.compress([tensors[k] for k in picks], "NONE", "NONE", 1024, checksum=32)     # (a flipped byte of a stored block is exactly a checksum mismatch)
        bad = blob.clone()
        bad[(offsets[3] + offsets[4]) // 2] ^= 0x10
        with pytest.raises(kz.KanziError, match="stream 3:") as e:
            codec.decompress(bad, offsets)
        assert e.value.code == 19
        bad = blob.clone()
        bad[offsets[5] + 1] ^= 0x10
        with pytest.raises(kz.KanziError, match="stream 5: Invalid stream type") as e:
            codec.decompress(bad, offsets)
        assert e.value.code == 15
        # the same call without the damaged stream, on the same codec
        keep = [k for k in range(len(picks)) if k != 5]
        good = torch.cat([bad[offsets[k]:offsets[k + 1]] for k in keep])
        offs = [0]
        for k in keep:
            offs.append(offs[-1] + offsets[k + 1] - offsets[k])
        back = codec.decompress(good, offs)
    assert [t.cpu().numpy().tobytes() for t in back] == [host[picks[k]] for k in keep]


def case_inputs_made_on_the_codecs_stream_need_no_synchronisation():
    torch, kz, _ = mods()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        inputs = [torch.randint(0, 256, (n,), dtype=torch.uint8, device="cuda") for n in (100000, 17, 65536, 4097)]
        inputs.append(torch.randint(-1000, 1000, (5000,), dtype=torch.int64, device="cuda"))
        with kz.TensorCodec() as codec:
            assert codec.stream == s
            blob, offsets = codec.compress(inputs, "LZ", "HUFFMAN", 65536, checksum=32)
            back = codec.decompress(blob, offsets)
        same = [torch.equal(b, t.view(torch.uint8)) for b, t in zip(back, inputs)]
    assert same == [True] * len(inputs)


def case_one_codec_many_calls_then_closed():
    torch, kz, _ = mods()
    host, tensors = corpus()
    codec = kz.TensorCodec()
    small, _ = codec.compress(tensors[:12], "LZ", "HUFFMAN", 65536)
    large, offsets = codec.compress(tensors[:120], "LZ", "HUFFMAN", 65536)
    assert small.numel() < large.numel()
    assert streams_of(large, offsets) == kz.compress_many(host[:120], "LZ", "HUFFMAN", 65536)
    codec.close()
    codec.close()
    with pytest.raises(RuntimeError, match="closed"):
        codec.compress(tensors[:2], "LZ", "HUFFMAN", 65536)
    with pytest.raises(RuntimeError, match="closed"):
        codec.decompress(large, offsets)


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
