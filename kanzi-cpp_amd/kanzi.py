"""Compressor / Decompressor classes over the C API of libkanzi_amd.so.

Mirrors the reference's ctypes shim (src/api/kanzi_c_api.py:88-137 for the bindings,
src/api/kanzi.py for the two classes): same struct layouts, same call sequence
(init -> compress()/decompress() per block -> dispose). Only marshals data.

compress_many / decompress_many (near the end) are the batch form for many small independent buffers: they go over the device
C ABI directly (hipapi.Context.encode_streams / decode_streams) and framing.py, many buffers per device call. TensorCodec (at the end) is
the same for torch tensors that live on the GPU: the payload never leaves the device. torch is imported only there, on first use.
"""
import contextlib
import ctypes as C
import importlib
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libkanzi_amd.so")

C_API_SYMBOLS = ["getCompressorVersion", "initCompressor", "compress", "disposeCompressor",
                 "getDecompressorVersion", "initDecompressor", "decompress", "disposeDecompressor"]


class cData(C.Structure):
    _fields_ = [("transform", C.c_char * 64), ("entropy", C.c_char * 16), ("blockSize", C.c_size_t),
                ("jobs", C.c_uint), ("checksum", C.c_int), ("headerless", C.c_int)]


class dData(C.Structure):
    _fields_ = [("bufferSize", C.c_size_t), ("jobs", C.c_uint), ("headerless", C.c_int), ("transform", C.c_char * 64),
                ("entropy", C.c_char * 16), ("blockSize", C.c_uint), ("originalSize", C.c_size_t), ("checksum", C.c_int),
                ("bsVersion", C.c_int)]


_lib = None
_libc = None


def lib():
    global _lib, _libc
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError("libkanzi_amd.so not built: run __graft_entry__.build()")
        L = C.CDLL(LIB_PATH)
        L.getCompressorVersion.restype = C.c_uint
        L.getDecompressorVersion.restype = C.c_uint
        L.initCompressor.argtypes = [C.POINTER(cData), C.c_void_p, C.POINTER(C.c_void_p)]
        L.compress.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]
        L.disposeCompressor.argtypes = [C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]
        L.initDecompressor.argtypes = [C.POINTER(dData), C.c_void_p, C.POINTER(C.c_void_p)]
        L.decompress.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]
        L.disposeDecompressor.argtypes = [C.POINTER(C.c_void_p)]
        _lib = L
        _libc = C.CDLL(None)
        _libc.fopen.restype = C.c_void_p
        _libc.fopen.argtypes = [C.c_char_p, C.c_char_p]
        _libc.fclose.argtypes = [C.c_void_p]
    return _lib


class _PyBuffer(C.Structure):
    """Py_buffer (CPython's object.h): lets compress() hand the caller's own memory to the library, whatever
    bytes-like object it lives in (bytes, bytearray, memoryview, numpy array; read-only included), without a copy."""
    _fields_ = [("buf", C.c_void_p), ("obj", C.py_object), ("len", C.c_ssize_t), ("itemsize", C.c_ssize_t), ("readonly", C.c_int),
                ("ndim", C.c_int), ("format", C.c_char_p), ("shape", C.POINTER(C.c_ssize_t)), ("strides", C.POINTER(C.c_ssize_t)),
                ("suboffsets", C.POINTER(C.c_ssize_t)), ("internal", C.c_void_p)]


C.pythonapi.PyObject_GetBuffer.argtypes = [C.py_object, C.POINTER(_PyBuffer), C.c_int]
C.pythonapi.PyObject_GetBuffer.restype = C.c_int
C.pythonapi.PyBuffer_Release.argtypes = [C.POINTER(_PyBuffer)]
C.pythonapi.PyBuffer_Release.restype = None
C.pythonapi.PyBytes_FromStringAndSize.argtypes = [C.c_char_p, C.c_ssize_t]
C.pythonapi.PyBytes_FromStringAndSize.restype = C.py_object
C.pythonapi.PyBytes_AsString.argtypes = [C.py_object]
C.pythonapi.PyBytes_AsString.restype = C.c_void_p


class KanziError(RuntimeError):
    def __init__(self, code, what):
        super().__init__("%s failed with kanzi error %d" % (what, code))
        self.code = code


def _name(v):
    """Codec names arrive as str or, as in the reference's shim (src/api/kanzi.py), as bytes."""
    if isinstance(v, (bytes, bytearray)):
        return bytes(v)
    if isinstance(v, str):
        return v.encode()
    raise TypeError("codec name must be str or bytes, not %s" % type(v).__name__)


class Compressor:
    """src/api/kanzi.py Compressor: same positional/keyword arguments, `compress(data)`, `close()`, context manager."""

    def __init__(self, path, transform="NONE", entropy="NONE", block_size=4 << 20, jobs=1, checksum=0, headerless=False):
        L = lib()
        tname, ename = _name(transform), _name(entropy)
        self._f = _libc.fopen(os.fsencode(path), b"wb")
        if not self._f:
            raise OSError("cannot open %s" % path)
        self.params = cData(tname, ename, block_size, jobs, checksum, 1 if headerless else 0)
        self._ctx = C.c_void_p()
        rc = L.initCompressor(C.byref(self.params), self._f, C.byref(self._ctx))
        if rc != 0:
            _libc.fclose(self._f)
            self._f = None
            raise KanziError(rc, "initCompressor")
        self.written = 0

    def __enter__(self):
        return self

    def __exit__(self, exc_type, exc, tb):
        self.close()

    def compress(self, data):
        out = C.c_size_t(0)
        view = _PyBuffer()
        if C.pythonapi.PyObject_GetBuffer(data, C.byref(view), 0) != 0:     # PyBUF_SIMPLE: contiguous bytes
            raise TypeError("compress() needs a contiguous bytes-like object")
        try:
            rc = lib().compress(self._ctx, view.buf, view.len, C.byref(out))
        finally:
            C.pythonapi.PyBuffer_Release(C.byref(view))
        if rc != 0:
            raise KanziError(rc, "compress")
        self.written += out.value
        return out.value

    def close(self):
        if self._ctx:
            out = C.c_size_t(0)
            rc = lib().disposeCompressor(C.byref(self._ctx), C.byref(out))
            self.written += out.value
            self._ctx = C.c_void_p()
            _libc.fclose(self._f)
            self._f = None
            if rc != 0:
                raise KanziError(rc, "disposeCompressor")
        return self.written


class Decompressor:
    """src/api/kanzi.py Decompressor: `Decompressor(path, buffer_size, jobs, headerless, **headerless_params)` with the
    reference's parameter names (transform, entropy, blockSize, originalSize, checksum, bsVersion; the snake_case
    spellings are accepted too), `decompress_block(max_output)`, `close()`, context manager."""

    def __init__(self, path, buffer_size=4 << 20, jobs=1, headerless=False, transform="NONE", entropy="NONE", block_size=0,
                 original_size=0, checksum=0, bs_version=6, **ref_names):
        L = lib()
        block_size = ref_names.pop("blockSize", block_size)
        original_size = ref_names.pop("originalSize", original_size)
        bs_version = ref_names.pop("bsVersion", bs_version)
        if ref_names:
            raise TypeError("unexpected arguments: %s" % ", ".join(sorted(ref_names)))
        self._f = _libc.fopen(os.fsencode(path), b"rb")
        if not self._f:
            raise OSError("cannot open %s" % path)
        self.params = dData(buffer_size, jobs, 1 if headerless else 0, _name(transform), _name(entropy), block_size,
                            original_size, checksum, bs_version)
        self._ctx = C.c_void_p()
        rc = L.initDecompressor(C.byref(self.params), self._f, C.byref(self._ctx))
        if rc != 0:
            _libc.fclose(self._f)
            self._f = None
            raise KanziError(rc, "initDecompressor")
        self.buffer_size = buffer_size

    def __enter__(self):
        return self

    def __exit__(self, exc_type, exc, tb):
        self.close()

    def decompress_block(self, max_output):
        return self.decompress(max_output)

    def decompress(self, n):
        # the library writes straight into the bytes object handed back (no zero fill, no second copy); only a
        # short last block is cut to size
        res = C.pythonapi.PyBytes_FromStringAndSize(None, max(1, n))
        ins, outs = C.c_size_t(0), C.c_size_t(n)
        rc = lib().decompress(self._ctx, C.pythonapi.PyBytes_AsString(res), C.byref(ins), C.byref(outs))
        if rc != 0:
            raise KanziError(rc, "decompress")
        return res if outs.value == len(res) else res[:outs.value]

    def close(self):
        if self._ctx:
            rc = lib().disposeDecompressor(C.byref(self._ctx))
            self._ctx = C.c_void_p()
            _libc.fclose(self._f)
            self._f = None
            if rc != 0:
                raise KanziError(rc, "disposeDecompressor")


# ---- many small buffers, many per device call (include/knz_hip.h: knz_hip_encode_streams / knz_hip_decode_streams)
def _mods():
    return (importlib.import_module("kanzi_amd.hipapi"), importlib.import_module("kanzi_amd.framing"),
            importlib.import_module("kanzi_amd.sharded"))


def _work_fits(blocks, longest, hipapi):
    """blocks x longest block of a call stay below 2 GiB (include/knz_hip.h): the device sizes its workspaces by the longest block's
    stride, which a chain makes somewhat longer than the block -- twice the block and 64 KiB hold any chain."""
    return blocks * (2 * longest + 65536) <= hipapi.BATCH_MAX_BYTES


def _fits_one_call(n, block_size, hipapi):
    blocks = (n + block_size - 1) // block_size
    return (n + 8448 * (blocks + 1) <= hipapi.BATCH_MAX_BYTES and blocks <= hipapi.STREAMS_MAX_BLOCKS and
            _work_fits(blocks, min(n, block_size), hipapi))


def _calls(sizes, block_size, hipapi):
    """Cuts the item numbers into runs that one device call takes: its item and block counts, its bytes (every item at a multiple
    of 16; the 2 GiB limit of a call leaves room for the blocks' slack, csrc/api.hip Encoder::check) and its workspaces (blocks x longest
    block). On the way back the sizes are the stored ones, which are the rooms the call is given. An item that is too large for any
    call is a ValueError: such a buffer belongs to the stream classes."""
    runs, cur, nbytes, nblocks, longest = [], [], 0, 0, 0
    for i, n in enumerate(sizes):
        blocks = (n + block_size - 1) // block_size
        if not _fits_one_call(n, block_size, hipapi):
            raise ValueError("buffer %d (%d bytes) exceeds what one device call takes; use Compressor / Decompressor" % (i, n))
        pad = (n + 15) & ~15
        if cur and (len(cur) == hipapi.STREAMS_MAX_ITEMS or nblocks + blocks > hipapi.STREAMS_MAX_BLOCKS or
                    nbytes + pad + 8448 * (nblocks + blocks + 1) > hipapi.BATCH_MAX_BYTES or
                    not _work_fits(nblocks + blocks, max(longest, min(n, block_size)), hipapi)):
            runs.append(cur)
            cur, nbytes, nblocks, longest = [], 0, 0, 0
        cur.append(i)
        nbytes += pad
        nblocks += blocks
        longest = max(longest, min(n, block_size))
    if cur:
        runs.append(cur)
    return runs


def _pack(buffers):
    blob, offs = bytearray(), []
    for b in buffers:
        blob += bytes(-len(blob) % 16)
        offs.append(len(blob))
        blob += b
    blob += bytes(64)
    return bytes(blob), offs


def _encode_two_tier(ctx, hipapi, p, d_in, in_bytes, items, prologues, room):
    """One encode_streams call over the packed input at d_in (in_bytes with its pads and slack) into room(cap), a device address with cap
    bytes behind it. For CM, TPAQ and TPAQX the bound is a first tier (include/knz_hip.h): a call that it does not hold is made again with
    the second, which holds whatever the format can write. Returns (the output's address, its bytes in use)."""
    cap = ctx.encode_streams_bound(p, items)
    try:
        d_out = room(cap)
        return d_out, ctx.encode_streams(p, d_in, items, d_out, cap, prologues=prologues)
    except hipapi.KnzError as e:
        if e.code != 12 or p.entropy_type not in hipapi.BINARY_CODERS:
            raise
    cap += 32 * in_bytes
    d_out = room(cap)
    return d_out, ctx.encode_streams(p, d_in, items, d_out, cap, prologues=prologues)


def compress_many(buffers, transform, entropy, block_size, checksum=0, jobs=1, device=0):
    """Every buffer as a stream of its own: the file the reference CLI writes for those bytes (the header stores the buffer's length
    as the original size), many buffers per device call. Returns the streams in the buffers' order."""
    hipapi, framing, sharded = _mods()
    buffers = [bytes(b) for b in buffers]
    ctx = hipapi.Context(device)
    try:
        p = ctx.params(transform, entropy, block_size, checksum, jobs)
        bufs = sharded._DeviceBuffers(ctx)
        out = [None] * len(buffers)
        for run in _calls([len(b) for b in buffers], block_size, hipapi):
            blob, offs = _pack([buffers[i] for i in run])
            items = (hipapi.Item * len(run))()
            pro = bytearray()
            for k, i in enumerate(run):
                h, hb = framing.make_header(p.entropy_type, p.transform_type, block_size, checksum, len(buffers[i]))
                items[k].in_off, items[k].in_len, items[k].prologue_off, items[k].prologue_bits = offs[k], len(buffers[i]), len(pro), hb
                pro += h
            d_in = bufs.get("in", len(blob))
            ctx.h2d(d_in, blob)
            d_out, used = _encode_two_tier(ctx, hipapi, p, d_in, len(blob), items, bytes(pro), lambda cap: bufs.get("out", cap))
            raw = ctx.d2h(d_out, used)
            for k, i in enumerate(run):
                out[i] = raw[items[k].out_off:items[k].out_off + (items[k].out_len + 7) // 8]
        return out
    finally:
        ctx.close()


def decompress_many(streams, jobs=1, device=0):
    """The way back: the headers are parsed here, streams of equal parameters share device calls, each stream's room is its stored
    original size. A stream without a stored size is decoded by itself (sharded.decompress_sharded). Raises KanziError with the code
    of the first stream that fails."""
    hipapi, framing, sharded = _mods()
    streams = [bytes(s) for s in streams]
    out = [None] * len(streams)
    groups = {}
    ctx = hipapi.Context(device)
    try:
        for i, s in enumerate(streams):
            try:
                h = framing.parse_header(s)
            except framing.HeaderError as e:
                raise KanziError(e.code, "stream %d: %s" % (i, e))
            if h["orig_size"] == 0 or not _fits_one_call(h["orig_size"], h["block_size"], hipapi) or not _fits_one_call(len(s), 1024, hipapi):
                # no stored size (it may still hold data), or more than one call decodes
                out[i] = sharded.decompress_sharded(s, 0, 1, sharded.DeviceRunDecoder(device, jobs), lambda part: [part])
                continue
            key = (h["etype"], h["ttype"], h["block_size"], h["checksum_bits"], h["bs_version"])
            groups.setdefault(key, []).append((i, h))
        bufs = sharded._DeviceBuffers(ctx)
        for (etype, ttype, bs, ck, ver), members in groups.items():
            p = ctx.params(ttype, etype, bs, ck, jobs, ver or 1)       # a parsed version 0 is an old layout (the C ABI keeps 0 for "unset = current")
            for run in _calls([h["orig_size"] for _, h in members], bs, hipapi):
                blob, offs = _pack([streams[members[k][0]] for k in run])
                items = (hipapi.Item * len(run))()
                at = 0
                for n, k in enumerate(run):
                    i, h = members[k]
                    items[n].in_off, items[n].in_len, items[n].start_bit = offs[n], 8 * len(streams[i]), h["bits"]
                    items[n].out_off, items[n].out_cap = at, h["orig_size"]
                    at += (h["orig_size"] + 15) & ~15
                d_in, d_out = bufs.get("in", len(blob)), bufs.get("out", at + 64)
                ctx.h2d(d_in, blob)
                ctx.decode_streams(p, d_in, items, d_out, at + 64)
                raw = ctx.d2h(d_out, at)
                for n, k in enumerate(run):
                    i, h = members[k]
                    if items[n].error:
                        raise KanziError(items[n].error, "stream %d: decoding" % i)
                    if items[n].out_len != h["orig_size"]:      # (the stream ends before the size its header promises)
                        raise KanziError(13, "stream %d: %d bytes where the header stores %d" % (i, items[n].out_len, h["orig_size"]))
                    out[i] = raw[items[n].out_off:items[n].out_off + items[n].out_len]
        return out
    finally:
        ctx.close()


# ---- byte planes: byte k of every element next to byte k of the others, so that an order-0 coder sees the compressible bytes of
# floating-point data (sign and exponent) apart from the incompressible ones (mantissa). No transform of the format: the stream codes the
# split bytes and does not store the width, which the caller keeps with the dtype and shape.
PLANE_WIDTHS = (1, 2, 4, 8)


def _as_elements(data, width):
    import numpy as np
    if width not in PLANE_WIDTHS:
        raise ValueError("width %r: elements of 1, 2, 4 and 8 bytes are taken" % (width,))
    a = np.frombuffer(data, dtype=np.uint8)
    if a.size % width:
        raise ValueError("%d bytes are no multiple of the width %d" % (a.size, width))
    return a


def split_bytes(data, width):
    """data as len(data) / width elements of width bytes: plane 0 (byte 0 of every element), then plane 1, ... as bytes. What
    TensorCodec.compress(planes=...) codes, done on the host with numpy: for compress_many, and the specification of the device kernel."""
    return _as_elements(data, width).reshape(-1, width).T.tobytes()


def join_bytes(data, width):
    """The way back of split_bytes: what turns the output of the reference tool for a stream of planes into the tensor's bytes."""
    return _as_elements(data, width).reshape(width, -1).T.tobytes()


# ---- the same for tensors that are on the device already: nothing payload-sized crosses the bus
HEADER_PEEK = 32               # bytes of every stream that decompress reads on the host: the longest header framing.make_header writes
                                # is 208 bits (32 + 4 + 2 + 5 + 48 + 28 + 2 + 48 + 15 + 24), and an empty stream's end marker follows a
                                # header without size (160 bits) inside them


def _plane_widths(tensors, planes):
    """The `planes` argument of TensorCodec.compress as one width per tensor (None: no planes), with its ValueErrors, by index."""
    if planes is None or planes is False:
        return None
    if planes is True:
        widths = [t.element_size() // 2 if t.is_complex() else t.element_size() for t in tensors]
        for i, w in enumerate(widths):
            if w > 8:
                raise ValueError("tensor %d: %s has numbers of %d bytes, planes of at most 8 are taken" % (i, tensors[i].dtype, w))
        return widths
    widths = list(planes)
    if len(widths) != len(tensors):
        raise ValueError("planes holds %d widths for %d tensors" % (len(widths), len(tensors)))
    for i, (t, w) in enumerate(zip(tensors, widths)):
        if isinstance(w, bool) or w not in PLANE_WIDTHS:
            raise ValueError("tensor %d: width %r, planes of 1, 2, 4 and 8 bytes are taken" % (i, w))
        if t.numel() * t.element_size() % w:
            raise ValueError("tensor %d: %d bytes are no multiple of the width %d" % (i, t.numel() * t.element_size(), w))
    return [int(w) for w in widths]


def _check_tensors(tensors, device, planes=False):
    """The ValueErrors of TensorCodec.compress, by index, before any device work: what is no tensor first, then what is not contiguous,
    then what `planes` cannot mean for these tensors, then what is in the wrong place. device None leaves out the comparison of devices.
    Returns the plane widths (_plane_widths)."""
    import torch
    for i, t in enumerate(tensors):
        if not isinstance(t, torch.Tensor):
            raise ValueError("tensor %d is no torch.Tensor but %s" % (i, type(t).__name__))
    for i, t in enumerate(tensors):
        if not t.is_contiguous():
            raise ValueError("tensor %d is not contiguous (its bytes in memory order are asked for; call .contiguous() first)" % i)
    widths = _plane_widths(tensors, planes)
    for i, t in enumerate(tensors):
        if t.device.type != "cuda":
            raise ValueError("tensor %d is on %s, not on the GPU (compress_many takes host bytes)" % (i, t.device))
        if device is not None and t.device != device:
            raise ValueError("tensor %d is on %s, the codec on %s" % (i, t.device, device))
    return widths


def _only_end_marker(head, bits, length):
    """A stream without a stored size has no bytes when the end marker (eight zero bits) is all that follows its header: what compress
    writes for an empty tensor. Told from the stream's first bytes when the header ends at a byte boundary (it does since version 6)."""
    return bits % 8 == 0 and length == bits // 8 + 1 and head[bits // 8:bits // 8 + 1] == b"\0"


class TensorCodec:
    """compress_many / decompress_many for tensors that are on the GPU, with one device context, its workspaces and torch's caching
    allocator kept across calls. Every stream is byte for byte what compress_many returns for the tensor's bytes, so the file the reference
    CLI writes for them; the payload stays on the device in both directions (scattered tensors are gathered, and the streams compacted,
    by knz_hip_copy_many), and only the stream headers (HEADER_PEEK bytes each) and the per-item results are read on the host. With
    `planes` the tensors are coded as the byte planes of their elements (split_bytes above), split and joined by the gathering kernels.

    All work is ordered on `stream` (a torch.cuda.Stream; default: the stream current on `device` when the codec is made), and every buffer
    is allocated from torch's allocator while the stream that the kernels run on is current. The calls wait for that stream where the C
    ABI does (the read-back of the items, the header table); they synchronise nothing else. Tensors produced on the same stream need no
    synchronisation by the caller; tensors produced on another stream are the caller's to order (stream.wait_stream / events), and
    results used on another stream likewise: torch's own rule.

    A torch build that ships its own HIP runtime has to be imported before the device library is first loaded (hipapi.lib(), any
    hipapi.Context), as bench.py does: the library then shares torch's runtime. The other way round torch finds no GPU."""

    def __init__(self, device=None, stream=None):
        import torch
        hipapi, self._framing, self._sharded = _mods()
        self._hipapi = hipapi
        dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device("cuda", device) if isinstance(device, int) else torch.device(device)
        if dev.type != "cuda":
            raise ValueError("TensorCodec needs a GPU device, not %s" % dev)
        if dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        self.device = dev
        self.stream = torch.cuda.current_stream(dev) if stream is None else stream
        # torch's default stream has the handle 0, which knz_hip_create takes as "a stream of the context's own": the codec then works on a
        # torch stream of its own that every call puts behind what `stream` holds and that `stream` is put behind again afterwards, both on
        # the device (events, no host synchronisation), so that the caller sees the order of one stream
        self._work = self.stream if self.stream.cuda_stream else torch.cuda.Stream(dev)
        self.ctx = hipapi.Context(dev.index, stream=self._work.cuda_stream)

    def __enter__(self):
        return self

    def __exit__(self, exc_type, exc, tb):
        self.close()

    def close(self):
        if self.ctx is not None:
            self.ctx.close()
            self.ctx = None

    def _open(self):
        if self.ctx is None:
            raise RuntimeError("TensorCodec is closed")

    @contextlib.contextmanager
    def _enqueue(self):
        """The codec's device and working stream current; the working stream behind the caller's stream before, in front of it after."""
        import torch
        with torch.cuda.device(self.device), torch.cuda.stream(self._work):
            if self._work is not self.stream:
                self._work.wait_stream(self.stream)
            try:
                yield
            finally:
                if self._work is not self.stream:
                    self.stream.wait_stream(self._work)

    def _hand_over(self, t):
        """A result allocated on the working stream is the caller's from here on: torch's allocator is told the stream that uses it."""
        if self._work is not self.stream and t.numel():
            t.record_stream(self.stream)
        return t

    def _empty(self, n):
        import torch
        return torch.empty(n, dtype=torch.uint8, device=self.device)

    def _copy(self, copies):
        most = self._hipapi.COPY_MAX_COPIES
        for k in range(0, len(copies), most):
            self.ctx.copy_many(copies[k:k + most])

    def _planes(self, entries, split):
        most = self._hipapi.COPY_MAX_COPIES
        for k in range(0, len(entries), most):
            (self.ctx.split_many if split else self.ctx.join_many)(entries[k:k + most])

    def _gather(self, parts, widths=None):
        """parts: (device address, bytes) each. One copy_many moves them into a new buffer, every part at a multiple of 16, the pads
        between them and 64 bytes behind the last zero, as _pack leaves them. With widths (one per part) it is one split_many, which
        leaves part k as its byte planes and copies the zeros as elements of one byte. Returns (the buffer, the parts' offsets)."""
        import torch
        offs, at = [], 0
        for _, n in parts:
            offs.append(at)
            at += (n + 15) & ~15
        buf = self._empty(at + 64)
        zeros = torch.zeros(64, dtype=torch.uint8, device=self.device)
        base, z = buf.data_ptr(), zeros.data_ptr()
        copies = [(a, base + o, n) for (a, n), o in zip(parts, offs)]
        copies += [(z, base + o + n, -n % 16) for (_, n), o in zip(parts, offs) if n % 16]
        copies.append((z, base + at, 64))
        if widths is None:
            self._copy(copies)
        else:
            self._planes([c + (w,) for c, w in zip(copies, list(widths) + [1] * (len(copies) - len(parts)))], True)
        return buf, offs

    def compress(self, tensors, transform, entropy, block_size, checksum=0, jobs=1, planes=False):
        """tensors: torch tensors of any dtype on the codec's device, contiguous; tensor i stands for its numel() * element_size() bytes in
        memory order. Returns (blob, offsets): blob a 1-D uint8 tensor on the device, offsets a list of len(tensors) + 1 ints, stream k =
        blob[offsets[k]:offsets[k + 1]]. ValueError, with the index, for a tensor that is not contiguous, on the CPU or on another
        device (nothing is moved or made contiguous behind the caller's back), and for one too large for a device call.

        planes: True codes every tensor as the byte planes of its elements (split_bytes of its bytes; the width is element_size(), half of
        it for a complex dtype), which is what makes an order-0 coder worth its while on floating-point data; a sequence gives one width
        of 1, 2, 4 or 8 per tensor, for uint8 tensors that hold the bytes of another type. Stream k is then compress_many's for
        split_bytes(bytes of tensor k, width k), and the kernel that gathers the call's input does the split, so the payload is still
        moved once. The width is NOT stored in the stream: decompress has to be given it again. ValueError, with the index, for a width
        that is not taken or does not divide the tensor's bytes."""
        import torch
        self._open()
        tensors = list(tensors)
        widths = _check_tensors(tensors, self.device, planes)
        hipapi, framing, ctx = self._hipapi, self._framing, self.ctx
        sizes = [t.numel() * t.element_size() for t in tensors]
        runs = _calls(sizes, block_size, hipapi)
        with self._enqueue():
            p = ctx.params(transform, entropy, block_size, checksum, jobs)
            where, keep = [None] * len(tensors), []                  # (address, bytes) of every stream in its call's output, which `keep` holds
            for run in runs:
                packed, offs = self._gather([(tensors[i].data_ptr(), sizes[i]) for i in run], None if widths is None else [widths[i] for i in run])
                items = (hipapi.Item * len(run))()
                pro = bytearray()
                for k, i in enumerate(run):
                    h, hb = framing.make_header(p.entropy_type, p.transform_type, block_size, checksum, sizes[i])
                    items[k].in_off, items[k].in_len, items[k].prologue_off, items[k].prologue_bits = offs[k], sizes[i], len(pro), hb
                    pro += h

                def room(cap):
                    keep.append(self._empty(cap))
                    return keep[-1].data_ptr()
                d_out, _ = _encode_two_tier(ctx, hipapi, p, packed.data_ptr(), packed.numel(), items, bytes(pro), room)
                for k, i in enumerate(run):
                    where[i] = (d_out + items[k].out_off, (items[k].out_len + 7) // 8)
            offsets = [0]
            for _, n in where:
                offsets.append(offsets[-1] + n)
            blob = self._empty(offsets[-1])
            self._copy([(a, blob.data_ptr() + o, n) for (a, n), o in zip(where, offsets)])
        return self._hand_over(blob), offsets

    def decompress(self, blob, offsets, planes=None):
        """The way back: blob a 1-D uint8 tensor on the codec's device, stream k = blob[offsets[k]:offsets[k + 1]], written by this class,
        by compress_many or by the reference. Returns a list of uint8 tensors on the device, each starting at a multiple of 16 bytes (so
        .view(dtype) gives any dtype back); the tensors of one device call are views of one allocation. The first HEADER_PEEK bytes of
        every stream are read on the host, the headers parsed there, streams of equal parameters share device calls. Raises KanziError
        with the stream's index as decompress_many does. A stream without a stored size that holds data, or one that needs more than one
        device call, goes decompress_many's way through the host and is uploaded again; streams that compress wrote never do.

        planes: one width of 1, 2, 4 or 8 per stream, the widths that compress(planes=...) split the tensors with (the streams do not
        store them). Every device call then decodes into a buffer of its own, and one join_many writes the results from there (join_bytes
        of what the stream decodes to). ValueError, with the stream's index, for a width that is not taken or does not divide the
        decoded length."""
        import torch
        self._open()
        hipapi, framing, sharded, ctx = self._hipapi, self._framing, self._sharded, self.ctx
        offsets = [int(o) for o in offsets]
        n = len(offsets) - 1
        if not isinstance(blob, torch.Tensor) or blob.device != self.device or blob.dtype != torch.uint8 or blob.dim() != 1 or not blob.is_contiguous():
            raise ValueError("blob must be a contiguous 1-D uint8 tensor on %s" % self.device)
        if n < 0 or offsets[0] < 0 or offsets[-1] > blob.numel() or any(a > b for a, b in zip(offsets, offsets[1:])):
            raise ValueError("offsets must rise from 0 to at most the blob's length")
        widths = None if planes is None else list(planes)
        if widths is not None:
            if len(widths) != n:
                raise ValueError("planes holds %d widths for %d streams" % (len(widths), n))
            for i, w in enumerate(widths):
                if isinstance(w, bool) or w not in PLANE_WIDTHS:
                    raise ValueError("stream %d: width %r, planes of 1, 2, 4 and 8 bytes are taken" % (i, w))

        def whole_elements(i, decoded):
            if widths is not None and decoded % widths[i]:
                raise ValueError("stream %d: %d decoded bytes are no multiple of the width %d" % (i, decoded, widths[i]))
        if n == 0:
            return []
        out = [None] * n
        lens = [offsets[k + 1] - offsets[k] for k in range(n)]
        base = blob.data_ptr()
        with self._enqueue():
            table = self._empty(HEADER_PEEK * n)
            self._copy([(base + offsets[k], table.data_ptr() + HEADER_PEEK * k, min(HEADER_PEEK, lens[k])) for k in range(n)])
            heads = ctx.d2h(table.data_ptr(), HEADER_PEEK * n)
            groups = {}
            for i in range(n):
                head = heads[HEADER_PEEK * i:HEADER_PEEK * i + min(HEADER_PEEK, lens[i])]
                try:
                    h = framing.parse_header(head)
                except framing.HeaderError as e:
                    raise KanziError(e.code, "stream %d: %s" % (i, e))
                if h["orig_size"] == 0 and _only_end_marker(head, h["bits"], lens[i]):
                    out[i] = self._empty(0)
                    continue
                if h["orig_size"] == 0 or not _fits_one_call(h["orig_size"], h["block_size"], hipapi) or not _fits_one_call(lens[i], 1024, hipapi):
                    s = bytes(blob[offsets[i]:offsets[i + 1]].cpu().numpy())
                    back = sharded.decompress_sharded(s, 0, 1, sharded.DeviceRunDecoder(self.device.index, 1), lambda part: [part])
                    whole_elements(i, len(back))
                    if widths is not None:
                        back = join_bytes(back, widths[i])
                    out[i] = self._hand_over(torch.frombuffer(bytearray(back), dtype=torch.uint8).to(self.device)) if back else self._empty(0)
                    continue
                whole_elements(i, h["orig_size"])
                key = (h["etype"], h["ttype"], h["block_size"], h["checksum_bits"], h["bs_version"])
                groups.setdefault(key, []).append((i, h))
            for (etype, ttype, bs, ck, ver), members in groups.items():
                p = ctx.params(ttype, etype, bs, ck, 1, ver or 1)
                for run in _calls([h["orig_size"] for _, h in members], bs, hipapi):
                    packed, offs = self._gather([(base + offsets[members[k][0]], lens[members[k][0]]) for k in run])
                    items = (hipapi.Item * len(run))()
                    at = 0
                    for m, k in enumerate(run):
                        i, h = members[k]
                        items[m].in_off, items[m].in_len, items[m].start_bit = offs[m], 8 * lens[i], h["bits"]
                        items[m].out_off, items[m].out_cap = at, h["orig_size"]
                        at += (h["orig_size"] + 15) & ~15
                    d_out = self._hand_over(self._empty(at + 64))
                    d_dec = d_out if widths is None else self._empty(at + 64)       # planes: decoded here, joined into d_out
                    ctx.decode_streams(p, packed.data_ptr(), items, d_dec.data_ptr(), at + 64)
                    for m, k in enumerate(run):
                        i, h = members[k]
                        if items[m].error:
                            raise KanziError(items[m].error, "stream %d: decoding" % i)
                        if items[m].out_len != h["orig_size"]:
                            raise KanziError(13, "stream %d: %d bytes where the header stores %d" % (i, items[m].out_len, h["orig_size"]))
                        out[i] = d_out[items[m].out_off:items[m].out_off + items[m].out_len]
                    if widths is not None:
                        self._planes([(d_dec.data_ptr() + items[m].out_off, d_out.data_ptr() + items[m].out_off, items[m].out_len, widths[members[k][0]])
                                      for m, k in enumerate(run)], False)
        return out


def compress_tensors(tensors, transform, entropy, block_size, checksum=0, jobs=1, planes=False):
    """TensorCodec.compress on torch's current device and stream, with a codec made for this one call."""
    tensors = list(tensors)
    planes = planes if planes is None or isinstance(planes, bool) else list(planes)
    _check_tensors(tensors, None, planes)
    with TensorCodec() as codec:
        return codec.compress(tensors, transform, entropy, block_size, checksum, jobs, planes)


def decompress_tensors(blob, offsets, planes=None):
    """TensorCodec.decompress on the blob's device and torch's current stream there, with a codec made for this one call."""
    with TensorCodec(blob.device) as codec:
        return codec.decompress(blob, offsets, planes)
