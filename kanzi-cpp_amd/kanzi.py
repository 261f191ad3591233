"""Compressor / Decompressor classes over the C API of libkanzi_amd.so.

Mirrors the reference's ctypes shim (src/api/kanzi_c_api.py:88-137 for the bindings,
src/api/kanzi.py for the two classes): same struct layouts, same call sequence
(init -> compress()/decompress() per block -> dispose). Only marshals data.

compress_many / decompress_many (at the end) are the batch form for many small independent buffers: they go over the device
C ABI directly (hipapi.Context.encode_streams / decode_streams) and framing.py, many buffers per device call.
"""
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
    of 16; the 2 GiB limit of a call leaves room for the blocks' slack, csrc/api.hip encode_impl) and its workspaces (blocks x longest
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
            cap = ctx.encode_streams_bound(p, items)
            d_in = bufs.get("in", len(blob))
            ctx.h2d(d_in, blob)
            try:
                used = ctx.encode_streams(p, d_in, items, bufs.get("out", cap), cap, prologues=bytes(pro))
            except hipapi.KnzError as e:
                # CM, TPAQ, TPAQX: the bound is a first tier (include/knz_hip.h); the second holds whatever the format can write
                if e.code != 12 or p.entropy_type not in hipapi.BINARY_CODERS:
                    raise
                cap += 32 * len(blob)
                used = ctx.encode_streams(p, d_in, items, bufs.get("out", cap), cap, prologues=bytes(pro))
            raw = ctx.d2h(bufs.get("out", cap), used)
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
