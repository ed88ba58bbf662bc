"""Python binding of liblz4mi.so (include/lz4mi.h) — the MI355X LZ4 block codec.

Used by bench.py, __graft_entry__ and the tests. Every compute entry point goes
through the HIP C-ABI; there is no CPU fallback: if the library or a gfx950
device is missing, calls raise Lz4miError.

Mirrors the reference's raw-block and frame functions
(src/block/blockCompress.js:31, src/block/blockDecompress.js:30,
src/xxhash32/xxhash32.js:21) with the same argument meaning and error strings.
"""
import ctypes
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
PKG_DIR = os.path.dirname(_HERE)
LIB_PATH = os.path.join(PKG_DIR, "liblz4mi.so")

OK = 0
ERR_OUTPUT_TOO_SMALL, ERR_MALFORMED, ERR_OFFSET0, ERR_DICT_OOB = -1, -2, -3, -4
ERR_MAGIC, ERR_VERSION, ERR_CHECKSUM, ERR_RANGE, ERR_CROSS_BLOCK = -5, -6, -7, -8, -9
ERR_BLOCK_CHECKSUM = -10
ERR_HIP, ERR_ARG, ERR_NO_DEVICE, ERR_DEVICE_BOUND = -100, -101, -102, -103

DEVICE_PTRS = 0x1
JS_COMPAT = 0x2
JS_EXACT = 0x8
XXH_STANDARD = 0x4
XXH_LEN64 = 0x10
BLOCK_CHECKSUM = 0x20
FRAME_WORDS = 0x40
LINKED = 0x80
LINKED_EXACT = 0x100
VERIFY_BLOCKS = 0x200
VERIFY_CONTENT = 0x400
FRAMES_MEASURE = 0x800
FRAMES_CONTENT_CHECKSUM = 0x1000
FRAMES_NO_CONTENT_SIZE = 0x2000
FRAMES_DEPENDENT = 0x4000
FRAMES_PACKED = 0x8000
FRAMES_CHAINS = 0x10000

# finfo[f][7] of the frame batch calls, decode and encode (include/lz4mi.h LZ4MI_FRAMES_DECLINE_*)
(DECLINE_CAP_BLOCKS, DECLINE_PAST_END, DECLINE_EMPTY, DECLINE_UNSIZED_EXACT, DECLINE_MEASURE, DECLINE_SIZE_MISMATCH,
 DECLINE_OUT_CAP, DECLINE_LAYOUT, DECLINE_DEPENDENT, DECLINE_HASH_4G) = range(1, 11)

GEN_RANDOM, GEN_REPETITIVE, GEN_TILES216 = 0, 1, 2
GENERATORS = {"random": GEN_RANDOM, "repetitive": GEN_REPETITIVE, "tiles216": GEN_TILES216}
# decode batches of at most this many blocks take the small-batch path (the library's default,
# csrc/lz4mi_capi.cpp small_blocks(); LZ4MI_SMALL_BLOCKS changes it, read once per process)
SMALL_BLOCKS = int(os.environ.get("LZ4MI_SMALL_BLOCKS", "192"))

# every symbol include/lz4mi.h declares (checked by tests/test_capi_cpu.py)
EXPORTS = ("lz4mi_status_message", "lz4mi_init", "lz4mi_device_count", "lz4mi_version",
           "lz4mi_decompress_blocks", "lz4mi_compress_blocks", "lz4mi_compress_block_table",
           "lz4mi_xxh32", "lz4mi_xxh32_blocks", "lz4mi_frame_pack", "lz4mi_generate_blocks",
           "lz4mi_build_id", "lz4mi_xxh32_reset", "lz4mi_xxh32_update", "lz4mi_xxh32_digest",
           "lz4mi_frame_decompress", "lz4mi_frame_index", "lz4mi_compress_chain",
           "lz4mi_host_compress_block", "lz4mi_host_compress_chain", "lz4mi_host_decompress_block",
           "lz4mi_decoded_sizes", "lz4mi_host_decoded_size", "lz4mi_host_block_read_end",
           "lz4mi_verify_blocks", "lz4mi_host_verify_blocks", "lz4mi_frames_index", "lz4mi_frames_decompress",
           "lz4mi_host_frames_index", "lz4mi_host_frame_index", "lz4mi_frame_bound", "lz4mi_frames_plan",
           "lz4mi_frames_compress", "lz4mi_host_frames_plan", "lz4mi_host_frames_compress",
           "lz4mi_frames_verify_blocks", "lz4mi_host_frames_verify_blocks")


class Lz4miError(RuntimeError):
    def __init__(self, status, message=None):
        self.status = status
        super().__init__(message or status_message(status))


_lib = None
_vp = ctypes.c_void_p


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise Lz4miError(ERR_NO_DEVICE, "liblz4mi.so not built (run __graft_entry__.build())")
        # PyTorch wheels bundle their own libamdhip64 under a different file name;
        # load torch first so one HIP runtime serves both (a second runtime
        # instance in the process cannot see the GPU).
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        L = ctypes.CDLL(LIB_PATH)
        L.lz4mi_status_message.restype = ctypes.c_char_p
        L.lz4mi_status_message.argtypes = [ctypes.c_int32]
        L.lz4mi_version.restype = ctypes.c_char_p
        L.lz4mi_build_id.restype = ctypes.c_char_p
        L.lz4mi_xxh32_reset.restype = None
        L.lz4mi_xxh32_reset.argtypes = [_vp, ctypes.c_uint32, ctypes.c_uint32]
        L.lz4mi_xxh32_update.restype = None
        L.lz4mi_xxh32_update.argtypes = [_vp, _vp, ctypes.c_size_t]
        L.lz4mi_xxh32_digest.restype = ctypes.c_uint32
        L.lz4mi_xxh32_digest.argtypes = [_vp]
        L.lz4mi_init.restype = ctypes.c_int32
        L.lz4mi_init.argtypes = [ctypes.c_int32]
        L.lz4mi_device_count.restype = ctypes.c_int32
        L.lz4mi_decompress_blocks.restype = ctypes.c_int32
        L.lz4mi_decompress_blocks.argtypes = [_vp, _vp, _vp, _vp, _vp, _vp, _vp, ctypes.c_uint32, _vp, _vp,
                                              ctypes.c_uint32, ctypes.c_uint32, _vp]
        L.lz4mi_compress_blocks.restype = ctypes.c_int32
        L.lz4mi_compress_blocks.argtypes = [_vp, _vp, _vp, _vp, _vp, _vp, ctypes.c_uint32, ctypes.c_uint32, _vp]
        L.lz4mi_compress_block_table.restype = ctypes.c_int64
        L.lz4mi_compress_block_table.argtypes = [_vp, ctypes.c_uint64, ctypes.c_int32, ctypes.c_int32, _vp, _vp,
                                                 ctypes.c_uint64, ctypes.c_int32, ctypes.c_uint32, _vp]
        L.lz4mi_xxh32.restype = ctypes.c_uint32
        L.lz4mi_xxh32.argtypes = [_vp, ctypes.c_size_t, ctypes.c_uint32, ctypes.c_uint32]
        L.lz4mi_xxh32_blocks.restype = ctypes.c_int32
        L.lz4mi_xxh32_blocks.argtypes = [_vp, _vp, _vp, ctypes.c_uint32, _vp, ctypes.c_uint32, ctypes.c_uint32, _vp]
        L.lz4mi_frame_pack.restype = ctypes.c_int32
        L.lz4mi_frame_pack.argtypes = [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, ctypes.c_uint32, ctypes.c_uint32, _vp]
        L.lz4mi_frame_decompress.restype = ctypes.c_int32
        L.lz4mi_frame_decompress.argtypes = [_vp, ctypes.c_uint64, _vp, ctypes.c_uint64, _vp, ctypes.c_uint32, _vp]
        L.lz4mi_compress_chain.restype = ctypes.c_int32
        L.lz4mi_compress_chain.argtypes = [_vp, ctypes.c_uint64, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, _vp,
                                           _vp, _vp, _vp, ctypes.c_uint32, _vp]
        L.lz4mi_host_compress_block.restype = ctypes.c_int64
        L.lz4mi_host_compress_block.argtypes = [_vp, ctypes.c_uint64, ctypes.c_int32, ctypes.c_int32, _vp, _vp,
                                                ctypes.c_uint64, ctypes.c_int32]
        L.lz4mi_host_compress_chain.restype = ctypes.c_int32
        L.lz4mi_host_compress_chain.argtypes = [_vp, ctypes.c_uint64, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32,
                                                _vp, _vp, _vp, _vp]
        L.lz4mi_host_decompress_block.restype = ctypes.c_int64
        L.lz4mi_host_decompress_block.argtypes = [_vp, ctypes.c_uint64, ctypes.c_int64, ctypes.c_int64, _vp,
                                                  ctypes.c_uint64, ctypes.c_int64, _vp, ctypes.c_uint32, ctypes.c_uint32]
        L.lz4mi_decoded_sizes.restype = ctypes.c_int32
        L.lz4mi_decoded_sizes.argtypes = [_vp, _vp, _vp, _vp, _vp, ctypes.c_uint32, ctypes.c_uint32, _vp]
        L.lz4mi_host_decoded_size.restype = ctypes.c_int64
        L.lz4mi_host_decoded_size.argtypes = [_vp, ctypes.c_uint64, ctypes.c_int64, ctypes.c_int64, _vp]
        L.lz4mi_host_block_read_end.restype = ctypes.c_int64
        L.lz4mi_host_block_read_end.argtypes = [_vp, ctypes.c_uint64, ctypes.c_int64, ctypes.c_int64]
        L.lz4mi_verify_blocks.restype = ctypes.c_int32
        L.lz4mi_verify_blocks.argtypes = [_vp, ctypes.c_uint64, _vp, _vp, _vp, ctypes.c_uint32, ctypes.c_uint32, _vp]
        L.lz4mi_host_verify_blocks.restype = ctypes.c_int32
        L.lz4mi_host_verify_blocks.argtypes = [_vp, ctypes.c_uint64, _vp, _vp, _vp, ctypes.c_uint32, ctypes.c_uint32]
        L.lz4mi_frame_index.restype = ctypes.c_int32
        L.lz4mi_frame_index.argtypes = [_vp, ctypes.c_uint64, _vp, _vp, ctypes.c_uint32, _vp, ctypes.c_uint32, _vp]
        L.lz4mi_frames_index.restype = ctypes.c_int32
        L.lz4mi_frames_index.argtypes = [_vp, _vp, _vp, ctypes.c_uint32, _vp, _vp, _vp, _vp, ctypes.c_uint32, _vp, _vp,
                                         ctypes.c_uint32, _vp]
        L.lz4mi_frames_decompress.restype = ctypes.c_int32
        L.lz4mi_frames_decompress.argtypes = [_vp, _vp, _vp, _vp, _vp, ctypes.c_uint32, _vp, ctypes.c_uint32, _vp, _vp,
                                              _vp, ctypes.c_uint32, _vp]
        fverify = [_vp, _vp, _vp, ctypes.c_uint32, _vp, _vp, _vp, ctypes.c_uint32, _vp, _vp, ctypes.c_uint32]
        L.lz4mi_frames_verify_blocks.restype = ctypes.c_int32
        L.lz4mi_frames_verify_blocks.argtypes = fverify + [_vp]
        L.lz4mi_host_frames_verify_blocks.restype = ctypes.c_int32
        L.lz4mi_host_frames_verify_blocks.argtypes = fverify
        L.lz4mi_host_frames_index.restype = ctypes.c_int32
        L.lz4mi_host_frames_index.argtypes = [_vp, _vp, _vp, ctypes.c_uint32, _vp, _vp, _vp, _vp, ctypes.c_uint32, _vp,
                                              _vp, ctypes.c_uint32]
        L.lz4mi_host_frame_index.restype = ctypes.c_int32
        L.lz4mi_host_frame_index.argtypes = [_vp, ctypes.c_uint64, _vp, _vp, ctypes.c_uint32, _vp]
        L.lz4mi_frame_bound.restype = ctypes.c_uint64
        L.lz4mi_frame_bound.argtypes = [ctypes.c_uint64, ctypes.c_uint32]
        plan = [_vp, _vp, ctypes.c_uint32, ctypes.c_uint32, _vp, _vp, _vp, _vp, ctypes.c_uint32, _vp, _vp, ctypes.c_uint32]
        comp = [_vp, _vp, _vp, _vp, _vp, ctypes.c_uint32, _vp, ctypes.c_uint32, _vp, ctypes.c_uint64, _vp, ctypes.c_uint64,
                _vp, _vp, ctypes.c_uint32]
        L.lz4mi_frames_plan.restype = ctypes.c_int32
        L.lz4mi_frames_plan.argtypes = plan + [_vp]
        L.lz4mi_host_frames_plan.restype = ctypes.c_int32
        L.lz4mi_host_frames_plan.argtypes = plan
        L.lz4mi_frames_compress.restype = ctypes.c_int32
        L.lz4mi_frames_compress.argtypes = comp + [_vp]
        L.lz4mi_host_frames_compress.restype = ctypes.c_int32
        L.lz4mi_host_frames_compress.argtypes = comp
        L.lz4mi_generate_blocks.restype = ctypes.c_int32
        L.lz4mi_generate_blocks.argtypes = [_vp, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32,
                                            ctypes.c_uint32, _vp]
        _lib = L
    return _lib


def status_message(status):
    return lib().lz4mi_status_message(int(status)).decode()


def _check(st):
    if st != OK:
        raise Lz4miError(st)


def init(device=-1):
    _check(lib().lz4mi_init(device))


def device_count():
    return lib().lz4mi_device_count()


def build_id():
    """Hash of the sources liblz4mi.so was compiled from (see Makefile SRC_HASH)."""
    return lib().lz4mi_build_id().decode()


def _p(a):
    return a.ctypes.data if a is not None and a.size else None


def _u8(x):
    if x is None:
        return None
    if isinstance(x, (bytes, bytearray, memoryview)):
        return np.frombuffer(bytes(x), dtype=np.uint8)
    return np.ascontiguousarray(x, dtype=np.uint8)


def compress_bound(n):
    return n + n // 255 + 16


# ---------------------------------------------------------------- host API
def xxh32(data, seed=0, standard=False):
    """xxHash32 (reference variant by default; host CPU, one serial chain)."""
    a = _u8(data)
    return lib().lz4mi_xxh32(_p(a), a.size, seed & 0xFFFFFFFF, XXH_STANDARD if standard else 0)


class XXHash32:
    """Streaming XXH32 (class XXHash32, src/xxhash32/xxhash32Stateful.js:13-152) over the
    library's host implementation: update(chunk) any number of times, digest() any time.
    len64=True keeps the 64-bit length (the reference wraps it at 2 GiB, :37)."""

    def __init__(self, seed=0, standard=False, len64=False):
        self._st = np.zeros(7, dtype=np.uint64)       # lz4mi_xxh32_state
        lib().lz4mi_xxh32_reset(self._st.ctypes.data, seed & 0xFFFFFFFF,
                                (XXH_STANDARD if standard else 0) | (XXH_LEN64 if len64 else 0))

    def update(self, data):
        a = _u8(data)
        lib().lz4mi_xxh32_update(self._st.ctypes.data, _p(a), a.size)
        return self

    def digest(self):
        return lib().lz4mi_xxh32_digest(self._st.ctypes.data)


def compress_blocks(blocks):
    """Independent raw blocks -> list of compressed byte arrays (GPU)."""
    arrs = [_u8(b) for b in blocks]
    n = len(arrs)
    if n == 0:
        return []
    in_len = np.array([a.size for a in arrs], dtype=np.uint32)
    in_off = np.zeros(n, dtype=np.uint64)
    in_off[1:] = np.cumsum(in_len[:-1].astype(np.uint64))
    src = np.concatenate(arrs) if in_len.sum() else np.zeros(1, dtype=np.uint8)
    bounds = np.array([compress_bound(int(x)) for x in in_len], dtype=np.uint64)
    out_off = np.zeros(n, dtype=np.uint64)
    out_off[1:] = np.cumsum(bounds[:-1])
    out = np.zeros(int(bounds.sum()), dtype=np.uint8)
    out_len = np.zeros(n, dtype=np.uint32)
    _check(lib().lz4mi_compress_blocks(_p(src), _p(in_off), _p(in_len), _p(out), _p(out_off), _p(out_len), n, 0,
                                       None))
    return [out[int(o):int(o) + int(l)].copy() for o, l in zip(out_off, out_len)]


def compress_block(data):
    return compress_blocks([data])[0]


def compress_raw(src, output, src_start, src_len, hash_table, output_offset):
    """compressBlock(src, output, srcStart, srcLen, hashTable, outputOffset) with
    the reference's full semantics (table in/out, absolute positions)."""
    s = _u8(src)
    assert hash_table.dtype == np.int32 and hash_table.size == 16384 and hash_table.flags.c_contiguous
    assert output.dtype == np.uint8 and output.flags.c_contiguous
    r = lib().lz4mi_compress_block_table(_p(s), s.size, src_start, src_len, hash_table.ctypes.data,
                                         _p(output), output.size, output_offset or 0, 0, None)
    if r < 0:
        raise Lz4miError(int(r))
    return 0 if output_offset is None else int(r)   # (dIndex - undefined) | 0 (blockCompress.js:232)


def compress_chain(src, start, length, block_size, hash_table, host=False):
    """Dependent blocks in order with one carried table (lz4mi_compress_chain, or with `host`
    the host encoder lz4mi_host_compress_chain): returns the list of compressed blocks, each
    what compressBlock(src, scratch, start_b, n_b, table, 0) writes; hash_table (int32[16384])
    is updated in place."""
    s = _u8(src)
    assert hash_table.dtype == np.int32 and hash_table.size == 16384 and hash_table.flags.c_contiguous
    nb = -(-length // block_size) if length > 0 else 0
    if nb == 0:
        return []
    ns = [min(block_size, length - b * block_size) for b in range(nb)]
    bounds = np.array([compress_bound(n) for n in ns], dtype=np.uint64)
    out_off = np.zeros(nb, dtype=np.uint64)
    out_off[1:] = np.cumsum(bounds[:-1])
    out = np.zeros(int(bounds.sum()), dtype=np.uint8)
    comp_len = np.zeros(nb, dtype=np.uint32)
    if host:
        _check(lib().lz4mi_host_compress_chain(_p(s), s.size, start, length, block_size, hash_table.ctypes.data,
                                               _p(out), _p(out_off), _p(comp_len)))
    else:
        _check(lib().lz4mi_compress_chain(_p(s), s.size, start, length, block_size, hash_table.ctypes.data,
                                          _p(out), _p(out_off), _p(comp_len), 0, None))
    return [out[int(o):int(o) + int(n)].copy() for o, n in zip(out_off, comp_len)]


def host_decompress_raw(inp, input_offset, input_size, output, output_offset=0, dictionary=None, spec=False):
    """decompressBlock on the host decoder (lz4mi_host_decompress_block): writes into `output`
    (numpy uint8, the whole output array) and returns bytes written; raises with the reference's
    message. Reference bytes (F1 included) unless `spec`."""
    a = _u8(inp)
    d = None if dictionary is None else _u8(dictionary)
    assert output.dtype == np.uint8 and output.flags.c_contiguous
    r = lib().lz4mi_host_decompress_block(_p(a), a.size, input_offset, input_size, _p(output), output.size,
                                          output_offset, None if d is None else _p(d), 0 if d is None else d.size,
                                          0 if spec else JS_EXACT)
    if r < 0:
        raise Lz4miError(int(r))
    return int(r)


def host_compress_raw(src, output, src_start, src_len, hash_table, output_offset):
    """compressRaw on the host encoder (lz4mi_host_compress_block): the same contract as
    compress_raw, no device involved."""
    s = _u8(src)
    assert hash_table.dtype == np.int32 and hash_table.size == 16384 and hash_table.flags.c_contiguous
    assert output.dtype == np.uint8 and output.flags.c_contiguous
    r = lib().lz4mi_host_compress_block(_p(s), s.size, src_start, src_len, hash_table.ctypes.data, _p(output),
                                        output.size, output_offset or 0)
    if r < 0:
        raise Lz4miError(int(r))
    return 0 if output_offset is None else int(r)


def _dec_flags(js_compat, js_exact):
    return JS_COMPAT if js_compat else (JS_EXACT if js_exact else 0)


def _linked_flag(linked):
    """linked=True: LZ4MI_LINKED (spec mode); linked="exact": LZ4MI_LINKED_EXACT (the reference's bytes)."""
    if isinstance(linked, str):
        if linked != "exact":
            raise ValueError("linked: True, False or 'exact'")
        return LINKED_EXACT
    return LINKED if linked else 0


def _pack(arrs):
    n = len(arrs)
    in_len = np.array([a.size for a in arrs], dtype=np.uint32)
    in_off = np.zeros(n, dtype=np.uint64)
    if n > 1:
        in_off[1:] = np.cumsum(in_len[:-1].astype(np.uint64))
    src = np.concatenate(arrs) if n and in_len.sum() else np.zeros(1, dtype=np.uint8)
    return src, in_off, in_len


def decoded_sizes(blocks):
    """Independent compressed blocks -> (statuses, sizes): what each block decodes to, measured
    on the GPU without decoding (lz4mi_decoded_sizes; statuses 0, ERR_MALFORMED, ERR_OFFSET0, or
    ERR_OUTPUT_TOO_SMALL above 2^31 - 1 bytes)."""
    arrs = [_u8(b) for b in blocks]
    n = len(arrs)
    src, in_off, in_len = _pack(arrs)
    sizes = np.zeros(n, dtype=np.uint32)
    status = np.zeros(n, dtype=np.int32)
    if n:
        _check(lib().lz4mi_decoded_sizes(_p(src), _p(in_off), _p(in_len), _p(sizes), _p(status), n, 0, None))
    return status, sizes


def host_decoded_size(comp, in_off=0, in_size=None):
    """Decoded size of comp[in_off : in_off + in_size] on the host walker (lz4mi_host_decoded_size,
    no device needed) -> (status, size)."""
    a = _u8(comp)
    if in_size is None:
        in_size = a.size - in_off
    st = ctypes.c_int32(0)
    r = lib().lz4mi_host_decoded_size(_p(a), a.size, in_off, in_size, ctypes.addressof(st))
    if r < 0:
        raise Lz4miError(int(r))
    return int(st.value), int(r)


def host_block_read_end(comp, in_off=0, in_size=None):
    """Where the reference's walk of comp[in_off : in_off + in_size] stops reading (host, no device
    needed; lz4mi_host_block_read_end): above in_off + in_size when the block reads past its end."""
    a = _u8(comp)
    if in_size is None:
        in_size = a.size - in_off
    r = lib().lz4mi_host_block_read_end(_p(a), a.size, in_off, in_size)
    if r < 0:
        raise Lz4miError(int(r))
    return int(r)


def decompress_blocks(blocks, out_sizes=None, js_compat=False, dictionary=None, js_exact=False, linked=False):
    """Independent compressed blocks -> (statuses, outputs) (GPU).
    linked: the blocks may reference the output of the blocks before them (LZ4MI_LINKED: the
    blocks of a dependent frame in order; the outputs lie back to back); after the first
    failing block every later one reports ERR_CROSS_BLOCK. Spec mode; linked="exact"
    (LZ4MI_LINKED_EXACT): the reference decoder's bytes, what it leaves in one array after decoding
    the blocks in order -- its tail rewrite reaches up to 4 bytes into the block before.
    out_sizes=None: the sizes are measured first (decoded_sizes) and the blocks decoded at them;
    a block the size pass fails keeps that status and decodes to nothing.
    js_compat: the serial reference-exact kernel; js_exact: the parallel spec
    kernel plus a serial re-decode of the blocks the reference's F1 rewrite changes."""
    if out_sizes is None:
        blocks = list(blocks)
        mst, msz = decoded_sizes(blocks)
        ok = mst == OK
        st, outs, out_len = decompress_blocks([b if k else b"" for b, k in zip(blocks, ok)],
                                              [int(z) if k else 0 for z, k in zip(msz, ok)], js_compat=js_compat,
                                              dictionary=dictionary, js_exact=js_exact, linked=linked)
        st = np.where(ok, st, mst).astype(np.int32)
        return st, outs, out_len
    arrs = [_u8(b) for b in blocks]
    n = len(arrs)
    in_len = np.array([a.size for a in arrs], dtype=np.uint32)
    in_off = np.zeros(n, dtype=np.uint64)
    if n > 1:
        in_off[1:] = np.cumsum(in_len[:-1].astype(np.uint64))
    src = np.concatenate(arrs) if n and in_len.sum() else np.zeros(1, dtype=np.uint8)
    out_cap = np.array(out_sizes, dtype=np.uint32)
    out_off = np.zeros(n, dtype=np.uint64)
    if n > 1:
        out_off[1:] = np.cumsum(out_cap[:-1].astype(np.uint64))
    out = np.zeros(max(1, int(out_cap.sum())), dtype=np.uint8)
    out_len = np.zeros(n, dtype=np.uint32)
    status = np.zeros(n, dtype=np.int32)
    d = _u8(dictionary)
    _check(lib().lz4mi_decompress_blocks(_p(src), _p(in_off), _p(in_len), _p(out), _p(out_off), _p(out_cap),
                                         _p(d), 0 if d is None else d.size, _p(out_len), _p(status), n,
                                         _dec_flags(js_compat, js_exact) | _linked_flag(linked), None))
    outs = [out[int(o):int(o) + min(int(l), int(c))].copy() for o, l, c in zip(out_off, out_len, out_cap)]
    return status, outs, out_len


def decompress_raw(inp, input_offset, input_size, output, output_offset=0, dictionary=None, js_compat=False,
                   js_exact=False):
    """decompressBlock(input, inputOffset, inputSize, output, outputOffset, dictionary):
    writes into `output` (numpy uint8) and returns bytes written; raises with the
    reference's message on error."""
    a = _u8(inp)
    seg = a[input_offset:input_offset + input_size]
    in_off = np.zeros(1, dtype=np.uint64)
    in_len = np.array([seg.size], dtype=np.uint32)
    out_off = np.array([output_offset], dtype=np.uint64)
    out_cap = np.array([max(0, output.size - output_offset)], dtype=np.uint32)
    out_len = np.zeros(1, dtype=np.uint32)
    status = np.zeros(1, dtype=np.int32)
    d = _u8(dictionary)
    seg = np.ascontiguousarray(seg) if seg.size else np.zeros(1, dtype=np.uint8)
    _check(lib().lz4mi_decompress_blocks(_p(seg), _p(in_off), _p(in_len), _p(output), _p(out_off), _p(out_cap),
                                         _p(d), 0 if d is None else d.size, _p(out_len), _p(status), 1,
                                         _dec_flags(js_compat, js_exact), None))
    if status[0] != OK:
        raise Lz4miError(int(status[0]))
    return int(out_len[0])


def xxh32_blocks(blocks, seed=0, standard=False):
    arrs = [_u8(b) for b in blocks]
    n = len(arrs)
    ln = np.array([a.size for a in arrs], dtype=np.uint32)
    off = np.zeros(n, dtype=np.uint64)
    if n > 1:
        off[1:] = np.cumsum(ln[:-1].astype(np.uint64))
    src = np.concatenate(arrs) if n and ln.sum() else np.zeros(1, dtype=np.uint8)
    h = np.zeros(n, dtype=np.uint32)
    _check(lib().lz4mi_xxh32_blocks(_p(src), _p(off), _p(ln), seed & 0xFFFFFFFF, _p(h), n,
                                    XXH_STANDARD if standard else 0, None))
    return h


def _records(buf, offs, lens_or_words):
    a = _u8(buf)
    off = np.ascontiguousarray(offs, dtype=np.uint64)
    ln = np.ascontiguousarray(np.asarray(lens_or_words, dtype=np.int64) & 0xFFFFFFFF, dtype=np.uint32)
    assert off.ndim == 1 and off.shape == ln.shape
    # (an empty buffer still needs an address: the call refuses NULL inputs)
    return a if a.size else np.zeros(1, dtype=np.uint8), a.size, off, ln


def verify_blocks(buf, offs, lens_or_words, frame_words=False):
    """Frame block checksums checked on the GPU (lz4mi_verify_blocks, host pointers): record b is the
    payload buf[offs[b] : offs[b] + n] and the LE32 behind it; -> int32 statuses, 0 or
    ERR_BLOCK_CHECKSUM (a record that buf's end cuts included). frame_words: the lengths are frame
    size words (bit 31 = stored, masked off)."""
    a, total, off, ln = _records(buf, offs, lens_or_words)
    status = np.zeros(off.size, dtype=np.int32)
    _check(lib().lz4mi_verify_blocks(_p(a), total, _p(off), _p(ln), status.ctypes.data, off.size,
                                     FRAME_WORDS if frame_words else 0, None))
    return status


def host_verify_blocks(buf, offs, lens_or_words, frame_words=False):
    """verify_blocks on the calling thread (lz4mi_host_verify_blocks, no device needed)."""
    a, total, off, ln = _records(buf, offs, lens_or_words)
    status = np.zeros(off.size, dtype=np.int32)
    _check(lib().lz4mi_host_verify_blocks(_p(a), total, _p(off), _p(ln), status.ctypes.data, off.size,
                                          FRAME_WORDS if frame_words else 0))
    return status


def host_frames_index(arena, frame_off, frame_len, cap_blocks, measure=False, js_exact=False):
    """lz4mi_frames_index on the calling thread (lz4mi_host_frames_index, no device needed): the frames
    arena[frame_off[f] : frame_off[f] + frame_len[f]] -> dict with finfo (nframes x 8 int64), totals (4 int64)
    and the block lists blk_in_off / blk_word / blk_frame / blk_size (cap_blocks entries each, the first
    totals[1] of them written)."""
    a = _u8(arena)
    off = np.ascontiguousarray(frame_off, dtype=np.uint64)
    ln = np.ascontiguousarray(frame_len, dtype=np.uint64)
    assert off.ndim == 1 and off.shape == ln.shape
    n = off.size
    res = {"finfo": np.zeros((n, 8), dtype=np.int64), "totals": np.zeros(4, dtype=np.int64),
           "blk_in_off": np.zeros(cap_blocks, dtype=np.uint64), "blk_word": np.zeros(cap_blocks, dtype=np.uint32),
           "blk_frame": np.zeros(cap_blocks, dtype=np.uint32), "blk_size": np.zeros(cap_blocks, dtype=np.uint32)}
    _check(lib().lz4mi_host_frames_index(_p(a) if a.size else np.zeros(1, dtype=np.uint8).ctypes.data, _p(off), _p(ln),
                                         n, _p(res["blk_in_off"]), _p(res["blk_word"]), _p(res["blk_frame"]),
                                         _p(res["blk_size"]), cap_blocks, res["finfo"].ctypes.data,
                                         res["totals"].ctypes.data,
                                         (FRAMES_MEASURE if measure else 0) | (JS_EXACT if js_exact else 0)))
    return res


def host_frames_verify_blocks(arena, frame_off, frame_len, index):
    """lz4mi_frames_verify_blocks on the calling thread (lz4mi_host_frames_verify_blocks, no device needed): the
    block checksums of the frames host_frames_index listed (`index`: its dict; nblocks is the lists' length).
    index["finfo"] is updated in place -- [0] of a checked frame with a failing record becomes
    ERR_BLOCK_CHECKSUM -- and blk_status (int32 per list entry: 0 or ERR_BLOCK_CHECKSUM) is returned."""
    a = _u8(arena)
    off = np.ascontiguousarray(frame_off, dtype=np.uint64)
    ln = np.ascontiguousarray(frame_len, dtype=np.uint64)
    fi = index["finfo"]
    assert off.ndim == 1 and off.shape == ln.shape and fi.shape == (off.size, 8)
    assert fi.dtype == np.int64 and fi.flags.c_contiguous
    nb = index["blk_in_off"].size
    status = np.zeros(nb, dtype=np.int32)
    _check(lib().lz4mi_host_frames_verify_blocks(_p(a) if a.size else np.zeros(1, dtype=np.uint8).ctypes.data, _p(off),
                                                 _p(ln), off.size, _p(index["blk_in_off"]), _p(index["blk_word"]),
                                                 _p(index["blk_frame"]), nb, _p(fi), _p(status), 0))
    return status


def host_frame_index(frame, pay_off, size_word, cap_blocks, info):
    """lz4mi_frame_index on the calling thread (lz4mi_host_frame_index, no device needed) into the caller's
    arrays: pay_off (uint64) and size_word (uint32), of which the first cap_blocks entries may be written, and
    info (8 x int64)."""
    a = _u8(frame)
    assert pay_off.dtype == np.uint64 and size_word.dtype == np.uint32 and info.dtype == np.int64 and info.size == 8
    assert cap_blocks <= min(pay_off.size, size_word.size)
    src = a if a.size else np.zeros(1, dtype=np.uint8)   # (an empty frame still needs an address)
    _check(lib().lz4mi_host_frame_index(_p(src), a.size, _p(pay_off), _p(size_word), cap_blocks, _p(info)))


def frame_bound(n, block_max=4194304):
    """lz4mi_frame_bound: no frame of the frame batch encoder for n source bytes is longer."""
    return int(lib().lz4mi_frame_bound(int(n), int(block_max) & 0xFFFFFFFF))


def frames_enc_flags(independent=True, content_checksum=False, add_content_size=True, block_checksum=False,
                     packed=False, chains=False):
    """The flags of lz4mi_frames_plan / lz4mi_frames_compress (without LZ4MI_DEVICE_PTRS). chains
    (LZ4MI_FRAMES_CHAINS, only with independent=False): dependent frames of more than one block are written too,
    one chain per frame."""
    return ((0 if independent else FRAMES_DEPENDENT) | (FRAMES_CONTENT_CHECKSUM if content_checksum else 0) |
            (0 if add_content_size else FRAMES_NO_CONTENT_SIZE) | (BLOCK_CHECKSUM if block_checksum else 0) |
            (FRAMES_PACKED if packed else 0) | (FRAMES_CHAINS if chains else 0))


def host_frames_plan(src_off, src_len, block_max, cap_blocks, flags=0):
    """lz4mi_frames_plan on the calling thread (lz4mi_host_frames_plan, no device needed) -> dict with finfo
    (nframes x 8 int64), totals (4 int64) and the block lists blk_in_off / blk_len / blk_frame / blk_work_off
    (cap_blocks entries each, the first totals[1] of them written). flags: frames_enc_flags()."""
    off = np.ascontiguousarray(src_off, dtype=np.uint64)
    ln = np.ascontiguousarray(src_len, dtype=np.uint64)
    assert off.ndim == 1 and off.shape == ln.shape
    n = off.size
    res = {"finfo": np.zeros((n, 8), dtype=np.int64), "totals": np.zeros(4, dtype=np.int64),
           "blk_in_off": np.zeros(cap_blocks, dtype=np.uint64), "blk_len": np.zeros(cap_blocks, dtype=np.uint32),
           "blk_frame": np.zeros(cap_blocks, dtype=np.uint32), "blk_work_off": np.zeros(cap_blocks, dtype=np.uint64)}
    _check(lib().lz4mi_host_frames_plan(_p(off), _p(ln), n, int(block_max) & 0xFFFFFFFF, _p(res["blk_in_off"]),
                                        _p(res["blk_len"]), _p(res["blk_frame"]), _p(res["blk_work_off"]), cap_blocks,
                                        res["finfo"].ctypes.data, res["totals"].ctypes.data, flags))
    return res


def host_frames_compress(arena, plan, out, flags=0, slots=None, work=None):
    """lz4mi_frames_compress on the calling thread (lz4mi_host_frames_compress, no device needed): the frames of
    `plan` (host_frames_plan's result over ranges of `arena`; its finfo is updated in place) into `out` (numpy
    uint8, written in place). slots: (frame_out_off, frame_out_cap), or None with FRAMES_PACKED in flags.
    work: the scratch (numpy uint8; default: totals[3] bytes). Returns finfo."""
    a = _u8(arena)
    assert out.dtype == np.uint8 and out.flags.c_contiguous
    nb = int(plan["totals"][1])
    if work is None:
        work = np.zeros(int(plan["totals"][3]), dtype=np.uint8)
    so = sc = None
    if slots is not None:
        so = np.ascontiguousarray(slots[0], dtype=np.uint64)
        sc = np.ascontiguousarray(slots[1], dtype=np.uint64)
    fi = plan["finfo"]
    _check(lib().lz4mi_host_frames_compress(_p(a), _p(plan["blk_in_off"]), _p(plan["blk_len"]), _p(plan["blk_frame"]),
                                            _p(plan["blk_work_off"]), nb, fi.ctypes.data, fi.shape[0], _p(work),
                                            work.size, out.ctypes.data, out.size, None if so is None else _p(so),
                                            None if sc is None else _p(sc), flags))
    return fi


# -------------------------------------------------------------- device API
# Raw device pointers (ints, e.g. torch tensor .data_ptr()) and a hipStream_t
# handle (int, e.g. torch.cuda.current_stream().cuda_stream). Async.
def decompress_blocks_dev(in_ptr, in_off_ptr, in_len_ptr, out_ptr, out_off_ptr, out_cap_ptr, out_len_ptr,
                          status_ptr, nblocks, stream=0, js_compat=False, dict_ptr=None, dict_len=0,
                          frame_words=False, js_exact=False, linked=False):
    """Batch decode on device pointers. frame_words: in_len holds frame size words (bit 31 =
    stored block, copied in the same launch; include/lz4mi.h LZ4MI_FRAME_WORDS). js_exact: the
    reference decoder's bytes (LZ4MI_JS_EXACT, the JS layer's default). linked: dependent blocks
    in ascending, disjoint slots (LZ4MI_LINKED, spec mode; "exact": LZ4MI_LINKED_EXACT, the reference's bytes)."""
    _check(lib().lz4mi_decompress_blocks(in_ptr, in_off_ptr, in_len_ptr, out_ptr, out_off_ptr, out_cap_ptr,
                                         dict_ptr, dict_len, out_len_ptr, status_ptr, nblocks,
                                         DEVICE_PTRS | _dec_flags(js_compat, js_exact) |
                                         (FRAME_WORDS if frame_words else 0) | _linked_flag(linked),
                                         stream or None))


def decoded_sizes_dev(in_ptr, in_off_ptr, in_len_ptr, out_len_ptr, status_ptr, nblocks, stream=0, frame_words=False):
    """Decoded sizes of a batch on device pointers (lz4mi_decoded_sizes): asynchronous on `stream`,
    nothing read back. frame_words: in_len holds frame size words (bit 31 = stored block)."""
    _check(lib().lz4mi_decoded_sizes(in_ptr, in_off_ptr, in_len_ptr, out_len_ptr, status_ptr, nblocks,
                                     DEVICE_PTRS | (FRAME_WORDS if frame_words else 0), stream or None))


def verify_blocks_dev(in_ptr, in_total, in_off_ptr, in_len_ptr, status_ptr, nblocks, stream=0, frame_words=False):
    """Block checksums of a batch on device pointers (lz4mi_verify_blocks): asynchronous on `stream`,
    nothing read back; status 0 or ERR_BLOCK_CHECKSUM per record. in_total: the size of the buffer at
    in_ptr (nothing past it is read). frame_words: in_len holds frame size words."""
    _check(lib().lz4mi_verify_blocks(in_ptr, in_total, in_off_ptr, in_len_ptr, status_ptr, nblocks,
                                     DEVICE_PTRS | (FRAME_WORDS if frame_words else 0), stream or None))


def compress_blocks_dev(in_ptr, in_off_ptr, in_len_ptr, out_ptr, out_off_ptr, out_len_ptr, nblocks, stream=0):
    _check(lib().lz4mi_compress_blocks(in_ptr, in_off_ptr, in_len_ptr, out_ptr, out_off_ptr, out_len_ptr, nblocks,
                                       DEVICE_PTRS, stream or None))


def xxh32_blocks_dev(in_ptr, off_ptr, len_ptr, hashes_ptr, nblocks, seed=0, stream=0, standard=False):
    _check(lib().lz4mi_xxh32_blocks(in_ptr, off_ptr, len_ptr, seed & 0xFFFFFFFF, hashes_ptr, nblocks,
                                    DEVICE_PTRS | (XXH_STANDARD if standard else 0), stream or None))


def frame_decompress_dev(frame_ptr, frame_len, out_ptr, out_cap, stream=0, js_exact=False, linked=False,
                         verify_blocks=False):
    """Decode a device-resident LZ4 frame into out (device pointers): returns the info dict
    (include/lz4mi.h lz4mi_frame_decompress); raises if the frame needs the host path.
    linked: the compressed blocks go in one linked call (LZ4MI_LINKED, not with js_exact; "exact":
    LZ4MI_LINKED_EXACT, that call in the reference decoder's bytes). verify_blocks: block checksums
    (FLG 0x10) are checked on the device (LZ4MI_VERIFY_BLOCKS): a mismatch is status
    ERR_BLOCK_CHECKSUM with written 0."""
    info = np.zeros(8, dtype=np.int64)
    _check(lib().lz4mi_frame_decompress(frame_ptr, frame_len, out_ptr, out_cap, info.ctypes.data,
                                        DEVICE_PTRS | (JS_EXACT if js_exact else 0) | _linked_flag(linked) |
                                        (VERIFY_BLOCKS if verify_blocks else 0), stream or None))
    keys = ("status", "flg", "content_size", "written", "stored_blocks", "checksum_pos", "block_max", "overflow")
    return dict(zip(keys, (int(x) for x in info)))


def frames_index_dev(in_ptr, frame_off_ptr, frame_len_ptr, nframes, blk_in_off_ptr, blk_word_ptr, blk_frame_ptr,
                     blk_size_ptr, cap_blocks, finfo_ptr, totals_ptr, stream=0, measure=False, js_exact=False):
    """Block index of a batch of device-resident frames (include/lz4mi.h lz4mi_frames_index): device pointers,
    asynchronous on `stream`, nothing read back. measure: LZ4MI_FRAMES_MEASURE; js_exact: unsized frames are
    declined."""
    _check(lib().lz4mi_frames_index(in_ptr, frame_off_ptr, frame_len_ptr, nframes, blk_in_off_ptr, blk_word_ptr,
                                    blk_frame_ptr, blk_size_ptr, cap_blocks, finfo_ptr, totals_ptr,
                                    DEVICE_PTRS | (FRAMES_MEASURE if measure else 0) | (JS_EXACT if js_exact else 0),
                                    stream or None))


def frames_verify_blocks_dev(in_ptr, frame_off_ptr, frame_len_ptr, nframes, blk_in_off_ptr, blk_word_ptr, blk_frame_ptr,
                             nblocks, finfo_ptr, blk_status_ptr, stream=0):
    """Block checksums of the frames lz4mi_frames_index listed (include/lz4mi.h lz4mi_frames_verify_blocks): device
    pointers, asynchronous on `stream`, nothing read back. blk_status holds 0 or ERR_BLOCK_CHECKSUM per list entry
    afterwards, and finfo[f][0] of a frame with a failing record ERR_BLOCK_CHECKSUM, so frames_decompress_dev
    passes it over."""
    _check(lib().lz4mi_frames_verify_blocks(in_ptr, frame_off_ptr, frame_len_ptr, nframes, blk_in_off_ptr, blk_word_ptr,
                                            blk_frame_ptr, nblocks, finfo_ptr, blk_status_ptr, DEVICE_PTRS,
                                            stream or None))


def frames_decompress_dev(in_ptr, blk_in_off_ptr, blk_word_ptr, blk_frame_ptr, blk_size_ptr, nblocks, finfo_ptr,
                          nframes, out_ptr, frame_out_off_ptr, frame_out_cap_ptr, stream=0, js_exact=False,
                          verify_content=False, chains=False):
    """Decode the frames lz4mi_frames_index listed, in one call (include/lz4mi.h lz4mi_frames_decompress): device
    pointers, asynchronous on `stream`; finfo holds each frame's status, bytes written and decline code afterwards.
    verify_content: LZ4MI_VERIFY_CONTENT, the content checksums on the device. chains: LZ4MI_FRAMES_CHAINS, frames
    with dependent blocks are decoded in the call too, one wave per frame in block order."""
    _check(lib().lz4mi_frames_decompress(in_ptr, blk_in_off_ptr, blk_word_ptr, blk_frame_ptr, blk_size_ptr, nblocks,
                                         finfo_ptr, nframes, out_ptr, frame_out_off_ptr, frame_out_cap_ptr,
                                         DEVICE_PTRS | (JS_EXACT if js_exact else 0) |
                                         (VERIFY_CONTENT if verify_content else 0) |
                                         (FRAMES_CHAINS if chains else 0), stream or None))


def frames_plan_dev(src_off_ptr, src_len_ptr, nframes, block_max, blk_in_off_ptr, blk_len_ptr, blk_frame_ptr,
                    blk_work_off_ptr, cap_blocks, finfo_ptr, totals_ptr, stream=0, flags=0):
    """Block plan of a batch of device-resident buffers (include/lz4mi.h lz4mi_frames_plan): device pointers,
    asynchronous on `stream`, nothing read back. flags: frames_enc_flags()."""
    _check(lib().lz4mi_frames_plan(src_off_ptr, src_len_ptr, nframes, int(block_max) & 0xFFFFFFFF, blk_in_off_ptr,
                                   blk_len_ptr, blk_frame_ptr, blk_work_off_ptr, cap_blocks, finfo_ptr, totals_ptr,
                                   DEVICE_PTRS | flags, stream or None))


def frames_compress_dev(in_ptr, blk_in_off_ptr, blk_len_ptr, blk_frame_ptr, blk_work_off_ptr, nblocks, finfo_ptr,
                        nframes, work_ptr, work_bytes, out_ptr, out_total, frame_out_off_ptr=None,
                        frame_out_cap_ptr=None, stream=0, flags=0):
    """Compress the buffers lz4mi_frames_plan listed into one frame each, in one call (include/lz4mi.h
    lz4mi_frames_compress): device pointers, asynchronous on `stream`; finfo holds each frame's length, position
    and decline code afterwards. flags: frames_enc_flags(), the plan's; with packed the slot arrays may be None."""
    _check(lib().lz4mi_frames_compress(in_ptr, blk_in_off_ptr, blk_len_ptr, blk_frame_ptr, blk_work_off_ptr, nblocks,
                                       finfo_ptr, nframes, work_ptr, work_bytes, out_ptr, out_total, frame_out_off_ptr,
                                       frame_out_cap_ptr, DEVICE_PTRS | flags, stream or None))


def generate_blocks_dev(out_ptr, kind, seed0, block_size, nblocks, stream=0):
    k = GENERATORS[kind] if isinstance(kind, str) else kind
    _check(lib().lz4mi_generate_blocks(out_ptr, k, seed0, block_size, nblocks, stream or None))


def frame_pack_dev(raw_ptr, raw_off_ptr, raw_len_ptr, comp_ptr, comp_off_ptr, comp_len_ptr, frame_ptr, rec_off_ptr,
                   nblocks, stream=0, block_checksum=False):
    """Device-side frame block records (size word + compressed or stored payload [+ XXH32 of
    the payload with block_checksum]) at rec_off."""
    _check(lib().lz4mi_frame_pack(raw_ptr, raw_off_ptr, raw_len_ptr, comp_ptr, comp_off_ptr, comp_len_ptr, frame_ptr,
                                  rec_off_ptr, nblocks, DEVICE_PTRS | (BLOCK_CHECKSUM if block_checksum else 0),
                                  stream or None))


def frame_index_dev(frame_ptr, frame_len, pay_off_ptr, size_word_ptr, cap_blocks, info_ptr, stream=0):
    """Block index of a device-resident frame (include/lz4mi.h lz4mi_frame_index): device
    pointers, asynchronous on `stream`."""
    _check(lib().lz4mi_frame_index(frame_ptr, frame_len, pay_off_ptr, size_word_ptr, cap_blocks, info_ptr,
                                   DEVICE_PTRS, stream or None))
