"""LZ4MI_FRAMES_CHAINS on the decode side (lz4mi_frames_decompress, include/lz4mi.h): what can be checked
without a GPU -- the flag and NULL checks, which run before a device is looked for, the Python wrappers'
parameter, the header's text, and the claims of the inputs that tests/test_gpu_frames_chains_decode.py decodes
(tests/frames_chains_decode_common.py)."""
import inspect
import os

import numpy as np

import frames_chains_decode_common as D
import frames_common as C
import lz4mi

CH = 0x10000
DEV = lz4mi.DEVICE_PTRS


def has_gpu():
    try:
        return lz4mi.device_count() > 0 and lz4mi.lib().lz4mi_init(0) == 0
    except Exception:
        return False


def host_args():
    """Valid arguments in host memory: only for calls that return before anything is launched."""
    a, off, ln = C.arena(0)
    n = len(C.NAMES)
    fi = np.zeros(8 * n, dtype=np.int64)
    lists = [np.zeros(8, dtype=np.uint64)] + [np.zeros(8, dtype=np.uint32) for _ in range(3)]
    out = np.zeros(64, dtype=np.uint8)
    keep = (a, off, ln, fi, lists, out)
    return [a.ctypes.data, *[x.ctypes.data for x in lists], 8, fi.ctypes.data, n, out.ctypes.data, off.ctypes.data,
            ln.ctypes.data], keep


def test_the_inputs_claims_hold_on_the_oracle():
    assert D.claims()


def test_decompress_takes_the_flag():
    L = lz4mi.lib()
    assert lz4mi.FRAMES_CHAINS == CH
    if has_gpu():
        # no frames: the call returns behind its checks, before it launches anything
        z = np.zeros(8, dtype=np.uint64).ctypes.data
        for extra in (0, lz4mi.JS_EXACT, lz4mi.VERIFY_CONTENT, lz4mi.JS_EXACT | lz4mi.VERIFY_CONTENT):
            assert L.lz4mi_frames_decompress(z, z, z, z, z, 0, z, 0, z, z, z, DEV | CH | extra, None) == 0, extra
        return
    dargs, keep = host_args()
    for extra in (0, lz4mi.JS_EXACT, lz4mi.VERIFY_CONTENT, lz4mi.JS_EXACT | lz4mi.VERIFY_CONTENT):
        assert L.lz4mi_frames_decompress(*dargs, DEV | CH | extra, None) == lz4mi.ERR_NO_DEVICE, extra
    assert L.lz4mi_frames_decompress(*dargs, DEV, None) == lz4mi.ERR_NO_DEVICE


def test_flag_combinations_and_null_pointers_are_refused_before_a_device_is_looked_for():
    L = lz4mi.lib()
    dargs, keep = host_args()
    for extra in (lz4mi.LINKED, lz4mi.LINKED_EXACT, lz4mi.VERIFY_BLOCKS, lz4mi.FRAMES_MEASURE, lz4mi.JS_COMPAT,
                  lz4mi.FRAMES_DEPENDENT, lz4mi.FRAMES_PACKED):
        assert L.lz4mi_frames_decompress(*dargs, DEV | CH | extra, None) == lz4mi.ERR_ARG, extra
    assert L.lz4mi_frames_decompress(*dargs, CH, None) == lz4mi.ERR_ARG          # host pointers
    for k in (0, 1, 2, 3, 4, 6, 8, 9, 10):                                         # every required pointer
        args = list(dargs)
        args[k] = None
        assert L.lz4mi_frames_decompress(*args, DEV | CH, None) == lz4mi.ERR_ARG, k
    # an array the call writes (finfo, out) that is one it reads, or the other one
    for w in (6, 8):
        for r in (0, 1, 2, 3, 4, 9, 10, 14 - w):
            args = list(dargs)
            args[w] = args[r]
            assert L.lz4mi_frames_decompress(*args, DEV | CH, None) == lz4mi.ERR_ARG, (w, r)


def test_index_still_refuses_the_flag():
    L = lz4mi.lib()
    a, off, ln = C.arena(0)
    n = len(C.NAMES)
    fi, tot = np.zeros(8 * n, dtype=np.int64), np.zeros(4, dtype=np.int64)
    lists = [np.zeros(8, dtype=np.uint64)] + [np.zeros(8, dtype=np.uint32) for _ in range(3)]
    args = [a.ctypes.data, off.ctypes.data, ln.ctypes.data, n, *[x.ctypes.data for x in lists], 8, fi.ctypes.data,
            tot.ctypes.data]
    for extra in (0, lz4mi.JS_EXACT, lz4mi.FRAMES_MEASURE):
        assert L.lz4mi_frames_index(*args, DEV | CH | extra, None) == lz4mi.ERR_ARG
        assert L.lz4mi_host_frames_index(*args, CH | extra) == lz4mi.ERR_ARG


def test_wrappers_accept_chains():
    from lz4mi import frame as F
    for fn in (lz4mi.frames_decompress_dev, F.decompress_frames_device):
        p = inspect.signature(fn).parameters.get("chains")
        assert p is not None and p.default is False, fn.__name__
    assert "chains" not in inspect.signature(lz4mi.frames_index_dev).parameters


def test_header_declares_the_flag_for_the_call():
    with open(os.path.join(os.path.dirname(lz4mi.PKG_DIR), "include", "lz4mi.h")) as f:
        header = f.read()
    assert "#define LZ4MI_FRAMES_CHAINS 0x10000u" in header
    doc = header[header.index(" * lz4mi_frames_decompress takes the lists"):header.index("int32_t lz4mi_frames_index(")]
    flags = doc[doc.index(" * flags: LZ4MI_DEVICE_PTRS"):]
    assert "LZ4MI_FRAMES_CHAINS" in flags.split("Any other")[0]
    assert "frames with dependent blocks are declined" not in doc
    assert "LZ4MI_LINKED* and" in doc and "are not taken" in doc
