"""lz4mi_host_frames_index -- the host checker of the frame batch's device passes (include/lz4mi.h) -- against
shard.frame_blocks, the oracle's frame decoder and lz4mi_host_decoded_size, on the zoo of
tests/frames_common.py. No GPU needed."""
import numpy as np
import pytest

import frames_common as C
import lz4mi
import oracle as O
from lz4mi import shard


def index(fill=0x00, cap=None, **kw):
    a, off, ln = C.arena(fill)
    return lz4mi.host_frames_index(a, off, ln, C.need_blocks() if cap is None else cap, **kw), a, off, ln


@pytest.mark.parametrize("fill", C.FILLS)
def test_blocks_are_those_of_the_frame_alone(fill):
    r, a, off, ln = index(fill)
    fi = r["finfo"]
    assert r["totals"][0] == r["totals"][1] == C.need_blocks()
    at = 0
    for k, name in enumerate(C.NAMES):
        st, dc = C.expected_index(name)
        if st or dc in (C.PAST_END, C.EMPTY):
            continue
        _, blocks = shard.frame_blocks(C.zoo()[name])
        n = len(blocks)
        assert (fi[k, 4], fi[k, 6]) == (at, n), name
        assert r["blk_in_off"][at:at + n].tolist() == [int(off[k]) + p for p, _, _ in blocks], name
        assert r["blk_word"][at:at + n].tolist() == [nb | (0x80000000 if s else 0) for _, nb, s in blocks], name
        assert (r["blk_frame"][at:at + n] == k).all(), name
        at += n
    assert at == C.need_blocks()


def test_header_fields_and_totals_are_the_oracles():
    r, a, off, ln = index(0xFF)
    fi = r["finfo"]
    for k, name in enumerate(C.NAMES):
        f = C.zoo()[name]
        st, dc = C.expected_index(name)
        assert (fi[k, 0], fi[k, 7]) == (st, dc), name
        if st:
            continue
        info, blocks = shard.frame_blocks(f)
        assert fi[k, 1] & 0xFF == info["flg"] and (fi[k, 1] >> 8) & 0xFF == int(f[5]) if f.size > 5 else True, name
        assert fi[k, 2] == info["content_size"] and fi[k, 5] == info["end"] and fi[k, 6] == len(blocks), name
        if dc == 0 and info["flg"] & 0x04:
            want = int.from_bytes(bytes(f[info["end"]:info["end"] + 4]).ljust(4, b"\0"), "little")
            assert (int(fi[k, 1]) >> 32) & 0xFFFFFFFF == want, name
        if dc:
            continue
        # the decoded total: what the oracle's decoder returns for a frame it decodes, the content size (the
        # reference's zero-initialised result) for a sized frame one of whose blocks fails
        ost, out = O.decompress_frame(f, verify_checksum=False)
        assert fi[k, 3] == (out.size if ost == 0 else info["content_size"]), (name, ost)
        assert bool(fi[k, 1] & (1 << 16)) == (not info["flg"] & 0x08), name


@pytest.mark.parametrize("js_exact,measure", [(False, False), (True, False), (False, True), (True, True)])
def test_decline_codes_by_name(js_exact, measure):
    r, *_ = index(js_exact=js_exact, measure=measure)
    got = {n: (int(r["finfo"][k, 0]), int(r["finfo"][k, 7])) for k, n in enumerate(C.NAMES)}
    want = {n: C.expected_index(n, js_exact, measure) for n in C.NAMES}
    assert got == want
    assert r["totals"][3] == sum(1 for v in want.values() if v[1])
    # the expectations are not hollow: every index-time code has a frame
    assert {v[1] for v in want.values()} >= {0, C.PAST_END, C.EMPTY} | ({C.UNSIZED_EXACT} if js_exact else set()) | \
        ({C.MEASURE, C.SIZE_MISMATCH} if measure else set())


def test_sizes_layout_and_measured():
    """blk_size: the reference encoder's layout for sized frames, lz4mi_host_decoded_size for measured ones."""
    for measure in (False, True):
        r, a, off, ln = index(measure=measure)
        fi = r["finfo"]
        for k, name in enumerate(C.NAMES):
            if fi[k, 0] or fi[k, 7] in (C.PAST_END, C.EMPTY):
                continue
            first, n = int(fi[k, 4]), int(fi[k, 6])
            words = r["blk_word"][first:first + n]
            got = r["blk_size"][first:first + n].tolist()
            if fi[k, 1] & (1 << 16):
                want = []
                for b in range(first, first + n):
                    w = int(r["blk_word"][b])
                    if w & 0x80000000:
                        want.append(w & 0x7FFFFFFF)
                    else:
                        p = int(r["blk_in_off"][b])
                        want.append(lz4mi.host_decoded_size(a[p:p + w])[1])
                assert got == want, name
                assert measure or not fi[k, 1] & 0x08, name
            else:
                size, pos, want = int(fi[k, 2]), 0, []
                for w in words.tolist():
                    if w & 0x80000000:
                        want.append(w & 0x7FFFFFFF)
                        pos += w & 0x7FFFFFFF
                    else:
                        want.append(max(0, min(C.BS, size - pos)))
                        pos += C.BS
                assert got == want, name
    # the partial-block frame: 65536 + 30000 + 65536 measured, 65536 + 65536 + 30000 by the layout
    k = C.NAMES.index("partial_sized")
    r, *_ = index()
    assert r["blk_size"][int(r["finfo"][k, 4]):][:3].tolist() == [65536, 65536, 30000]
    r, *_ = index(measure=True)
    assert r["blk_size"][int(r["finfo"][k, 4]):][:3].tolist() == list(C.PARTIAL) and r["finfo"][k, 7] == 0


def test_cap_blocks_one_short():
    need = C.need_blocks()
    full, a, off, ln = index()
    r, *_ = index(cap=need - 1)
    assert r["totals"][0] == need
    fi, ff = r["finfo"], full["finfo"]
    # the last frame with blocks overflows: every frame before it is listed as before, it lists none
    last = max(k for k in range(len(C.NAMES)) if ff[k, 6] and not ff[k, 0] and ff[k, 7] not in (C.PAST_END, C.EMPTY))
    for k in range(len(C.NAMES)):
        if k == last:
            assert fi[k, 7] == C.CAP_BLOCKS and fi[k, 4] == ff[k, 4]
        else:
            assert (fi[k] == ff[k]).all(), C.NAMES[k]
    listed = need - int(ff[last, 6])
    assert r["totals"][1] == listed
    for key in ("blk_in_off", "blk_word", "blk_frame", "blk_size"):
        assert (r[key][:listed] == full[key][:listed]).all() and not r[key][listed:].any(), key
    # an earlier frame overflowing: the frames before it are listed, it and every later frame with blocks are not
    r, *_ = index(cap=int(ff[10, 4]) + int(ff[10, 6]) - 1)
    assert r["totals"][0] == need and r["totals"][1] == ff[10, 4]
    assert (r["finfo"][:10] == ff[:10]).all() and r["finfo"][10, 7] == C.CAP_BLOCKS


def test_flag_and_null_checks_need_no_device():
    L = lz4mi.lib()
    a, off, ln = C.arena(0)
    n = len(C.NAMES)
    fi, tot = np.zeros(8 * n, dtype=np.int64), np.zeros(4, dtype=np.int64)
    lists = [np.zeros(8, dtype=np.uint64)] + [np.zeros(8, dtype=np.uint32) for _ in range(3)]
    lp = [x.ctypes.data for x in lists]
    args = [a.ctypes.data, off.ctypes.data, ln.ctypes.data, n, *lp, 8, fi.ctypes.data, tot.ctypes.data]
    assert L.lz4mi_host_frames_index(*args, lz4mi.DEVICE_PTRS) == lz4mi.ERR_ARG
    assert L.lz4mi_host_frames_index(*args, lz4mi.VERIFY_CONTENT) == lz4mi.ERR_ARG
    assert L.lz4mi_host_frames_index(*args[:9], None, args[10], 0) == lz4mi.ERR_ARG
    assert L.lz4mi_host_frames_index(None, *args[1:], 0) == lz4mi.ERR_ARG
    assert L.lz4mi_host_frames_index(*args[:4], None, *args[5:], 0) == lz4mi.ERR_ARG
    # the device calls refuse before they look for a device: no device pointers, a foreign flag, NULL pointers
    for flags in (0, lz4mi.DEVICE_PTRS | lz4mi.LINKED, lz4mi.DEVICE_PTRS | lz4mi.VERIFY_BLOCKS,
                  lz4mi.DEVICE_PTRS | lz4mi.VERIFY_CONTENT):
        assert L.lz4mi_frames_index(*args, flags, None) == lz4mi.ERR_ARG, flags
    assert L.lz4mi_frames_index(*args[:9], None, args[10], lz4mi.DEVICE_PTRS, None) == lz4mi.ERR_ARG
    assert L.lz4mi_frames_index(*args[:9], args[9], None, lz4mi.DEVICE_PTRS, None) == lz4mi.ERR_ARG
    dargs = [a.ctypes.data, *lp, 8, fi.ctypes.data, n, a.ctypes.data, off.ctypes.data, ln.ctypes.data]
    for flags in (0, lz4mi.DEVICE_PTRS | lz4mi.LINKED, lz4mi.DEVICE_PTRS | lz4mi.LINKED_EXACT,
                  lz4mi.DEVICE_PTRS | lz4mi.VERIFY_BLOCKS, lz4mi.DEVICE_PTRS | lz4mi.FRAMES_MEASURE,
                  lz4mi.DEVICE_PTRS | lz4mi.JS_COMPAT):
        assert L.lz4mi_frames_decompress(*dargs, flags, None) == lz4mi.ERR_ARG, flags
    assert L.lz4mi_frames_decompress(*dargs[:6], None, *dargs[7:], lz4mi.DEVICE_PTRS, None) == lz4mi.ERR_ARG
    assert L.lz4mi_frames_decompress(*dargs[:8], None, *dargs[9:], lz4mi.DEVICE_PTRS, None) == lz4mi.ERR_ARG
    assert L.lz4mi_frames_decompress(*dargs[:1], None, *dargs[2:], lz4mi.DEVICE_PTRS, None) == lz4mi.ERR_ARG


def test_symbols_exported_and_declared():
    import os
    with open(os.path.join(os.path.dirname(lz4mi.PKG_DIR), "include", "lz4mi.h")) as f:
        header = f.read()
    for sym in ("lz4mi_frames_index", "lz4mi_frames_decompress", "lz4mi_host_frames_index"):
        assert sym in lz4mi.EXPORTS and hasattr(lz4mi.lib(), sym) and f" {sym}(" in header
    assert (lz4mi.VERIFY_CONTENT, lz4mi.FRAMES_MEASURE) == (0x400, 0x800)
    for name in ("CAP_BLOCKS", "PAST_END", "EMPTY", "UNSIZED_EXACT", "MEASURE", "SIZE_MISMATCH", "OUT_CAP", "LAYOUT",
                 "DEPENDENT", "HASH_4G"):
        assert f"#define LZ4MI_FRAMES_DECLINE_{name} {getattr(C, name)}" in header
        assert getattr(lz4mi, "DECLINE_" + name) == getattr(C, name)


def test_tiny_frames_counts():
    for n in (1, 63, 64, 65, 1025):
        a, off, ln = C.pack(C.tiny_frames(n))
        r = lz4mi.host_frames_index(a, off, ln, n)
        assert r["totals"].tolist() == [n, n, n, 0]
        assert r["finfo"][:, 4].tolist() == list(range(n)) and (r["blk_size"] == 1).all()
