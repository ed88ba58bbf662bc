"""The single-frame walk on the calling thread: lz4mi_host_frame_index (include/lz4mi.h) and the scan's debug
entry lz4mi_debug_frame_scan run the functions that the one lane of lz4mi_frame_index's and
lz4mi_frame_decompress's kernels runs (index_frame / scan_frame, csrc/lz4mi_frames.h). Expectation:
damaged_common.walk, the byte-wise restatement of the reference's walk, on every damaged frame of the fixture
and on every prefix of three frames of the zoo. No GPU needed."""
import ctypes
import functools
import os

import numpy as np
import pytest

import damaged_common as D
import frames_common as C
import lz4mi

P64, P32, PINFO = (1 << 64) - 7, (1 << 32) - 77, -777
U64_LISTS, U32_LISTS = ("c_in_off", "c_out_off", "s_in_off", "s_out_off"), ("c_in_len", "c_out_cap", "s_len", "c_idx", "s_idx")
# the prefixes: a content size with block checksums; no content size; a stored block behind a compressed one
PREFIX_FRAMES = ("five_bsum", "c65537_iun", "c65537_isc")


def _signed(v):
    return v - (1 << 64) if v >= 1 << 63 else v


@functools.lru_cache(maxsize=None)
def _buffers(room):
    """The poisoned lists of one call, reused by the calls with the same room: four uint64 and five uint32
    lists (the index uses the first of each), the info words, and their addresses."""
    u64, u32, info = np.empty((4, room), dtype=np.uint64), np.empty((5, room), dtype=np.uint32), np.empty(8, dtype=np.int64)
    p64, p32 = [u64[k].ctypes.data for k in range(4)], [u32[k].ctypes.data for k in range(5)]
    # lz4mi_debug_frame_scan's order: c_in_off, c_in_len, c_out_off, c_out_cap, s_in_off, s_len, s_out_off, c_idx, s_idx
    scan_args = (p64[0], p32[0], p64[1], p32[1], p64[2], p32[2], p64[3], p32[3], p32[4], info.ctypes.data)
    return u64, u32, info, scan_args


def _poison(room):
    u64, u32, info, scan_args = _buffers(room)
    u64.fill(P64)
    u32.fill(P32)
    info.fill(PINFO)
    return u64, u32, info, scan_args


def _index(f, cap, room):
    """host_frame_index on f with lists of `room` poisoned entries: (info, pay_off, size_word)."""
    u64, u32, info, _ = _poison(room)
    lz4mi.host_frame_index(f, u64[0], u32[0], cap, info)
    return info.tolist(), u64[0].tolist(), u32[0].tolist()


@functools.lru_cache(maxsize=None)
def _scan_entry():
    L = lz4mi.lib()
    L.lz4mi_debug_frame_scan.restype = ctypes.c_int
    L.lz4mi_debug_frame_scan.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32] + [ctypes.c_void_p] * 10
    return L.lz4mi_debug_frame_scan


def _scan(f, cap, room):
    """lz4mi_debug_frame_scan on f with lists of `room` poisoned entries: (info, {list name: values})."""
    u64, u32, info, scan_args = _poison(room)
    a = np.ascontiguousarray(f, dtype=np.uint8)
    src = a if a.size else np.zeros(1, dtype=np.uint8)
    assert _scan_entry()(src.__array_interface__["data"][0], a.size, cap, *scan_args) == 0
    got = dict(zip(U64_LISTS, u64.tolist()))
    got.update(zip(U32_LISTS, u32.tolist()))
    return info.tolist(), got


def _caps(nb):
    return sorted({nb, max(nb - 1, 0), min(nb, 1), 0})


def index_errors(f):
    """test_gpu_damaged_frames.test_frame_index_equals_the_reference_walk's assertions on one frame: all eight
    info words and the blocks, the four entries behind them poisoned; at a capacity below the block count
    info[:3] + [cap, 0, the position behind the first unlisted size word, info[6], 1], the first `cap`
    entries and poison behind them."""
    info, blocks = D.walk(f)
    info[2] = _signed(info[2])
    nb, bad = len(blocks), []
    room = nb + 4
    gi, gp, gw = _index(f, room, room)
    if gi != info or list(zip(gp[:nb], gw[:nb])) != blocks or gp[nb:] != [P64] * 4 or gw[nb:] != [P32] * 4:
        bad.append(("room", gi, info, gp, gw))
    for cap in _caps(nb):
        gi, gp, gw = _index(f, cap, room)
        want = info if cap == nb else info[:3] + [cap, 0, blocks[cap][0], info[6], 1]
        if gi != want or list(zip(gp[:cap], gw[:cap])) != blocks[:cap] or gp[cap:] != [P64] * (room - cap) or \
                gw[cap:] != [P32] * (room - cap):
            bad.append(("cap", cap, gi, want))
    return bad


def scan_lists(blocks, size, bmax):
    """The two lists of the reference encoder's layout for the walk's blocks, written out: a stored block takes
    its declared size and advances by it, a compressed one takes what is left of `size`, block_max at most, and
    advances by block_max."""
    want = {k: [] for k in U64_LISTS + U32_LISTS}
    pos = 0
    for k, (p, w) in enumerate(blocks):
        n = w & 0x7FFFFFFF
        if w & 0x80000000:
            for key, v in (("s_in_off", p), ("s_len", n), ("s_out_off", pos), ("s_idx", k)):
                want[key].append(v)
            pos += n
        else:
            for key, v in (("c_in_off", p), ("c_in_len", n), ("c_out_off", pos), ("c_out_cap", max(0, min(bmax, size - pos))),
                           ("c_idx", k)):
                want[key].append(v)
            pos += bmax
    return want


def scan_errors(f):
    """The scan's lists partition the walk's blocks in order, lengths without bit 31, positions and capacities
    of the layout rule; info is the index's with [3] / [4] the two counts; nothing behind the counts is written,
    at full room and at the index test's capacities."""
    info, blocks = D.walk(f)
    size, bmax = info[2], info[6]
    info[2] = _signed(info[2])
    nb, bad = len(blocks), []
    room = nb + 4
    for cap in [room] + _caps(nb):
        listed = blocks[:cap]
        want = scan_lists(listed, size, bmax)
        nc, ns = len(want["c_idx"]), len(want["s_idx"])
        assert nc + ns == len(listed) and sorted(want["c_idx"] + want["s_idx"]) == list(range(len(listed)))
        winfo = info[:3] + [nc, ns] + (info[5:] if cap >= nb else [blocks[cap][0], info[6], 1])
        gi, got = _scan(f, cap, room)
        if gi != winfo:
            bad.append(("info", cap, gi, winfo))
        for key, vals in want.items():
            poison = P64 if key in U64_LISTS else P32
            if got[key] != vals + [poison] * (room - len(vals)):
                bad.append((key, cap, got[key], vals))
    return bad


@pytest.mark.parametrize("name", D.base_names())
def test_host_frame_index_equals_the_reference_walk(name):
    """Every case of the fixture, the unspecified ones included (the walk decodes nothing)."""
    bad = [(k, c["k"], e) for k, c, f in D.cases(name, specified=False) for e in index_errors(f)]
    assert not bad, "%d cases: %r" % (len(bad), bad[:4])


@pytest.mark.parametrize("name", D.base_names())
def test_scan_partitions_the_walks_blocks(name):
    bad = [(k, c["k"], e) for k, c, f in D.cases(name, specified=False) for e in scan_errors(f)]
    assert not bad, "%d cases: %r" % (len(bad), bad[:4])


def test_prefix_frames_have_their_shapes():
    z = C.zoo()
    flg = {n: int(z[n][4]) for n in PREFIX_FRAMES}
    assert flg["five_bsum"] & 0x18 == 0x18 and not flg["c65537_iun"] & 0x08
    words = [w for _, w in D.walk(z["c65537_isc"])[1]]
    assert [w >> 31 for w in words] == [0, 1]
    assert any(w >> 31 for _, w in D.walk(z["five_bsum"])[1])


@pytest.mark.parametrize("name", PREFIX_FRAMES)
def test_every_prefix(name):
    """f[:n] for n = 0 .. len(f): every cut position of the header and of the records."""
    f = C.zoo()[name]
    bad = [(n, e) for n in range(f.size + 1) for e in index_errors(f[:n]) + scan_errors(f[:n])]
    assert not bad, "%d prefixes: %r" % (len(bad), bad[:4])


def test_scan_slots_are_the_batch_indexs_sizes():
    """One layout rule, seen from both callers: for every sized frame of the zoo that the batch index does not
    decline, the scan's slot sizes in frame order equal blk_size of lz4mi_host_frames_index without measure."""
    a, off, ln = C.arena(0)
    r = lz4mi.host_frames_index(a, off, ln, C.need_blocks())
    fi, seen = r["finfo"], 0
    for k, name in enumerate(C.NAMES):
        if fi[k, 0] or fi[k, 7] or not (fi[k, 1] & 0x08 and fi[k, 2]):
            continue
        assert not fi[k, 1] & (1 << 16), name
        first, n = int(fi[k, 4]), int(fi[k, 6])
        info, got = _scan(C.zoo()[name], n, n)
        nc, ns = info[3], info[4]
        assert nc + ns == n and info[7] == 0, name
        slots = dict(zip(got["c_idx"][:nc], got["c_out_cap"][:nc]))
        slots.update(zip(got["s_idx"][:ns], got["s_len"][:ns]))
        assert [slots[b] for b in range(n)] == r["blk_size"][first:first + n].tolist(), name
        seen += 1
    assert seen >= 30


def test_symbols_exported_and_declared():
    with open(os.path.join(os.path.dirname(lz4mi.PKG_DIR), "include", "lz4mi.h")) as f:
        header = f.read()
    assert "lz4mi_host_frame_index" in lz4mi.EXPORTS and " lz4mi_host_frame_index(" in header
    assert hasattr(lz4mi.lib(), "lz4mi_host_frame_index") and hasattr(lz4mi, "host_frame_index")
    # a debug entry, like lz4mi_debug_layout: exported by the library, not part of the header
    assert hasattr(lz4mi.lib(), "lz4mi_debug_frame_scan") and "lz4mi_debug_frame_scan" not in header
    assert "lz4mi_debug_frame_scan" not in lz4mi.EXPORTS
    L = lz4mi.lib()
    info = np.zeros(8, dtype=np.int64)
    one = np.zeros(1, dtype=np.uint8)
    assert L.lz4mi_host_frame_index(one.ctypes.data, 1, None, None, 0, None) == lz4mi.ERR_ARG
    assert L.lz4mi_host_frame_index(one.ctypes.data, 1, None, None, 1, info.ctypes.data) == lz4mi.ERR_ARG
    assert L.lz4mi_host_frame_index(None, 1, None, None, 0, info.ctypes.data) == lz4mi.ERR_ARG
    assert L.lz4mi_host_frame_index(one.ctypes.data, 1, None, None, 0, info.ctypes.data) == lz4mi.OK
    assert info.tolist() == [-5, 0, 0, 0, 0, 0, 4194304, 0]
