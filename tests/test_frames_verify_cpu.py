"""lz4mi_host_frames_verify_blocks (the checker of the device pass) on the zoo of tests/frames_verify_common.py,
without a GPU: its statuses against lz4mi_host_verify_blocks over each frame alone, the fold into finfo, the frames
that fail against decompress_frame_host, the bounds rule on hand-made lists, and the argument rules of both calls."""
import os

import numpy as np
import pytest

import frames_verify_common as C
import lz4mi
from lz4mi import frame as F
from lz4mi import shard

SLACK = 7      # list entries behind the listed blocks: nblocks = cap_blocks, not totals[1]


def indexed(fill, **kw):
    a, off, ln = C.arena(fill)
    return a, off, ln, lz4mi.host_frames_index(a, off, ln, C.need_blocks() + SLACK, **kw)


def test_zoo_shape():
    z = C.zoo()
    assert C.records() >= 130 and C.records() % 16 != 0 and len(C.NAMES) % 64 != 0, (C.records(), len(C.NAMES))
    a, off, ln = C.arena(0)
    assert [int(o) % 4 for o in off] == [k % 4 for k in range(off.size)]
    assert int(off[-1] + ln[-1]) == a.size
    for name, (f, dmg) in z.items():      # the damage is what the oracle hash sees, block by block
        if dmg is None or name == "pre_stored_past":
            continue
        blocks = shard.frame_blocks(f)[1]
        bad = {b for b, (p, n, _) in enumerate(blocks)
               if int(f[p + n:p + n + 4].view("<u4")[0]) != C.O.xxh32_std(f[p:p + n])}
        assert bad == dmg, (name, bad, dmg)


@pytest.mark.parametrize("fill", C.FILLS)
@pytest.mark.parametrize("kw", [{}, {"measure": True}, {"js_exact": True}], ids=["layout", "measure", "js_exact"])
def test_statuses_equal_the_single_frame_yardstick_and_fold(fill, kw):
    a, off, ln, index = indexed(fill, **kw)
    before = {k: v.copy() for k, v in index.items()}
    nb = index["blk_in_off"].size
    assert int(index["totals"][1]) == C.need_blocks() == nb - SLACK
    status = lz4mi.host_frames_verify_blocks(a, off, ln, index)
    want = C.yardstick(a, off, ln, before, nb)
    assert status.dtype == np.int32 and status.shape == (nb,)
    assert (status == want).all(), np.nonzero(status != want)[0][:8]
    assert set(np.unique(status).tolist()) == {0, C.ERR_BLOCK_CHECKSUM}
    # finfo: only [0], only of the frames with a failing record
    fi = index["finfo"]
    failing = set()
    for f, name in enumerate(C.NAMES):
        lo, n = int(before["finfo"][f, 4]), int(before["finfo"][f, 6])
        bad = np.flatnonzero(status[lo:lo + n]) if C.checked(before["finfo"][f], nb) else np.zeros(0, dtype=np.int64)
        assert set(bad.tolist()) == (C.zoo()[name][1] or set()), name
        if bad.size:
            failing.add(name)
    assert failing == C.expected_failing()
    want_fi = before["finfo"].copy()
    want_fi[[C.NAMES.index(n) for n in failing], 0] = C.ERR_BLOCK_CHECKSUM
    assert (fi == want_fi).all()
    assert fi[C.NAMES.index("bad_magic"), 0] == C.ERR_MAGIC
    for key in ("totals", "blk_in_off", "blk_word", "blk_frame", "blk_size"):
        assert (index[key] == before[key]).all(), key
    if kw:      # declines that leave the blocks listed do not matter: those frames are checked
        declined = [n for f, n in enumerate(C.NAMES) if before["finfo"][f, 7] and C.checked(before["finfo"][f], nb)]
        assert declined and any(n in failing for n in declined), declined


def test_failing_frames_are_those_the_host_route_refuses():
    a, off, ln, index = indexed(0)
    lz4mi.host_frames_verify_blocks(a, off, ln, index)
    for f, name in enumerate(C.NAMES):
        try:
            F.decompress_frame_host(C.zoo()[name][0], verify_blocks=True)
            st = 0
        except lz4mi.Lz4miError as e:
            st = e.status
        assert (st == C.ERR_BLOCK_CHECKSUM) == (index["finfo"][f, 0] == C.ERR_BLOCK_CHECKSUM), (name, st)
        if name in C.PRECEDENCE:
            assert st == C.ERR_BLOCK_CHECKSUM
            with pytest.raises(lz4mi.Lz4miError) as e:       # its own error, without the check
                F.decompress_frame_host(C.zoo()[name][0], verify_blocks=False)
            assert e.value.status not in (0, C.ERR_BLOCK_CHECKSUM)


def test_frames_past_nblocks_and_failed_frames_are_not_checked():
    a, off, ln, index = indexed(0)
    fi0 = index["finfo"].copy()
    # nblocks cuts the last listed frame's range: that frame is not checked, its entries are 0
    last = max(f for f in range(off.size) if C.checked(fi0[f], 10 ** 9))
    short = int(fi0[last, 4] + fi0[last, 6]) - 1
    cut = {k: (v[:short].copy() if k.startswith("blk_") else v.copy()) for k, v in index.items()}
    status = lz4mi.host_frames_verify_blocks(a, off, ln, cut)
    assert (status == C.yardstick(a, off, ln, index, short)).all() and not status[int(fi0[last, 4]):].any()
    assert cut["finfo"][last, 0] == 0
    # a frame whose [0] is set keeps it and is not checked
    k = C.NAMES.index("five_b2_mid")
    index["finfo"][k, 0] = -2
    status = lz4mi.host_frames_verify_blocks(a, off, ln, index)
    assert index["finfo"][k, 0] == -2 and not status[int(fi0[k, 4]):int(fi0[k, 4] + fi0[k, 6])].any()


@pytest.mark.parametrize("fill", C.FILLS)
def test_handmade_lists_bounds_rule(fill):
    a, off, ln, index, want, want0 = C.handmade(fill)
    index = {k: v.copy() for k, v in index.items()}
    before = index["finfo"].copy()
    status = lz4mi.host_frames_verify_blocks(a, off, ln, index)
    assert status.tolist() == want.tolist()
    assert index["finfo"][:, 0].tolist() == want0 and (index["finfo"][:, 1:] == before[:, 1:]).all()


def _args(index, a, off, ln, status):
    fi = index["finfo"]
    return [a.ctypes.data, off.ctypes.data, ln.ctypes.data, off.size, index["blk_in_off"].ctypes.data,
            index["blk_word"].ctypes.data, index["blk_frame"].ctypes.data, index["blk_in_off"].size, fi.ctypes.data,
            status.ctypes.data]


def test_argument_rules_need_no_device():
    L = lz4mi.lib()
    a, off, ln, index, _, _ = C.handmade(0)
    index = {k: v.copy() for k, v in index.items()}
    status = np.full(4, 77, dtype=np.int32)
    fi0 = index["finfo"].copy()
    args = _args(index, a, off, ln, status)
    every_flag = [1 << k for k in range(32)]
    for flag in every_flag:                               # the twin takes no flag at all
        assert L.lz4mi_host_frames_verify_blocks(*args, flag) == lz4mi.ERR_ARG, hex(flag)
    for flag in every_flag[1:]:                           # the device call LZ4MI_DEVICE_PTRS and nothing else
        assert L.lz4mi_frames_verify_blocks(*args, lz4mi.DEVICE_PTRS | flag, None) == lz4mi.ERR_ARG, hex(flag)
    assert L.lz4mi_frames_verify_blocks(*args, 0, None) == lz4mi.ERR_ARG
    assert L.lz4mi_frames_verify_blocks(*args, lz4mi.VERIFY_BLOCKS, None) == lz4mi.ERR_ARG
    calls = ((L.lz4mi_host_frames_verify_blocks, (0,)), (L.lz4mi_frames_verify_blocks, (lz4mi.DEVICE_PTRS, None)))
    for call, tail in calls:
        for k in (0, 1, 2, 4, 5, 6, 8, 9):                # every pointer NULL in turn
            assert call(*args[:k], None, *args[k + 1:], *tail) == lz4mi.ERR_ARG, k
        for w in (8, 9):                                  # finfo / blk_status is an array the call reads, or the other
            for r in (0, 1, 2, 4, 5, 6, 8, 9):
                if r != w:
                    assert call(*args[:w], args[r], *args[w + 1:], *tail) == lz4mi.ERR_ARG, (w, r)
    assert (status == 77).all() and (index["finfo"] == fi0).all()
    # nothing to do: OK on the host, and nothing is written
    z = [None] * 10
    assert L.lz4mi_host_frames_verify_blocks(*z[:3], 0, *z[4:7], 0, *z[8:], 0) == 0
    assert L.lz4mi_host_frames_verify_blocks(*args[:3], 0, *args[4:], 0) == 0
    assert L.lz4mi_host_frames_verify_blocks(*args[:7], 0, *args[8:], 0) == 0
    assert (status == 77).all() and (index["finfo"] == fi0).all()


def has_gpu():
    try:
        return lz4mi.device_count() > 0 and lz4mi.lib().lz4mi_init(0) == 0
    except Exception:
        return False


def test_device_call_without_a_device():
    L = lz4mi.lib()
    if has_gpu():
        # nothing to do: the call returns behind its checks, before it launches anything
        z = np.zeros(8, dtype=np.uint64).ctypes.data
        assert L.lz4mi_frames_verify_blocks(z + 8, z, z, 0, z, z, z, 0, z + 16, z + 24, lz4mi.DEVICE_PTRS, None) == 0
        return
    a, off, ln, index, _, _ = C.handmade(0)
    index = {k: v.copy() for k, v in index.items()}
    status = np.full(4, 77, dtype=np.int32)
    args = _args(index, a, off, ln, status)
    assert L.lz4mi_frames_verify_blocks(*args, lz4mi.DEVICE_PTRS, None) == lz4mi.ERR_NO_DEVICE
    assert L.lz4mi_frames_verify_blocks(*args[:9], None, lz4mi.DEVICE_PTRS, None) == lz4mi.ERR_ARG   # checked first
    assert (status == 77).all()


def test_symbols_exported_and_declared():
    with open(os.path.join(os.path.dirname(lz4mi.PKG_DIR), "include", "lz4mi.h")) as f:
        header = f.read()
    for sym in ("lz4mi_frames_verify_blocks", "lz4mi_host_frames_verify_blocks"):
        assert sym in lz4mi.EXPORTS and hasattr(lz4mi.lib(), sym) and f" {sym}(" in header
    assert callable(lz4mi.frames_verify_blocks_dev) and callable(lz4mi.host_frames_verify_blocks)
    import inspect
    assert inspect.signature(F.decompress_frames_device).parameters["verify_blocks"].default is False
