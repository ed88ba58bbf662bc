"""lz4mi_host_frames_plan / lz4mi_host_frames_compress -- the host checkers of the frame batch encoder's device
passes (include/lz4mi.h) -- against a closed-form plan and the oracle's frames, on the zoo of
tests/frames_enc_common.py. No GPU needed."""
import numpy as np
import pytest

import frames_enc_common as C
import lz4mi
import oracle as O
from lz4mi import frame as F
from lz4mi import shard

GUARD = 0xA5


def flags_of(combo, packed=False):
    return lz4mi.frames_enc_flags(*combo, packed=packed)


def need_blocks(group):
    _, bs, names = C.GROUPS[group]
    return sum(len(C.SHAPES[n]) for n in names)


def plan(group, fill, combo, cap=None, packed=False):
    a, off, ln = C.arena(group, fill)
    cap = need_blocks(group) if cap is None else cap
    return lz4mi.host_frames_plan(off, ln, C.GROUPS[group][0], cap, flags_of(combo, packed)), a, off, ln


def compress_packed(group, fill, combo):
    p, a, off, ln = plan(group, fill, combo, packed=True)
    out = np.full(int(p["totals"][2]) + 64, GUARD, dtype=np.uint8)
    fi = lz4mi.host_frames_compress(a, p, out[:int(p["totals"][2])], flags_of(combo, True))
    return fi, out, p


def test_zoo_shapes():
    C.shapes()


@pytest.mark.parametrize("group", C.GROUPS)
@pytest.mark.parametrize("combo", C.COMBOS, ids=C.combo_id)
def test_plan_is_the_closed_form(group, combo):
    _, bs, names = C.GROUPS[group]
    need = need_blocks(group)
    for cap in (need, need - 1, need + 3):
        p, a, off, ln = plan(group, 0, combo, cap)
        rows, totals, in_off, blen, bframe, woff = C.closed_form_plan(ln.tolist(), off.tolist(), bs, combo, cap)
        assert p["finfo"].tolist() == rows, cap
        assert p["totals"].tolist() == totals, cap
        n = totals[1]
        for key, want in (("blk_in_off", in_off), ("blk_len", blen), ("blk_frame", bframe), ("blk_work_off", woff)):
            assert p[key][:n].tolist() == want and not p[key][n:].any(), (key, cap)
    if combo[0]:
        p, *_ = plan(group, 0, combo, need - 1)
        assert p["totals"][0] == need and p["totals"][1] < need and (p["finfo"][:, 7] == C.CAP_BLOCKS).sum() == 1


def test_block_max_resolves_like_get_block_id():
    for bm, want in ((0, 65536), (1, 65536), (65536, 65536), (65537, 262144), (262144, 262144), (262145, 1048576),
                     (1048576, 1048576), (1048577, 4194304), (4194304, 4194304), (1 << 31, 4194304)):
        p = lz4mi.host_frames_plan([0], [want + 1], bm, 4)
        assert p["blk_len"][:2].tolist() == [want, 1] and p["totals"][0] == 2, bm
        assert (p["finfo"][0, 1] >> 12) & 7 == F.block_id(bm), bm
        assert lz4mi.frame_bound(want + 1, bm) == 23 + want + 1 + 16 == p["finfo"][0, 3]


@pytest.mark.parametrize("group", C.GROUPS)
@pytest.mark.parametrize("fill", C.FILLS)
@pytest.mark.parametrize("combo", C.COMBOS, ids=C.combo_id)
def test_frames_are_the_oracles(group, fill, combo):
    _, bs, names = C.GROUPS[group]
    fi, out, p = compress_packed(group, fill, combo)
    at = 0
    for k, name in enumerate(names):
        want = C.expected(name, bs, combo)
        if want is None:
            assert fi[k, 7] == C.DEPENDENT and len(C.SHAPES[name]) > 1, name
            continue
        assert fi[k, 7] == 0 and fi[k, 3] == want.size and fi[k, 5] == at, (name, fi[k].tolist())
        assert np.array_equal(out[at:at + want.size], want), name
        assert want.size <= lz4mi.frame_bound(C.content(name).size, bs), name
        at += want.size
    assert (out[at:] == GUARD).all()
    assert at <= p["totals"][2]
    # not hollow: dependent combos decline the multi-block contents and only those
    if not combo[0]:
        assert sum(1 for n in names if len(C.SHAPES[n]) > 1) == (fi[:, 7] == C.DEPENDENT).sum() > 0


def test_block_checksum_frames_verify():
    _, bs, names = C.GROUPS["b64k"]
    combo = (True, True, True, True)
    fi, out, p = compress_packed("b64k", 0, combo)
    for k, name in enumerate(names):
        f = out[fi[k, 5]:fi[k, 5] + fi[k, 3]]
        info, blocks = shard.frame_blocks(f)
        assert info["flg"] & 0x10 and tuple(st for _, _, st in blocks) == C.SHAPES[name]
        if blocks:
            st = lz4mi.host_verify_blocks(f, [q for q, _, _ in blocks], [n for _, n, _ in blocks])
            assert not st.any(), name
        assert np.array_equal(f, C.expected(name, bs, combo)), name
        ost, back = O.decompress_frame(f)
        assert ost == 0 and np.array_equal(back, C.content(name)), name


def test_frame_bound():
    assert lz4mi.frame_bound(0) == lz4mi.frame_bound(0, 65536) == 23
    p = lz4mi.host_frames_plan([0], [0], 65536, 0, flags_of((True, True, True, False), True))
    out = np.full(64, GUARD, dtype=np.uint8)
    fi = lz4mi.host_frames_compress(np.zeros(1, np.uint8), p, out[:23], flags_of((True, True, True, False), True))
    assert fi[0].tolist() == [0, 0x6C | 0x40 << 8, 0, 23, 0, 0, 0, 0]
    assert np.array_equal(out[:23], O.compress_frame(np.zeros(0, np.uint8), None, 65536, True, True, True))
    assert (out[23:] == GUARD).all()


@pytest.mark.parametrize("packed", (False, True))
def test_out_cap_one_byte_short_writes_nothing(packed):
    _, bs, names = C.GROUPS["b64k"]
    combo = (True, True, True, False)
    ref, _, _ = compress_packed("b64k", 0, combo)
    lens = ref[:, 3].copy()
    p, a, off, ln = plan("b64k", 0, combo, packed=packed)
    short = names.index("text4000")
    if packed:
        # out_total one byte short of the last frame: it is declined and takes no room, every frame before it stays
        total = int(lens.sum())
        out = np.full(total + 64, GUARD, dtype=np.uint8)
        fi = lz4mi.host_frames_compress(a, p, out[:total - 1], flags_of(combo, True))
        assert fi[:-1, 7].tolist() == [0] * (len(names) - 1) and fi[-1, 7] == C.OUT_CAP
        assert (fi[:-1, 5] == np.cumsum(lens)[:-1] - lens[:-1]).all()
        assert (out[total - int(lens[-1]):] == GUARD).all()
        return
    caps = lens.copy()
    caps[short] -= 1
    offs = np.cumsum(caps + 48) - caps
    out = np.full(int(offs[-1] + caps[-1]) + 64, GUARD, dtype=np.uint8)
    fi = lz4mi.host_frames_compress(a, p, out, flags_of(combo), slots=(offs, caps))
    for k, name in enumerate(names):
        lo, hi = int(offs[k]), int(offs[k] + caps[k])
        if k == short:
            assert fi[k, 7] == C.OUT_CAP and (out[lo - 48:hi + 48] == GUARD).all()
        else:
            assert fi[k, 7] == 0 and fi[k, 5] == lo and np.array_equal(out[lo:hi], C.expected(name, bs, combo)), name
            assert (out[hi:hi + 48] == GUARD).all()


def test_packed_positions_are_the_running_sum():
    fi, out, p = compress_packed("b64k", 0xFF, (True, False, False, True))
    assert not fi[:, 7].any()
    assert fi[:, 5].tolist() == (np.cumsum(fi[:, 3]) - fi[:, 3]).tolist()


def test_flag_and_null_checks_need_no_device():
    L = lz4mi.lib()
    a, off, ln = C.arena("b64k", 0)
    n = off.size
    fi, tot = np.zeros(8 * n, dtype=np.int64), np.zeros(4, dtype=np.int64)
    lists = [np.zeros(32, dtype=np.uint64), np.zeros(32, dtype=np.uint32), np.zeros(32, dtype=np.uint32),
             np.zeros(32, dtype=np.uint64)]
    lp = [x.ctypes.data for x in lists]
    args = [off.ctypes.data, ln.ctypes.data, n, 65536, *lp, 32, fi.ctypes.data, tot.ctypes.data]
    D = lz4mi.DEVICE_PTRS
    assert L.lz4mi_host_frames_plan(*args, 0) == 0
    for bad in (D, lz4mi.VERIFY_CONTENT, lz4mi.FRAMES_MEASURE, lz4mi.JS_EXACT, lz4mi.LINKED):
        assert L.lz4mi_host_frames_plan(*args, bad) == lz4mi.ERR_ARG, bad
        assert L.lz4mi_frames_plan(*args, D | bad, None) == lz4mi.ERR_ARG if bad != D else True
    assert L.lz4mi_frames_plan(*args, 0, None) == lz4mi.ERR_ARG                 # device pointers are required
    for k in (0, 1, 4, 5, 6, 7, 9, 10):
        nulled = args[:k] + [None] + args[k + 1:]
        assert L.lz4mi_host_frames_plan(*nulled, 0) == lz4mi.ERR_ARG, k
        assert L.lz4mi_frames_plan(*nulled, D, None) == lz4mi.ERR_ARG, k
    nb = int(tot[1])
    work, out = np.zeros(int(tot[3]), dtype=np.uint8), np.zeros(int(tot[2]), dtype=np.uint8)
    slots = [np.zeros(n, dtype=np.uint64), np.full(n, 1 << 20, dtype=np.uint64)]
    cargs = [a.ctypes.data, *lp, nb, fi.ctypes.data, n, work.ctypes.data, work.size, out.ctypes.data, out.size,
             slots[0].ctypes.data, slots[1].ctypes.data]
    P = lz4mi.FRAMES_PACKED
    for bad in (D, lz4mi.VERIFY_CONTENT, lz4mi.FRAMES_MEASURE, lz4mi.JS_EXACT):
        assert L.lz4mi_host_frames_compress(*cargs, bad) == lz4mi.ERR_ARG, bad
        assert L.lz4mi_frames_compress(*cargs, D | bad, None) == lz4mi.ERR_ARG if bad != D else True
    assert L.lz4mi_frames_compress(*cargs, P, None) == lz4mi.ERR_ARG
    for k in (0, 1, 2, 3, 4, 6, 8, 10):
        nulled = cargs[:k] + [None] + cargs[k + 1:]
        assert L.lz4mi_host_frames_compress(*nulled, P) == lz4mi.ERR_ARG, k
        assert L.lz4mi_frames_compress(*nulled, D | P, None) == lz4mi.ERR_ARG, k
    for k in (12, 13):   # the slot arrays: required without LZ4MI_FRAMES_PACKED only
        nulled = cargs[:k] + [None] + cargs[k + 1:]
        assert L.lz4mi_host_frames_compress(*nulled, 0) == lz4mi.ERR_ARG, k
        assert L.lz4mi_frames_compress(*nulled, D, None) == lz4mi.ERR_ARG, k
    # a work smaller than the lists need: the host twin sees it
    assert L.lz4mi_host_frames_compress(*cargs[:9], work.size - 1, *cargs[10:], P) == lz4mi.ERR_ARG
    assert L.lz4mi_host_frames_compress(*cargs[:9], 15, *cargs[10:], P) == lz4mi.ERR_ARG
    assert L.lz4mi_frames_compress(*cargs[:9], 15, *cargs[10:], D | P, None) == lz4mi.ERR_ARG
    assert L.lz4mi_host_frames_compress(*cargs, P) == 0 and not fi.reshape(n, 8)[:, 7].any()


def test_symbols_exported_and_declared():
    import os
    with open(os.path.join(os.path.dirname(lz4mi.PKG_DIR), "include", "lz4mi.h")) as f:
        header = f.read()
    for sym in ("lz4mi_frames_plan", "lz4mi_frames_compress", "lz4mi_host_frames_plan", "lz4mi_host_frames_compress",
                "lz4mi_frame_bound"):
        assert sym in lz4mi.EXPORTS and hasattr(lz4mi.lib(), sym) and f" {sym}(" in header
    for name in ("FRAMES_CONTENT_CHECKSUM", "FRAMES_NO_CONTENT_SIZE", "FRAMES_DEPENDENT", "FRAMES_PACKED"):
        v = getattr(lz4mi, name)
        assert f"#define LZ4MI_{name} 0x{v:x}u" in header and v > 0x800 and v & (v - 1) == 0
