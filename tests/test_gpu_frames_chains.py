"""LZ4MI_FRAMES_CHAINS on the device (lz4mi_frames_plan / lz4mi_frames_compress with LZ4MI_FRAMES_DEPENDENT |
LZ4MI_FRAMES_CHAINS, and frame.compress_frames_device(chains=True)) on the zoo of tests/frames_chain_common.py: the
frames against the oracle's and the host twin's, the call's footprint, more chains than CUs in one call, two calls
back to back on one stream, and the wrapper."""
import functools

import numpy as np
import pytest

import frames_chain_common as C
import lz4mi
import oracle as O
from lz4mi import frame as F
from test_gpu_frames_compress import GUARD, GUARD_BYTE, compress_dev, dev, plan_dev, slot_layout, torch_

pytestmark = pytest.mark.gpu
MARGIN = 4096      # poisoned bytes the test owns on both sides of `out`
ALL = (True, True, True)


def flags_of(combo, packed=False, chains=True):
    csum, sized, bsum = combo
    return lz4mi.frames_enc_flags(False, csum, sized, bsum, packed=packed, chains=chains)


@functools.lru_cache(maxsize=None)
def dev_arena(group, fill):
    a, off, ln = C.arena(group, fill)
    return dev(a), dev(off.astype(np.int64)), dev(ln.astype(np.int64))


def poisoned(total):
    """-> (the whole tensor, `out` = its middle `total` bytes)."""
    t = torch_()
    buf = t.full((MARGIN + total + MARGIN,), GUARD_BYTE, dtype=t.uint8, device="cuda")
    return buf, buf[MARGIN:MARGIN + total]


@pytest.mark.parametrize("group", C.GROUPS)
@pytest.mark.parametrize("fill", C.FILLS)
@pytest.mark.parametrize("packed", (False, True), ids=("slots", "packed"))
def test_device_frames_equal_the_oracles_and_the_host_twins(group, fill, packed):
    t = torch_()
    block_max, bs, names = C.GROUPS[group]
    a, off, ln = C.arena(group, fill)
    arena, d_off, d_ln = dev_arena(group, fill)
    need = C.need_blocks(group)
    for combo in C.COMBOS:
        fl = flags_of(combo, packed)
        lens = np.array([C.expected(n, bs, combo).size for n in names], dtype=np.int64)
        if packed:
            pos, caps, total = np.cumsum(lens) - lens, None, int(lens.sum())
        else:
            pos, caps, total = slot_layout(lens)
        hp = lz4mi.host_frames_plan(off, ln, block_max, need, fl)
        htotals = hp["totals"].copy()
        hfi = lz4mi.host_frames_compress(a, hp, np.full(total, GUARD_BYTE, dtype=np.uint8), fl,
                                         slots=None if packed else (pos, caps)).copy()
        L = plan_dev(d_off, d_ln, block_max, need, fl)
        totals = L.finfo()[1]
        assert totals.tolist() == htotals.tolist() and totals[1] == need
        work = t.full((int(totals[3]),), GUARD_BYTE, dtype=t.uint8, device="cuda")
        buf, out = poisoned(total)
        fi = compress_dev(arena, L, need, work, out, total, fl, None if packed else (dev(pos), dev(caps)))
        got = buf.cpu().numpy()
        image = np.full(got.size, GUARD_BYTE, dtype=np.uint8)
        assert not fi[:, 7].any() and not hfi[:, 7].any(), (combo, fi[:, 7].tolist())
        for k, name in enumerate(names):
            want = C.expected(name, bs, combo)
            assert fi[k, 3] == want.size == hfi[k, 3] and fi[k, 5] == pos[k], (combo, name, fi[k].tolist())
            assert fi[k].tolist() == hfi[k].tolist(), (combo, name)
            image[MARGIN + int(pos[k]):MARGIN + int(pos[k]) + want.size] = want
        bad = np.nonzero(got != image)[0]
        assert not bad.size, (combo, int(bad[0]) - MARGIN, np.searchsorted(pos, bad[0] - MARGIN, side="right") - 1)
    assert (arena.cpu().numpy() == a).all()


@pytest.mark.parametrize("fill", C.FILLS)
@pytest.mark.parametrize("how", ("out_cap", "cap_blocks"))
def test_footprint_with_declined_chains(fill, how):
    """Slot mode, `out` and the bytes around it poisoned: only out[finfo[f][5] .. +finfo[f][3]) of the written frames
    changes. out_cap: two chains and a single-block frame get a slot one byte short; cap_blocks: the call is given
    one block fewer than the plan listed, so the last frame -- a chain -- does not fit nblocks."""
    t = torch_()
    block_max, bs, names = C.GROUPS["c64k"]
    fl = flags_of(ALL)
    a, off, ln = C.arena("c64k", fill)
    arena, d_off, d_ln = dev_arena("c64k", fill)
    need = C.need_blocks("c64k")
    lens = np.array([C.expected(n, bs, ALL).size for n in names], dtype=np.int64)
    short = {names.index("rep2"), names.index("r65535x3"), names.index("text300")} if how == "out_cap" else set()
    cut = {len(names) - 1} if how == "cap_blocks" else set()
    assert len(C.SHAPES[names[-1]]) > 1
    L = plan_dev(d_off, d_ln, block_max, need, fl)
    finfo, totals = L.finfo()
    assert not finfo[:, 7].any()
    lists = [x.clone() for x in (L.off, L.len, L.frame, L.woff)]
    work = t.full((int(totals[3]),), GUARD_BYTE, dtype=t.uint8, device="cuda")
    offs, caps, total = slot_layout(lens, short)
    buf, out = poisoned(total)
    fi = compress_dev(arena, L, need - len(cut), work, out, total, fl, (dev(offs), dev(caps)))
    image = np.full(buf.numel(), GUARD_BYTE, dtype=np.uint8)
    for k, name in enumerate(names):
        if k in short:
            assert fi[k, 7] == C.OUT_CAP and fi[k, 3] == lens[k], name
        elif k in cut:
            assert fi[k, 7] == C.CAP_BLOCKS, name
        else:
            assert fi[k, 7] == 0 and fi[k, 5] == offs[k] and fi[k, 3] == lens[k], name
            image[MARGIN + offs[k]:MARGIN + offs[k] + lens[k]] = C.expected(name, bs, ALL)
    got = buf.cpu().numpy()
    bad = np.nonzero(got != image)[0]
    assert not bad.size, (int(bad[0]) - MARGIN, np.searchsorted(offs, bad[0] - MARGIN, side="right") - 1)
    assert (arena.cpu().numpy() == a).all()
    for before, after in zip(lists, (L.off, L.len, L.frame, L.woff)):
        assert t.equal(before, after)


@functools.lru_cache(maxsize=None)
def many_chains():
    """700 two-block sources of text and repetitive in turn, 65536 + k bytes for k = 1 .. 700, back to back."""
    lens = [65536 + k for k in range(1, 701)]
    offs = np.cumsum([0] + lens[:-1])
    text, rep = O.generate("text", 31, sum(lens)), O.generate("repetitive", 2, sum(lens))
    src = np.empty(sum(lens), dtype=np.uint8)
    for k, (o, n) in enumerate(zip(offs, lens)):
        src[o:o + n] = (text if k % 2 == 0 else rep)[o:o + n]
    return src, offs, lens


def test_700_chains_in_one_call():
    """More than two workgroups per CU: each re-initialises its table and rings. Against the host twin, which
    tests/test_frames_chains_cpu.py pins to the oracle."""
    t = torch_()
    src, offs, lens = many_chains()
    nf = len(lens)
    fl = flags_of((True, True, False), True)
    hp = lz4mi.host_frames_plan(offs, lens, 65536, 2 * nf, fl)
    assert hp["totals"][:2].tolist() == [2 * nf, 2 * nf] and not hp["finfo"][:, 7].any()
    hout = np.full(int(hp["totals"][2]), GUARD_BYTE, dtype=np.uint8)
    hfi = lz4mi.host_frames_compress(src, hp, hout, fl)
    assert not hfi[:, 7].any()
    # (not hollow: a few frames against the oracle here too, and the second block reaches into the first)
    for k in (0, 1, 350, 699):
        want = O.compress_frame(src[offs[k]:offs[k] + lens[k]], None, 65536, False, True, True)
        assert np.array_equal(hout[hfi[k, 5]:hfi[k, 5] + hfi[k, 3]], want), k
    arena = dev(src)
    L = plan_dev(dev(offs.astype(np.int64)), dev(np.array(lens, dtype=np.int64)), 65536, 2 * nf, fl)
    totals = L.finfo()[1]
    assert totals.tolist() == hp["totals"].tolist()
    work = t.empty(int(totals[3]), dtype=t.uint8, device="cuda")
    total = int(hfi[:, 3].sum())
    out = t.full((total + GUARD,), GUARD_BYTE, dtype=t.uint8, device="cuda")
    fi = compress_dev(arena, L, 2 * nf, work, out, total, fl)
    assert fi.tolist() == hfi.tolist()
    got = out.cpu().numpy()
    bad = np.nonzero(got[:total] != hout[:total])[0]
    assert not bad.size, (int(bad[0]), int(np.searchsorted(hfi[:, 5], bad[0], side="right") - 1))
    assert (got[total:] == GUARD_BYTE).all()


def test_two_calls_back_to_back_on_one_stream():
    t = torch_()
    combo = (True, True, False)
    fl = flags_of(combo, True)
    runs = []
    for group, fill in (("c64k", 0), ("c256k", 0xFF)):
        block_max, bs, names = C.GROUPS[group]
        arena, d_off, d_ln = dev_arena(group, fill)
        L = plan_dev(d_off, d_ln, block_max, C.need_blocks(group), fl)
        totals = L.finfo()[1]
        work = t.empty(int(totals[3]), dtype=t.uint8, device="cuda")
        out = t.full((int(totals[2]),), GUARD_BYTE, dtype=t.uint8, device="cuda")
        runs.append((group, arena, L, int(totals[1]), work, out))
    for group, arena, L, nb, work, out in runs:          # both enqueued before anything is read back
        lz4mi.frames_compress_dev(arena.data_ptr(), L.off.data_ptr(), L.len.data_ptr(), L.frame.data_ptr(),
                                  L.woff.data_ptr(), nb, L.finfo_ptr(), L.nf, work.data_ptr(), work.numel(),
                                  out.data_ptr(), out.numel(), None, None, flags=fl)
    for group, arena, L, nb, work, out in runs:
        _, bs, names = C.GROUPS[group]
        fi, got, at = L.finfo()[0], out.cpu().numpy(), 0
        assert not fi[:, 7].any()
        for k, name in enumerate(names):
            want = C.expected(name, bs, combo)
            assert fi[k, 5] == at and fi[k, 3] == want.size and np.array_equal(got[at:at + want.size], want), (group, name)
            at += want.size
        assert (got[at:] == GUARD_BYTE).all()


def test_wrapper_keeps_chains_in_the_batch():
    t = torch_()
    block_max, bs, names = C.GROUPS["c64k"]
    bufs = [dev(C.content(n)) if C.content(n).size else t.zeros(0, dtype=t.uint8, device="cuda") for n in names]
    for combo in ((True, True, False), (False, False, True)):
        csum, sized, bsum = combo
        rep = {}
        res = F.compress_frames_device(bufs, block_size=65536, independent=False, content_checksum=csum,
                                       add_content_size=sized, block_checksum=bsum, chains=True, report=rep)
        assert rep["routes"] == ["batch"] * len(names) and rep["declined"] == [0] * len(names)
        for k, name in enumerate(names):
            assert np.array_equal(res[k].cpu().numpy(), C.expected(name, bs, combo)), (combo, name)
    k = names.index("text4")
    back = F.decompress_frame_device(res[k], linked=True)
    assert np.array_equal(back.cpu().numpy(), C.content("text4"))
    # the default stays the per-frame chain
    rep = {}
    res = F.compress_frames_device(bufs[:3], block_size=65536, independent=False, report=rep)
    assert rep["routes"] == ["chain", "batch", "chain"] and rep["declined"] == [C.DEPENDENT, 0, C.DEPENDENT]
    assert np.array_equal(res[0].cpu().numpy(), C.expected("text4", bs, (False, True, False)))
