"""A batch of buffers compressed into frames on the device in one call (lz4mi_frames_plan / lz4mi_frames_compress
and frame.compress_frames_device) on the zoo of tests/frames_enc_common.py: the device plan against the host plan,
the frames against the host twin and the oracle, the calls' footprint, the encoder's slice boundary, the round
trip through the batch decoder and the wrapper."""
import functools

import numpy as np
import pytest

import footprint_common as FP
import frames_enc_common as C
import lz4mi
import oracle as O
from lz4mi import frame as F

pytestmark = pytest.mark.gpu
SENT = 16          # sentinel entries behind every list and around finfo / totals
GUARD = 48         # filler bytes between two frames' slots in `out`
GUARD_BYTE = 0xA5
D_COMBOS = ((True, False, True, False), (True, True, False, True), (False, True, True, False))


def torch_():
    import torch
    return torch


def dev(a):
    return torch_().from_numpy(np.array(a)).cuda()


def flags_of(combo, packed=False):
    return lz4mi.frames_enc_flags(*combo, packed=packed)


def need_blocks(group):
    return sum(len(C.SHAPES[n]) for n in C.GROUPS[group][2])


@functools.lru_cache(maxsize=None)
def dev_arena(group, fill):
    a, off, ln = C.arena(group, fill)
    return dev(a), dev(off.astype(np.int64)), dev(ln.astype(np.int64))


class Lists:
    """The plan call's outputs, SENT sentinel entries behind each list and on both sides of finfo + totals."""

    def __init__(self, nframes, cap):
        t = torch_()
        self.nf, self.cap = nframes, cap
        self.off, self.woff = (t.full((cap + SENT,), FP.FILL, dtype=t.int64, device="cuda") for _ in range(2))
        self.len, self.frame = (t.full((cap + SENT,), FP.FILL, dtype=t.int32, device="cuda") for _ in range(2))
        self.fin = t.full((SENT + 8 * nframes + 4 + SENT,), FP.FILL, dtype=t.int64, device="cuda")

    def finfo_ptr(self):
        return self.fin.data_ptr() + 8 * SENT

    def totals_ptr(self):
        return self.finfo_ptr() + 64 * self.nf

    def finfo(self):
        fin = self.fin.cpu().numpy()
        assert (fin[:SENT] == FP.FILL).all() and (fin[SENT + 8 * self.nf + 4:] == FP.FILL).all(), "finfo / totals sentinels"
        return fin[SENT:SENT + 8 * self.nf].reshape(self.nf, 8), fin[SENT + 8 * self.nf:][:4]

    def host(self):
        finfo, totals = self.finfo()
        res = {"finfo": finfo, "totals": totals}
        listed = int(totals[1])
        assert listed <= self.cap
        for key, arr in (("blk_in_off", self.off), ("blk_len", self.len), ("blk_frame", self.frame),
                         ("blk_work_off", self.woff)):
            h = arr.cpu().numpy()
            assert (h[listed:] == FP.FILL).all(), f"{key}: written behind the {listed} listed blocks"
            res[key] = h[:listed].astype(np.uint64 if arr.dtype == torch_().int64 else np.uint32)
        return res


def plan_dev(d_off, d_ln, block_max, cap, flags):
    L = Lists(d_off.numel(), cap)
    lz4mi.frames_plan_dev(d_off.data_ptr(), d_ln.data_ptr(), d_off.numel(), block_max, L.off.data_ptr(),
                          L.len.data_ptr(), L.frame.data_ptr(), L.woff.data_ptr(), cap, L.finfo_ptr(), L.totals_ptr(),
                          flags=flags)
    return L


def compress_dev(arena, L, nblocks, work, out, out_total, flags, slots=None):
    lz4mi.frames_compress_dev(arena.data_ptr(), L.off.data_ptr(), L.len.data_ptr(), L.frame.data_ptr(),
                              L.woff.data_ptr(), nblocks, L.finfo_ptr(), L.nf, work.data_ptr(), work.numel(),
                              out.data_ptr(), out_total, None if slots is None else slots[0].data_ptr(),
                              None if slots is None else slots[1].data_ptr(), flags=flags)
    return L.finfo()[0]


@pytest.mark.parametrize("group", C.GROUPS)
@pytest.mark.parametrize("combo", D_COMBOS, ids=C.combo_id)
def test_device_plan_equals_host_plan(group, combo):
    a, off, ln = C.arena(group, 0)
    arena, d_off, d_ln = dev_arena(group, 0)
    need = need_blocks(group)
    for cap in (need, need - 1, need + 5):
        got = plan_dev(d_off, d_ln, C.GROUPS[group][0], cap, flags_of(combo)).host()
        want = lz4mi.host_frames_plan(off, ln, C.GROUPS[group][0], cap, flags_of(combo))
        listed = int(want["totals"][1])
        assert got["totals"].tolist() == want["totals"].tolist(), cap
        assert got["finfo"].tolist() == want["finfo"].tolist(), cap
        for key in ("blk_in_off", "blk_len", "blk_frame", "blk_work_off"):
            assert (got[key] == want[key][:listed]).all(), (key, cap)


def test_device_plan_many_frames_crosses_the_scan_groups():
    """More frames than two passes of the carried scan (1024 frames each), lengths 0 to 4 blocks."""
    lens = [(k * 37) % 200000 for k in range(2500)]
    offs = np.cumsum([0] + lens[:-1])
    need = sum(-(-n // 65536) for n in lens)
    for cap in (need, need - 1):
        got = plan_dev(dev(offs.astype(np.int64)), dev(np.array(lens, dtype=np.int64)), 65536, cap, 0).host()
        want = lz4mi.host_frames_plan(offs, lens, 65536, cap, 0)
        assert got["totals"].tolist() == want["totals"].tolist() and got["finfo"].tolist() == want["finfo"].tolist()
        for key in ("blk_in_off", "blk_len", "blk_frame", "blk_work_off"):
            assert (got[key] == want[key][:int(want["totals"][1])]).all(), key


def slot_layout(lens, short=()):
    """Slots with GUARD bytes between them at start residues 1, 2, 3, 0 (mod 4): -> (offsets, capacities, total)."""
    caps = [int(n) - (1 if k in short else 0) for k, n in enumerate(lens)]
    offs, at = [], GUARD
    for k, c in enumerate(caps):
        at += ((k + 1) % 4 - at) % 4
        offs.append(at)
        at += c + GUARD
    return np.array(offs, dtype=np.int64), np.array(caps, dtype=np.int64), at


@pytest.mark.parametrize("group", C.GROUPS)
@pytest.mark.parametrize("fill", C.FILLS)
@pytest.mark.parametrize("packed", (False, True), ids=("slots", "packed"))
def test_device_frames_equal_the_host_twins_and_the_oracles(group, fill, packed):
    t = torch_()
    block_max, bs, names = C.GROUPS[group]
    a, off, ln = C.arena(group, fill)
    arena, d_off, d_ln = dev_arena(group, fill)
    need = need_blocks(group)
    for combo in C.COMBOS:
        fl = flags_of(combo, packed)
        hp = lz4mi.host_frames_plan(off, ln, block_max, need, fl)
        hout = np.full(int(hp["totals"][2]), GUARD_BYTE, dtype=np.uint8)
        hfi = lz4mi.host_frames_compress(a, hp, hout, flags_of(combo, True)).copy()
        L = plan_dev(d_off, d_ln, block_max, need, fl)
        totals = L.finfo()[1]
        work = t.full((int(totals[3]),), GUARD_BYTE, dtype=t.uint8, device="cuda")
        if packed:
            total = int(hfi[hfi[:, 7] == 0, 3].sum())
            out = t.full((total + GUARD,), GUARD_BYTE, dtype=t.uint8, device="cuda")
            fi = compress_dev(arena, L, int(totals[1]), work, out, total, fl)
            pos = hfi[:, 5]
        else:
            offs, caps, total = slot_layout(hfi[:, 3])
            out = t.full((total,), GUARD_BYTE, dtype=t.uint8, device="cuda")
            fi = compress_dev(arena, L, int(totals[1]), work, out, total, fl, (dev(offs), dev(caps)))
            pos = offs
        got = out.cpu().numpy()
        image = np.full(got.size, GUARD_BYTE, dtype=np.uint8)
        for k, name in enumerate(names):
            want = C.expected(name, bs, combo)
            if want is None:
                assert fi[k, 7] == hfi[k, 7] == C.DEPENDENT, (combo, name)
                continue
            assert fi[k, 7] == 0 and fi[k, 3] == want.size == hfi[k, 3] and fi[k, 5] == pos[k], (combo, name, fi[k].tolist())
            assert np.array_equal(hout[hfi[k, 5]:hfi[k, 5] + hfi[k, 3]], want), (combo, name)
            image[int(pos[k]):int(pos[k]) + want.size] = want
        bad = np.nonzero(got != image)[0]
        assert not bad.size, (combo, int(bad[0]), np.searchsorted(pos, bad[0], side="right") - 1)
    assert (arena.cpu().numpy() == a).all()


@pytest.mark.parametrize("packed", (False, True), ids=("slots", "packed"))
def test_out_cap_one_byte_short_writes_nothing(packed):
    t = torch_()
    block_max, bs, names = C.GROUPS["b64k"]
    combo = (True, True, True, True)
    fl = flags_of(combo, packed)
    a, off, ln = C.arena("b64k", 0xFF)
    arena, d_off, d_ln = dev_arena("b64k", 0xFF)
    lens = np.array([C.expected(n, bs, combo).size for n in names], dtype=np.int64)
    L = plan_dev(d_off, d_ln, block_max, need_blocks("b64k"), fl)
    totals = L.finfo()[1]
    work = t.empty(int(totals[3]), dtype=t.uint8, device="cuda")
    if packed:
        # out_total one byte short of the last frame: it is declined, every frame before it is written
        total = int(lens.sum())
        out = t.full((total + GUARD,), GUARD_BYTE, dtype=t.uint8, device="cuda")
        fi = compress_dev(arena, L, int(totals[1]), work, out, total - 1, fl)
        got = out.cpu().numpy()
        assert fi[:-1, 7].tolist() == [0] * (len(names) - 1) and fi[-1, 7] == C.OUT_CAP
        at = 0
        for k, name in enumerate(names[:-1]):
            assert fi[k, 5] == at and np.array_equal(got[at:at + lens[k]], C.expected(name, bs, combo)), name
            at += int(lens[k])
        assert (got[at:] == GUARD_BYTE).all()
        # one byte short of a frame in the middle: it takes no room, the frames behind it move up while they
        # fit -- the host twin's positions and bytes
        k = names.index("rand64k")
        short_total = int(lens[:k + 1].sum()) - 1
        hp = lz4mi.host_frames_plan(off, ln, block_max, need_blocks("b64k"), fl)
        hout = np.full(total + GUARD, GUARD_BYTE, dtype=np.uint8)
        hfi = lz4mi.host_frames_compress(a, hp, hout[:short_total], fl)
        assert hfi[k, 7] == C.OUT_CAP and hfi[k + 1, 7] == 0 and hfi[k + 1, 5] == hfi[k - 1, 5] + hfi[k - 1, 3]
        assert C.OUT_CAP in hfi[k + 2:, 7].tolist()
        L = plan_dev(d_off, d_ln, block_max, need_blocks("b64k"), fl)
        out.fill_(GUARD_BYTE)
        fi = compress_dev(arena, L, int(totals[1]), work, out, short_total, fl)
        assert fi.tolist() == hfi.tolist()
        assert np.array_equal(out.cpu().numpy(), hout)
        return
    short = {names.index("text4000"), names.index("tiles65537")}
    offs, caps, total = slot_layout(lens, short)
    out = t.full((total,), GUARD_BYTE, dtype=t.uint8, device="cuda")
    fi = compress_dev(arena, L, int(totals[1]), work, out, total, fl, (dev(offs), dev(caps)))
    got = out.cpu().numpy()
    image = np.full(total, GUARD_BYTE, dtype=np.uint8)
    for k, name in enumerate(names):
        if k in short:
            assert fi[k, 7] == C.OUT_CAP and fi[k, 3] == lens[k], name
        else:
            assert fi[k, 7] == 0 and fi[k, 5] == offs[k], name
            image[offs[k]:offs[k] + lens[k]] = C.expected(name, bs, combo)
    assert np.array_equal(got, image)
    assert (arena.cpu().numpy() == a).all()


def test_slot_longer_than_the_frame_keeps_its_rest():
    t = torch_()
    block_max, bs, names = C.GROUPS["b64k"]
    combo = (True, True, True, False)
    arena, d_off, d_ln = dev_arena("b64k", 0)
    lens = np.array([C.expected(n, bs, combo).size for n in names], dtype=np.int64)
    L = plan_dev(d_off, d_ln, block_max, need_blocks("b64k"), flags_of(combo))
    finfo, totals = L.finfo()
    bounds = finfo[:, 3].copy()
    assert (bounds >= lens).all() and bounds.tolist() == [lz4mi.frame_bound(C.content(n).size, bs) for n in names]
    offs, caps, total = slot_layout(bounds)
    out = t.full((total,), GUARD_BYTE, dtype=t.uint8, device="cuda")
    work = t.empty(int(totals[3]), dtype=t.uint8, device="cuda")
    fi = compress_dev(arena, L, int(totals[1]), work, out, total, flags_of(combo), (dev(offs), dev(caps)))
    image = np.full(total, GUARD_BYTE, dtype=np.uint8)
    for k, name in enumerate(names):
        image[offs[k]:offs[k] + lens[k]] = C.expected(name, bs, combo)
    assert not fi[:, 7].any() and fi[:, 3].tolist() == lens.tolist()
    assert np.array_equal(out.cpu().numpy(), image)


def test_work_too_small_declines_on_the_device():
    """The lists are the device's: a frame whose slots do not lie inside `work` is declined there, nothing is written
    for it, and the frames before it are."""
    t = torch_()
    block_max, bs, names = C.GROUPS["b64k"]
    combo = (True, False, True, False)
    fl = flags_of(combo, True)
    arena, d_off, d_ln = dev_arena("b64k", 0)
    L = plan_dev(d_off, d_ln, block_max, need_blocks("b64k"), fl)
    totals = L.finfo()[1]
    work = t.empty(int(totals[3]), dtype=t.uint8, device="cuda")
    out = t.full((int(totals[2]),), GUARD_BYTE, dtype=t.uint8, device="cuda")
    fi = compress_dev(arena, L, int(totals[1]), work, out, out.numel(), fl)
    assert not fi[:, 7].any()
    L = plan_dev(d_off, d_ln, block_max, need_blocks("b64k"), fl)
    out.fill_(GUARD_BYTE)
    fi = compress_dev(arena, L, int(totals[1]), work[:int(totals[3]) - 1], out, out.numel(), fl)
    assert fi[:-1, 7].tolist() == [0] * (len(names) - 1) and fi[-1, 7] == C.CAP_BLOCKS
    got, at = out.cpu().numpy(), 0
    for k, name in enumerate(names[:-1]):
        want = C.expected(name, bs, combo)
        assert fi[k, 5] == at and np.array_equal(got[at:at + want.size], want), name
        at += want.size
    assert (got[at:] == GUARD_BYTE).all()


@functools.lru_cache(maxsize=None)
def many_text():
    """4100 text frames of 20 to 720 bytes: -> (arena, offsets, lengths, oracle frames)."""
    lens = [20 + (k * 131) % 701 for k in range(4100)]
    src = O.generate("text", 7, sum(lens) + 64)
    offs = np.cumsum([0] + lens[:-1])
    frames = [O.compress_frame(src[o:o + n], None, 65536, True, True, True) for o, n in zip(offs, lens)]
    return src, offs, lens, frames


def test_4100_text_frames_cross_the_encoder_slice():
    t = torch_()
    src, offs, lens, frames = many_text()
    nf = len(lens)
    assert nf > 4096 and sum(1 for f, n in zip(frames, lens) if f.size < 19 + n + 4 + 4) >= 3000
    fl = flags_of((True, True, True, False), True)
    arena = dev(src)
    L = plan_dev(dev(offs.astype(np.int64)), dev(np.array(lens, dtype=np.int64)), 65536, nf, fl)
    totals = L.finfo()[1]
    assert totals[:2].tolist() == [nf, nf]
    work = t.empty(int(totals[3]), dtype=t.uint8, device="cuda")
    out = t.full((int(totals[2]),), GUARD_BYTE, dtype=t.uint8, device="cuda")
    fi = compress_dev(arena, L, nf, work, out, out.numel(), fl)
    want = np.concatenate(frames)
    assert not fi[:, 7].any() and fi[:, 3].tolist() == [f.size for f in frames]
    assert fi[:, 5].tolist() == (np.cumsum(fi[:, 3]) - fi[:, 3]).tolist()
    got = out.cpu().numpy()
    bad = np.nonzero(got[:want.size] != want)[0]
    assert not bad.size, (int(bad[0]), int(np.searchsorted(fi[:, 5], bad[0], side="right") - 1))
    assert (got[want.size:] == GUARD_BYTE).all()


def test_round_trip_through_the_batch_decoder():
    t = torch_()
    block_max, bs, names = C.GROUPS["b64k"]
    fl = flags_of((True, True, True, False), True)
    arena, d_off, d_ln = dev_arena("b64k", 0xFF)
    L = plan_dev(d_off, d_ln, block_max, need_blocks("b64k"), fl)
    totals = L.finfo()[1]
    work = t.empty(int(totals[3]), dtype=t.uint8, device="cuda")
    out = t.empty(int(totals[2]), dtype=t.uint8, device="cuda")
    fi = compress_dev(arena, L, int(totals[1]), work, out, out.numel(), fl)
    assert not fi[:, 7].any()
    rep = {}
    back = F.decompress_frames_device(out, offsets=fi[:, 5].tolist(), lengths=fi[:, 3].tolist(), report=rep)
    for k, name in enumerate(names):
        assert np.array_equal(back[k].cpu().numpy(), C.content(name)), name
    # the empty frame is the decoder's own fallback, everything else its batch
    assert [r == "batch" for r in rep["routes"]] == [C.content(n).size > 0 for n in names]


def test_wrapper_completes_declined_frames():
    block_max, bs, names = C.GROUPS["b64k"]
    bufs = [dev(C.content(n)) if C.content(n).size else torch_().zeros(0, dtype=torch_().uint8, device="cuda") for n in names]
    for combo in ((False, True, True, False), (True, False, False, True), (False, False, True, True)):
        indep, csum, sized, bsum = combo
        rep = {}
        res = F.compress_frames_device(bufs, block_size=block_max, independent=indep, content_checksum=csum,
                                       add_content_size=sized, block_checksum=bsum, report=rep)
        for k, name in enumerate(names):
            multi = len(C.SHAPES[name]) > 1
            want_route = "chain" if (multi and not indep) else "batch"
            assert rep["routes"][k] == want_route and rep["declined"][k] == (C.DEPENDENT if want_route == "chain" else 0), name
            if want_route == "batch":
                want = C.expected(name, bs, combo)
            elif not bsum:
                want = O.compress_frame(C.content(name), None, bs, False, csum, sized)
            else:
                want = None
            got = res[k].cpu().numpy()
            if want is not None:
                assert np.array_equal(got, want), (combo, name)
            ost, back = O.decompress_frame(got)
            assert ost == 0 and np.array_equal(back, C.content(name)), (combo, name)
    # the offsets form, and a frame only the per-frame device path takes (the batch has no room for its blocks'
    # slots: not reachable through the wrapper, so the route is exercised directly)
    a, off, ln = C.arena("b64k", 0)
    res = F.compress_frames_device(dev(a), block_size=block_max, content_checksum=True, offsets=off.tolist(),
                                   lengths=ln.tolist())
    for k, name in enumerate(names):
        assert np.array_equal(res[k].cpu().numpy(), C.expected(name, bs, (True, True, True, False))), name
    one, route = F._frame_alone(dev(C.content("five")), bs, True, True, True, False, None)
    assert route == "codec" and np.array_equal(one.cpu().numpy(), C.expected("five", bs, (True, True, True, False)))
