"""lz4mi_frames_verify_blocks on the device, on the zoo of tests/frames_verify_common.py: its statuses and finfo
against the host twin, its footprint, the hand-made lists of the bounds rule, what lz4mi_frames_decompress does with
the verdict, the precedence of the block checksum over a frame's other errors, and
frame.decompress_frames_device(verify_blocks=True) against the single-frame call."""
import functools

import numpy as np
import pytest

import footprint_common as FP
import frames_verify_common as C
import lz4mi
from lz4mi import frame as F

pytestmark = pytest.mark.gpu
SENT = 16          # sentinel entries behind every list and blk_status and around finfo / totals
SLACK = 7          # list entries behind the listed blocks that the verify call is given too (nblocks = cap_blocks)
GUARD = 48         # filler bytes between two frames' slots in `out`
ERR_OFFSET0, ERR_CHECKSUM, ERR_RANGE = -3, -7, -8


def torch_():
    import torch
    return torch


def dev(a):
    return torch_().from_numpy(np.array(a)).cuda()


def dev_spans(off, ln):
    return dev(off.astype(np.int64)), dev(ln.astype(np.int64))


class Lists:
    """The index call's outputs and blk_status, all pre-filled with FP.FILL, SENT sentinel entries behind each list
    and on both sides of finfo + totals. The entries behind the listed blocks keep the fill: blk_frame[b] = 77 there,
    a valid frame number whose range does not hold b."""

    def __init__(self, nframes, cap):
        t = torch_()
        self.nf, self.cap = nframes, cap
        self.off = t.full((cap + SENT,), FP.FILL, dtype=t.int64, device="cuda")
        self.word, self.frame, self.size, self.status = (t.full((cap + SENT,), FP.FILL, dtype=t.int32, device="cuda")
                                                         for _ in range(4))
        self.fin = t.full((SENT + 8 * nframes + 4 + SENT,), FP.FILL, dtype=t.int64, device="cuda")

    def finfo_ptr(self):
        return self.fin.data_ptr() + 8 * SENT

    def load(self, index):
        """Hand-made lists and finfo from the host."""
        t = torch_()
        n = index["blk_in_off"].size
        self.off[:n] = t.from_numpy(index["blk_in_off"].astype(np.int64)).cuda()
        for dst, key in ((self.word, "blk_word"), (self.frame, "blk_frame"), (self.size, "blk_size")):
            dst[:n] = t.from_numpy(index[key].view(np.int32)).cuda()
        self.fin[SENT:SENT + 8 * self.nf] = t.from_numpy(index["finfo"].reshape(-1)).cuda()

    def finfo(self):
        fin = self.fin.cpu().numpy()
        assert (fin[:SENT] == FP.FILL).all() and (fin[SENT + 8 * self.nf + 4:] == FP.FILL).all(), "finfo sentinels"
        return fin[SENT:SENT + 8 * self.nf].reshape(self.nf, 8).copy(), fin[SENT + 8 * self.nf:][:4].copy()

    def lists(self):
        return [x.cpu().numpy() for x in (self.off, self.word, self.frame, self.size)]


def index_dev(arena, d_off, d_ln, cap, **kw):
    L = Lists(d_off.numel(), cap)
    lz4mi.frames_index_dev(arena.data_ptr(), d_off.data_ptr(), d_ln.data_ptr(), d_off.numel(), L.off.data_ptr(),
                           L.word.data_ptr(), L.frame.data_ptr(), L.size.data_ptr(), cap, L.finfo_ptr(),
                           L.finfo_ptr() + 64 * L.nf, **kw)
    return L


def verify_dev(arena, d_off, d_ln, L, nblocks):
    lz4mi.frames_verify_blocks_dev(arena.data_ptr(), d_off.data_ptr(), d_ln.data_ptr(), L.nf, L.off.data_ptr(),
                                   L.word.data_ptr(), L.frame.data_ptr(), nblocks, L.finfo_ptr(), L.status.data_ptr(),
                                   torch_().cuda.current_stream().cuda_stream)
    torch_().cuda.synchronize()
    st = L.status.cpu().numpy()
    FP.assert_sentinels(st, nblocks, "blk_status[]")
    return st[:nblocks]


@functools.lru_cache(maxsize=None)
def dev_arena(fill):
    a, off, ln = C.arena(fill)
    return (dev(a),) + dev_spans(off, ln)


@pytest.mark.parametrize("fill", C.FILLS)
@pytest.mark.parametrize("kw", [{}, {"measure": True}, {"js_exact": True}], ids=["layout", "measure", "js_exact"])
def test_device_call_equals_host_twin(fill, kw):
    a, off, ln = C.arena(fill)
    arena, d_off, d_ln = dev_arena(fill)
    cap = C.need_blocks() + SLACK
    L = index_dev(arena, d_off, d_ln, cap, **kw)
    lists0, (fi0, totals0) = L.lists(), L.finfo()
    host = lz4mi.host_frames_index(a, off, ln, cap, **kw)
    assert (fi0 == host["finfo"]).all() and int(totals0[1]) == C.need_blocks()
    want = lz4mi.host_frames_verify_blocks(a, off, ln, host)
    got = verify_dev(arena, d_off, d_ln, L, cap)
    assert (got == want).all(), np.nonzero(got != want)[0][:8]
    assert np.count_nonzero(want) >= len(C.expected_failing())
    fi, totals = L.finfo()
    assert (fi == host["finfo"]).all() and (totals == totals0).all()
    assert {C.NAMES[f] for f in np.flatnonzero(fi[:, 0] == C.ERR_BLOCK_CHECKSUM)} == C.expected_failing()
    for x, y in zip(L.lists(), lists0):
        assert (x == y).all(), "a list was written"
    assert (arena.cpu().numpy() == a).all() and (d_off.cpu().numpy() == off.astype(np.int64)).all()
    assert (d_ln.cpu().numpy() == ln.astype(np.int64)).all()
    # nblocks = totals[1], the other way to call it: the same statuses
    L2 = index_dev(arena, d_off, d_ln, cap, **kw)
    assert (verify_dev(arena, d_off, d_ln, L2, C.need_blocks()) == want[:C.need_blocks()]).all()
    assert (L2.finfo()[0] == fi).all()


@pytest.mark.parametrize("fill", C.FILLS)
def test_handmade_lists_bounds_rule(fill):
    a, off, ln, index, want, want0 = C.handmade(fill)
    host = {k: v.copy() for k, v in index.items()}
    assert lz4mi.host_frames_verify_blocks(a, off, ln, host).tolist() == want.tolist()
    arena = dev(a)
    d_off, d_ln = dev_spans(off, ln)
    L = Lists(3, 4)
    L.load(index)
    got = verify_dev(arena, d_off, d_ln, L, 4)
    assert got.tolist() == want.tolist()
    fi, _ = L.finfo()
    assert (fi == host["finfo"]).all() and fi[:, 0].tolist() == want0
    assert (arena.cpu().numpy() == a).all()


# ------------------------------------------------------------------- index, verify, decompress
class Run:
    pass


@functools.lru_cache(maxsize=None)
def batch(verify, chains=False, verify_content=False):
    """Index, the verify call (or not), decompress of the whole zoo into a pattern-filled `out` in which every
    frame the index accepts has a slot, GUARD bytes apart."""
    t = torch_()
    a, off, ln = C.arena(0)
    arena, d_off, d_ln = dev_arena(0)
    r = Run()
    L = index_dev(arena, d_off, d_ln, C.need_blocks())
    r.index, _ = L.finfo()
    r.live = [k for k in range(len(C.NAMES)) if not r.index[k, 0] and not r.index[k, 7]]
    r.total = {k: int(r.index[k, 3]) for k in r.live}
    r.off = dict(zip(r.live, FP.layout([r.total[k] for k in r.live], guard=GUARD)))
    size = FP.MARGIN + r.off[r.live[-1]] + r.total[r.live[-1]] + FP.MARGIN
    r.init = FP.pattern(size, 0)
    out = dev(r.init)
    foff, fcap = np.zeros(len(C.NAMES), dtype=np.int64), np.zeros(len(C.NAMES), dtype=np.int64)
    for k in r.live:
        foff[k], fcap[k] = FP.MARGIN + r.off[k], r.total[k]
    d_foff, d_fcap = dev(foff), dev(fcap)
    s = t.cuda.current_stream().cuda_stream
    if verify:
        lz4mi.frames_verify_blocks_dev(arena.data_ptr(), d_off.data_ptr(), d_ln.data_ptr(), L.nf, L.off.data_ptr(),
                                       L.word.data_ptr(), L.frame.data_ptr(), L.cap, L.finfo_ptr(),
                                       L.status.data_ptr(), s)
    lz4mi.frames_decompress_dev(arena.data_ptr(), L.off.data_ptr(), L.word.data_ptr(), L.frame.data_ptr(),
                                L.size.data_ptr(), L.cap, L.finfo_ptr(), L.nf, out.data_ptr(), d_foff.data_ptr(),
                                d_fcap.data_ptr(), s, verify_content=verify_content, chains=chains)
    t.cuda.synchronize()
    r.finfo, _ = L.finfo()
    r.out = out.cpu().numpy()
    assert (arena.cpu().numpy() == a).all()
    return r


def slot(r, k, arr=None):
    lo = FP.MARGIN + r.off[k]
    return (r.out if arr is None else arr)[lo:lo + r.total[k]]


CONFIGS = [{}, {"chains": True}, {"verify_content": True}, {"chains": True, "verify_content": True}]


@pytest.mark.parametrize("cfg", CONFIGS, ids=["plain", "chains", "content", "chains_content"])
def test_decompress_passes_failed_frames_over(cfg):
    with_v, without = batch(True, **cfg), batch(False, **cfg)
    failing = {C.NAMES.index(n) for n in C.expected_failing()}
    assert failing <= set(with_v.live) | {C.NAMES.index("r129_u_mid")}
    decoded = 0
    for k, name in enumerate(C.NAMES):
        if k in failing:
            want = with_v.index[k].copy()
            want[0] = C.ERR_BLOCK_CHECKSUM
            assert (with_v.finfo[k] == want).all(), name
            if k in with_v.live:
                assert (slot(with_v, k) == slot(with_v, k, with_v.init)).all(), (name, "a byte of its slot was written")
            continue
        assert (with_v.finfo[k] == without.finfo[k]).all(), name
        if k in with_v.live:
            assert (slot(with_v, k) == slot(without, k)).all(), name
            if not with_v.finfo[k, 0] and not with_v.finfo[k, 7]:
                base = name.split("_")[0]
                if base in C.CONTENTS:
                    assert (slot(with_v, k) == C.content(base)).all(), name
                    decoded += 1
    assert decoded >= 60
    # everything outside the slots of the frames that were decoded is the pattern
    care = np.ones(with_v.out.size, dtype=bool)
    for k in with_v.live:
        if k not in failing:
            care[FP.MARGIN + with_v.off[k]:FP.MARGIN + with_v.off[k] + with_v.total[k]] = False
    assert (with_v.out[care] == with_v.init[care]).all()


def test_block_checksum_comes_before_the_frames_own_error():
    own = {"pre_decode0": ERR_OFFSET0, "pre_content": ERR_CHECKSUM, "pre_stored_past": ERR_RANGE}
    for cfg in ({"verify_content": True}, {"chains": True, "verify_content": True}):
        with_v, without = batch(True, **cfg), batch(False, **cfg)
        for name in C.PRECEDENCE:
            k = C.NAMES.index(name)
            assert (int(without.finfo[k, 0]), int(without.finfo[k, 7])) == (own[name], 0), name
            assert (int(with_v.finfo[k, 0]), int(with_v.finfo[k, 7])) == (C.ERR_BLOCK_CHECKSUM, 0), name


# --------------------------------------------------------------------------------------- the wrapper
def alone(name, js_exact, verify_blocks):
    rep = {}
    try:
        out = F.decompress_frame_device(dev(C.zoo()[name][0]), js_exact=js_exact, report=rep, verify_blocks=verify_blocks)
        return 0, None, out.cpu().numpy(), rep.get("route")
    except lz4mi.Lz4miError as e:
        return e.status, str(e), None, rep.get("route")


def wrapper(names, **kw):
    a, off, ln = C.arena(0)
    arena, _, _ = dev_arena(0)
    idx = [C.NAMES.index(n) for n in names]
    rep = {}
    res = F.decompress_frames_device(arena, offsets=[int(off[k]) for k in idx], lengths=[int(ln[k]) for k in idx],
                                     return_errors=True, report=rep, **kw)
    return res, rep


def same_as_alone(names, res, js_exact, verify_blocks):
    for name, r in zip(names, res):
        st, msg, want, _ = alone(name, js_exact, verify_blocks)
        if st:
            assert isinstance(r, lz4mi.Lz4miError) and (r.status, str(r)) == (st, msg), (name, r, st)
        else:
            assert not isinstance(r, Exception), (name, r)
            assert np.array_equal(r.cpu().numpy(), want), name


def test_wrapper_equals_the_single_frame_call():
    res, rep = wrapper(C.NAMES, verify_blocks=True)
    same_as_alone(C.NAMES, res, False, True)
    for k, name in enumerate(C.NAMES):
        dmg = C.zoo()[name][1]
        assert rep["bad_block"][k] == (min(dmg) if dmg else None), name
        if dmg:
            assert (res[k].status, str(res[k])) == (C.ERR_BLOCK_CHECKSUM, "LZ4: Block Checksum Error"), name
            assert rep["routes"][k] == "batch" and res[k].frame_index == k, name
    assert rep["routes"][C.NAMES.index("empty")] != "batch" and rep["declined"][C.NAMES.index("empty")] == C.EMPTY
    assert rep["routes"].count("batch") >= 90 and rep["index_calls"] == 1


SUBSET = ("empty", "unsized2", "r129_u", "r129_u_mid", "r4096", "tiles2", "tiles2_sum2", "five_plain", "bad_magic",
          "tiles5_b2_mid") + C.PRECEDENCE


def test_wrapper_declined_frames_take_the_lone_route_js_exact():
    res, rep = wrapper(SUBSET, verify_blocks=True, js_exact=True)
    same_as_alone(SUBSET, res, True, True)
    for name in ("empty", "unsized2", "r129_u", "r129_u_mid"):
        k = SUBSET.index(name)
        assert rep["declined"][k] and rep["routes"][k] != "batch", name
    k = SUBSET.index("r129_u_mid")      # declined, its blocks listed: checked all the same, and refused by the lone route
    assert rep["bad_block"][k] == 0 and res[k].status == C.ERR_BLOCK_CHECKSUM
    assert rep["bad_block"][SUBSET.index("unsized2")] is None


def test_wrapper_without_the_keyword_is_what_it_was():
    res, rep = wrapper(SUBSET)
    assert "bad_block" not in rep
    same_as_alone(SUBSET, res, False, False)
    for name, r in zip(SUBSET, res):
        if name in C.PRECEDENCE:
            assert isinstance(r, lz4mi.Lz4miError) and r.status != C.ERR_BLOCK_CHECKSUM, name


def test_wrapper_small_cap_runs_the_index_and_the_verify_again():
    res, rep = wrapper(SUBSET, verify_blocks=True, cap_blocks=3)
    assert rep["index_calls"] == 2
    same_as_alone(SUBSET, res, False, True)
    assert rep["bad_block"][SUBSET.index("tiles5_b2_mid")] == 2


def test_round_trip_and_one_flipped_byte():
    t = torch_()
    rng = np.random.default_rng(5)
    bufs = [C.content("tiles2"), C.content("r4097"), C.content("five"), C.content("r1"),
            rng.integers(0, 4, 70001, dtype=np.uint8), C.content("tiles1")]
    frames = F.compress_frames_device([dev(b) for b in bufs], block_size=65536, block_checksum=True)
    assert all(int(f[4]) & 0x10 for f in frames)
    frames = [f.clone() for f in frames]
    rep = {}
    back = F.decompress_frames_device(frames, verify_blocks=True, report=rep)
    assert rep["routes"] == ["batch"] * len(bufs) and rep["bad_block"] == [None] * len(bufs)
    for b, o in zip(bufs, back):
        assert np.array_equal(o.cpu().numpy(), b)
    frames[4][19 + 1234] ^= 0x40        # (a sized frame's first payload starts at byte 19)
    t.cuda.synchronize()
    rep = {}
    back = F.decompress_frames_device(frames, verify_blocks=True, return_errors=True, report=rep)
    for k, (b, o) in enumerate(zip(bufs, back)):
        if k == 4:
            assert isinstance(o, lz4mi.Lz4miError) and o.status == C.ERR_BLOCK_CHECKSUM and rep["bad_block"][k] == 0
        else:
            assert np.array_equal(o.cpu().numpy(), b) and rep["bad_block"][k] is None
