"""LZ4MI_FRAMES_CHAINS on the decode side (lz4mi_frames_decompress, frame.decompress_frames_device): frames whose
blocks read the blocks before them decoded in the batch, one wave per frame in block order. Expected bytes and
statuses are the CPU oracle's (frames_chains_decode_common.want), cross-checked against the single-frame call; the
inputs and their claims are tests/frames_chains_decode_common.py."""
import functools

import numpy as np
import pytest

import footprint_common as FP
import frames_chain_common as CC
import frames_chains_decode_common as D
import frames_common as C
import lz4mi
from lz4mi import shard

pytestmark = pytest.mark.gpu
GUARD = 48          # filler bytes between two frames' slots in `out` (slots at 16-byte-aligned offsets)
MODES = pytest.mark.parametrize("exact", [False, True], ids=["spec", "js_exact"])


def torch_():
    import torch
    return torch


def dev(a):
    return torch_().from_numpy(np.array(a)).cuda()


class Run:
    pass


def run(packed, fill, exact, verify, chains=True, cap=None, roomless=(), measure=False):
    """Index and decode of the frames in `packed` (arena, offsets, lengths). `out` begins FP.MARGIN bytes into a
    buffer of `fill` bytes; the slots are packed from frame_out_off 0 at 16-byte-aligned offsets, GUARD bytes
    between two. roomless: frames that get no room (capacity 0). measure: LZ4MI_FRAMES_MEASURE for the index."""
    from lz4mi.frame import content_size_bound
    t = torch_()
    a, off, ln = packed
    nf = off.size
    arena, d_off, d_ln = dev(a), dev(off.astype(np.int64)), dev(ln.astype(np.int64))
    cap = cap if cap is not None else sum(len(D.blocks_of(a[int(o):int(o + n)])) for o, n in zip(off, ln)) + 8
    blk_off = t.zeros(cap, dtype=t.int64, device="cuda")
    blk32 = t.zeros((3, cap), dtype=t.int32, device="cuda")
    fin = t.zeros(8 * nf + 4, dtype=t.int64, device="cuda")
    lz4mi.frames_index_dev(arena.data_ptr(), d_off.data_ptr(), d_ln.data_ptr(), nf, blk_off.data_ptr(),
                           blk32[0].data_ptr(), blk32[1].data_ptr(), blk32[2].data_ptr(), cap, fin.data_ptr(),
                           fin.data_ptr() + 64 * nf, js_exact=exact, measure=measure)
    h = fin.cpu().numpy()
    r = Run()
    r.exact = exact
    r.index = h[:8 * nf].reshape(nf, 8).copy()
    assert h[8 * nf] <= cap
    listed = int(h[8 * nf + 1])
    r.live = [k for k in range(nf) if not r.index[k, 0] and not r.index[k, 7] and k not in roomless and
              int(r.index[k, 2]) <= content_size_bound(int(ln[k]))]
    r.total = {k: int(r.index[k, 3]) for k in r.live}
    r.off, at = {}, 0
    for k in r.live:
        r.off[k] = at
        at = (at + r.total[k] + GUARD + 15) & ~15
    r.init = np.full(FP.MARGIN + at + FP.MARGIN, fill, dtype=np.uint8)
    buf = dev(r.init)
    foff, fcap = np.zeros(nf, dtype=np.int64), np.zeros(nf, dtype=np.int64)
    for k in r.live:
        foff[k], fcap[k] = r.off[k], r.total[k]
    d_foff, d_fcap = dev(foff), dev(fcap)
    lz4mi.frames_decompress_dev(arena.data_ptr(), blk_off.data_ptr(), blk32[0].data_ptr(), blk32[1].data_ptr(),
                                blk32[2].data_ptr(), listed, fin.data_ptr(), nf, buf.data_ptr() + FP.MARGIN,
                                d_foff.data_ptr(), d_fcap.data_ptr(), js_exact=exact, verify_content=verify,
                                chains=chains)
    t.cuda.synchronize()
    r.finfo = fin.cpu().numpy()[:8 * nf].reshape(nf, 8)
    r.out = buf.cpu().numpy()
    assert (arena.cpu().numpy() == a).all(), "`in` was written"
    r.result = [(int(r.finfo[k, 0]), int(r.finfo[k, 7])) for k in range(nf)]
    return r


def slot(r, k):
    lo = FP.MARGIN + r.off[k]
    return r.out[lo:lo + r.total[k]]


def assert_untouched_outside(r, what):
    """No byte outside out[frame_out_off[f] .. +finfo[f][3]) of a frame that went into the decode has changed; a
    frame declined before the decode has none changed at all."""
    mine = np.zeros(r.out.size, dtype=bool)
    for k in r.live:
        if r.result[k][1] not in (0, C.LAYOUT, C.DEPENDENT):
            continue
        lo = FP.MARGIN + r.off[k]
        assert 0 <= r.finfo[k, 3] <= r.total[k]
        # (a decoded frame with a content size holds that many bytes: zeros behind what its blocks wrote)
        whole = r.result[k][0] in (0, D.ERR_CHECKSUM) and r.result[k][1] == 0
        mine[lo:lo + (r.total[k] if whole else int(r.finfo[k, 3]))] = True
    bad = np.nonzero((r.out != r.init) & ~mine)[0]
    assert not bad.size, (what, "stray byte at out[%d]" % (int(bad[0]) - FP.MARGIN), bad.size)


@functools.lru_cache(maxsize=None)
def alone(frame_bytes, exact, verify):
    from lz4mi import frame as F
    try:
        out = F.decompress_frame_device(dev(np.frombuffer(frame_bytes, dtype=np.uint8)), js_exact=exact,
                                        verify_checksum=verify)
        return 0, out.cpu().numpy()
    except lz4mi.Lz4miError as e:
        return e.status, None


def check_frames(r, frames, verify, skip=()):
    """Every frame that is not declined against the oracle and the single-frame call. -> number decoded."""
    n = 0
    for k, f in enumerate(frames):
        st, dc = r.result[k]
        if dc or k in skip:
            continue
        wst, wbytes = D.want(f, r.exact, verify)
        assert st == wst, (k, st, wst)
        ast, abytes = alone(f.tobytes(), r.exact, verify)
        assert ast == wst, (k, ast, wst)
        if wst not in (0, D.ERR_CHECKSUM):
            continue
        got = slot(r, k)
        assert got.size == wbytes.size and (got == wbytes).all(), (k, int(np.argmax(got != wbytes[:got.size])))
        assert abytes is None or (abytes == wbytes).all(), k
        size = int(shard.frame_blocks(f)[0]["content_size"])
        assert r.finfo[k, 3] <= r.total[k] and (not size or r.total[k] == size)
        n += 1
    return n


# ------------------------------------------------------------------------------------------------ the chain zoo
@functools.lru_cache(maxsize=None)
def chain_run(fill, exact, verify, chains=True):
    assert D.claims()
    return run(D.chain_arena(fill), fill, exact, verify, chains)


@MODES
@pytest.mark.parametrize("verify", [False, True], ids=["noverify", "verify"])
@pytest.mark.parametrize("fill", D.FILLS)
def test_chain_zoo(fill, exact, verify):
    r = chain_run(fill, exact, verify)
    frames = [D.chain_frame(n) for n in D.NAMES64]
    for k, name in enumerate(D.NAMES64):
        assert r.result[k][1] == (C.EMPTY if name == "n0" else 0), (name, r.result[k])
        if name != "n0":
            assert r.finfo[k, 3] == CC.content(name).size, name
    assert check_frames(r, frames, verify) == len(D.NAMES64) - 1
    if not exact:
        for k, name in enumerate(D.NAMES64):
            assert name == "n0" or (r.result[k] == (0, 0) and (slot(r, k) == CC.content(name)).all()), name
    assert_untouched_outside(r, (fill, exact, verify))
    assert r.off[r.live[0]] == 0 and all(o % 16 == 0 for o in r.off.values())


@MODES
def test_four_mib_blocks(exact):
    assert D.claims()
    r = run(D.chain_arena(0xFF, "c4m"), 0xFF, exact, True)
    frames = [D.chain_frame(n, "c4m") for n in D.NAMES4M]
    assert [dc for _, dc in r.result] == [0, 0]
    assert check_frames(r, frames, True) == 2
    assert r.finfo[1, 3] == 4194304 + 70000
    assert_untouched_outside(r, exact)


@MODES
def test_flag_off_declines_the_chains_and_the_wrapper_gives_the_same(exact):
    from lz4mi import frame as F
    r = chain_run(0x00, exact, True, chains=False)
    for k, name in enumerate(D.NAMES64):
        if name in D.CHAINS64 and name != "r65536x3":
            assert r.result[k] == (0, C.DEPENDENT), (name, r.result[k])
    assert r.result[D.NAMES64.index("r65536x3")][1] == 0          # every block stored: nothing reads a block
    frames = [dev(D.chain_frame(n)) for n in D.NAMES64]
    reps, outs = [{}, {}], []
    for rep, chains in zip(reps, (False, True)):
        outs.append(F.decompress_frames_device(frames, js_exact=exact, report=rep, return_errors=True, chains=chains))
    for k, name in enumerate(D.NAMES64):
        x, y = outs[0][k], outs[1][k]
        if isinstance(x, Exception):
            assert isinstance(y, Exception) and x.status == y.status, name
        else:
            assert (x.cpu().numpy() == y.cpu().numpy()).all(), name
    assert [d for d in reps[1]["declined"]] == [C.EMPTY if n == "n0" else 0 for n in D.NAMES64]
    for name in D.CHAINS64:
        if name != "r65536x3":
            assert reps[0]["declined"][D.NAMES64.index(name)] == C.DEPENDENT, name


# ------------------------------------------------------------------------------------------------ the frame zoo
@functools.lru_cache(maxsize=None)
def zoo_run(fill, exact, verify=True):
    assert D.claims()
    return run(C.arena(fill), fill, exact, verify, cap=C.need_blocks())


@MODES
@pytest.mark.parametrize("verify", [False, True], ids=["noverify", "verify"])
def test_frame_zoo_statuses_and_declines(exact, verify):
    r = zoo_run(0x00, exact, verify)
    got = dict(zip(C.NAMES, r.result))
    want = {n: D.expected_zoo(n, exact, verify) for n in C.NAMES}
    assert got == want, {n: (got[n], want[n]) for n in C.NAMES if got[n] != want[n]}
    # by name: what the issue sets
    assert got["huge_size"] == (0, C.OUT_CAP)
    assert got["below_start"] == (C.ERR_DICT_OOB, 0)
    assert got["decode0"] == (C.ERR_OFFSET0, 0) and got["stored_past"] == (C.ERR_RANGE, 0)
    assert got["csum_flip"] == ((C.ERR_CHECKSUM if verify else 0), 0)
    assert got["text_isc"] == ((C.ERR_CHECKSUM if exact and verify else 0), 0)
    for n in C.NAMES:
        if C.is_dependent_five(n):
            sized = n.split("_")[1][1] == "s"
            assert got[n][1] == (C.UNSIZED_EXACT if exact and not sized else 0), (n, got[n])
        before = C.expected_batch(n, exact, False, verify)
        if before[1] != C.DEPENDENT:
            assert got[n] == before, (n, got[n], before)         # every other frame keeps its outcome
    assert not [n for n in C.NAMES if got[n][1] == C.DEPENDENT]
    assert sum(1 for n in C.NAMES if got[n][1] == 0) >= (31 if exact else 52)


@MODES
@pytest.mark.parametrize("fill", D.FILLS)
def test_frame_zoo_bytes(fill, exact):
    r = zoo_run(fill, exact)
    frames = [C.zoo()[n] for n in C.NAMES]
    skip = {C.NAMES.index("huge_size")}
    assert check_frames(r, frames, True, skip) >= (26 if exact else 47)
    names = [n for n in C.NAMES if C.is_dependent_five(n) and (not exact or n.split("_")[1][1] == "s")]
    names += [n for n in C.FIVE_INDEPENDENT_SIZED if n != "decode0"]
    for n in names:
        k = C.NAMES.index(n)
        st, dc = r.result[k]
        assert dc == 0 and st in (0, C.ERR_CHECKSUM), (n, st, dc)
        assert (slot(r, k) == D.want(C.zoo()[n], exact, False)[1]).all(), n
        if exact:          # the reference's bytes differ from the content in the text blocks
            assert (slot(r, k) != C.content("five")).any(), n
    # decode0 in a reference mode: block 0 fails, blocks 3 and 4 (whose rewrites read below them) go through the
    # chain behind the isolated blocks 1 and 2
    k = C.NAMES.index("decode0")
    assert r.result[k] == (C.ERR_OFFSET0, 0) and r.finfo[k, 3] == C.content("five").size
    ref = D.want(C.zoo()["cfive_isn"], exact, False)[1]
    assert (slot(r, k)[D.BS:] == ref[D.BS:]).all()
    assert_untouched_outside(r, (fill, exact))


# ------------------------------------------------------------------------------------ a failure inside a chain
@MODES
@pytest.mark.parametrize("fill", D.FILLS)
def test_failure_inside_a_chain(fill, exact):
    assert D.claims()
    g, base, end = D.damaged_five()
    frames = [C.zoo()["c65536_isn"], g, C.zoo()["c65535_isn"]]
    r = run(D.pack16(frames, fill), fill, exact, True)
    assert r.result[1] == (D.ERR_OFFSET0, 0), r.result[1]
    assert r.finfo[1, 3] == end and r.total[1] == C.content("five").size
    got = slot(r, 1)
    assert (got[:end] == D.partial_five(exact)).all()
    assert (got[end:] == fill).all(), "blocks 3 and 4 were written"
    assert alone(g.tobytes(), exact, True)[0] == D.ERR_OFFSET0
    assert r.result[0] == (0, 0) and r.result[2] == (0, 0)
    assert check_frames(r, frames, True, skip={1}) == 2
    assert_untouched_outside(r, (fill, exact))


# ------------------------------------------------------------------------------------ footprint and isolation
@MODES
@pytest.mark.parametrize("fill", D.FILLS)
def test_below_start_behind_a_decoded_frame_reads_nothing_of_it(fill, exact):
    assert D.claims()
    frames = list(D.neighbours())
    r = run(D.pack16(frames, fill), fill, exact, True)
    assert r.result == [(0, 0), (D.ERR_DICT_OOB, 0), (0, 0)], r.result
    assert r.finfo[1, 3] == 0
    assert check_frames(r, frames, True, skip={1}) == 2
    assert (slot(r, 1) == fill).all()
    assert_untouched_outside(r, (fill, exact))
    # the same frame first in the batch, at frame_out_off 0: nothing below `out` is read as history or written
    r = run(D.pack16(frames[1:], fill), fill, exact, True)
    assert r.result == [(D.ERR_DICT_OOB, 0), (0, 0)] and r.off[0] == 0
    assert_untouched_outside(r, (fill, exact, "first"))


@pytest.mark.parametrize("fill", D.FILLS)
def test_declined_frames_are_not_written(fill):
    """Frames declined before the decode keep every byte, chain frames among them: one without a content size in a
    reference mode (UNSIZED_EXACT, by the decode call: the index ran without the mode), one given no room (OUT_CAP:
    its slot would begin at frame_out_off 0, inside the first frame's)."""
    assert D.claims()
    z = C.zoo()
    frames = [z["cfive_dsn"], z["cfive_dun"], D.chain_frame("text4"), z["cfive_isn"]]
    packed = D.pack16(frames, fill)
    r = run(packed, fill, False, False)
    assert r.result == [(0, 0)] * 4 and check_frames(r, frames, False) == 4
    r = run(packed, fill, False, False, roomless={2})
    assert r.result == [(0, 0), (0, 0), (0, C.OUT_CAP), (0, 0)] and check_frames(r, frames, False) == 3
    assert_untouched_outside(r, (fill, "no room"))
    # the reference mode given to the decode only: the unsized chain frame was measured, has a slot and is declined
    t = torch_()
    a, off, ln = packed
    arena, d_off, d_ln = dev(a), dev(off.astype(np.int64)), dev(ln.astype(np.int64))
    cap = 32
    blk_off = t.zeros(cap, dtype=t.int64, device="cuda")
    blk32 = t.zeros((3, cap), dtype=t.int32, device="cuda")
    fin = t.zeros(8 * 4 + 4, dtype=t.int64, device="cuda")
    lz4mi.frames_index_dev(arena.data_ptr(), d_off.data_ptr(), d_ln.data_ptr(), 4, blk_off.data_ptr(),
                           blk32[0].data_ptr(), blk32[1].data_ptr(), blk32[2].data_ptr(), cap, fin.data_ptr(),
                           fin.data_ptr() + 64 * 4)
    h = fin.cpu().numpy()
    totals = [int(h[8 * k + 3]) for k in range(4)]
    assert not h[:32].reshape(4, 8)[:, 7].any() and totals[1] == C.content("five").size
    offs = [0]
    for n in totals[:-1]:
        offs.append((offs[-1] + n + GUARD + 15) & ~15)
    init = np.full(FP.MARGIN + offs[-1] + totals[-1] + FP.MARGIN, fill, dtype=np.uint8)
    buf = dev(init)
    d_foff, d_fcap = dev(np.array(offs, dtype=np.int64)), dev(np.array(totals, dtype=np.int64))
    lz4mi.frames_decompress_dev(arena.data_ptr(), blk_off.data_ptr(), blk32[0].data_ptr(), blk32[1].data_ptr(),
                                blk32[2].data_ptr(), int(h[33]), fin.data_ptr(), 4, buf.data_ptr() + FP.MARGIN,
                                d_foff.data_ptr(), d_fcap.data_ptr(), js_exact=True, chains=True)
    t.cuda.synchronize()
    fi = fin.cpu().numpy()[:32].reshape(4, 8)
    assert fi[:, 7].tolist() == [0, C.UNSIZED_EXACT, 0, 0] and not fi[:, 0].any()
    out = buf.cpu().numpy()
    lo = FP.MARGIN + offs[1]
    assert (out[lo - GUARD:lo + totals[1] + GUARD] == fill).all(), "a declined frame's slot was written"
    for k in (0, 2, 3):
        lo = FP.MARGIN + offs[k]
        assert (out[lo:lo + totals[k]] == D.want(frames[k], True, False)[1]).all(), k


# ------------------------------------------------------------------------------------------------ many frames
def test_sixty_five_two_block_frames():
    assert D.claims()
    frames = list(D.many_frames())
    assert len(frames) == 65
    r = run(D.pack16(frames, 0xFF), 0xFF, False, True)
    assert r.result == [(0, 0)] * 65
    for k, f in enumerate(frames):
        st, wbytes = D.want(f, False, True)
        assert st == 0 and (slot(r, k) == wbytes).all() and r.finfo[k, 3] == D.BS + 100, k
    assert_untouched_outside(r, "many")
    r = run(D.pack16(frames[:3] + frames[62:], 0x00), 0x00, True, False)
    assert r.result == [(0, 0)] * 6 and check_frames(r, frames[:3] + frames[62:], False) == 6


# ------------------------------------------------------------------------------------------------ round trip
def test_round_trip_through_both_batches():
    from lz4mi import frame as F
    t = torch_()
    srcs = [CC.content(n) for n in D.NAMES64]
    bufs = [dev(s) if s.size else t.zeros(0, dtype=t.uint8, device="cuda") for s in srcs]
    crep, drep = {}, {}
    frames = F.compress_frames_device(bufs, block_size=65536, independent=False, chains=True, report=crep)
    assert all(rt == "batch" for rt in crep["routes"]), crep["routes"]
    outs = F.decompress_frames_device(frames, report=drep, chains=True)
    empty = D.NAMES64.index("n0")          # the empty frame is the one the batch never takes (EMPTY)
    for k, (s, o) in enumerate(zip(srcs, outs)):
        assert drep["declined"][k] == (C.EMPTY if k == empty else 0), D.NAMES64[k]
        assert k == empty or drep["routes"][k] == "batch", D.NAMES64[k]
        assert o.numel() == s.size and (o.cpu().numpy() == s).all(), D.NAMES64[k]
    # the frames are the oracle's dependent frames (content size, no content checksum)
    f0 = CC.oracle_frame("text4", 65536, False, False, True)
    assert frames[0].numel() == f0.size and (frames[0].cpu().numpy() == f0).all()
