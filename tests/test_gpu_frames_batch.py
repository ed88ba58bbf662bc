"""A batch of frames decoded on the device in one call (lz4mi_frames_index / lz4mi_frames_decompress and
frame.decompress_frames_device) on the zoo of tests/frames_common.py: the device index against the host
index, the decoded frames against the single-frame call and the oracle, the exact set of declined frames, the
calls' footprint, capacities, content checksums and the wrapper."""
import functools

import numpy as np
import pytest

import footprint_common as FP
import frames_common as C
import lz4mi
import oracle as O

pytestmark = pytest.mark.gpu
SENT = 16          # sentinel entries behind every list and around finfo / totals
GUARD = 48         # filler bytes between two frames' slots in `out`


def torch_():
    import torch
    return torch


def dev(a):
    return torch_().from_numpy(np.array(a)).cuda()


@functools.lru_cache(maxsize=None)
def dev_arena(fill):
    a, off, ln = C.arena(fill)
    return dev(a), dev(off.astype(np.int64)), dev(ln.astype(np.int64))


class Lists:
    """The index call's outputs, SENT sentinel entries behind each list and on both sides of finfo + totals."""

    def __init__(self, nframes, cap):
        t = torch_()
        self.nf, self.cap = nframes, cap
        self.off = t.full((cap + SENT,), FP.FILL, dtype=t.int64, device="cuda")
        self.word, self.frame, self.size = (t.full((cap + SENT,), FP.FILL, dtype=t.int32, device="cuda") for _ in range(3))
        self.fin = t.full((SENT + 8 * nframes + 4 + SENT,), FP.FILL, dtype=t.int64, device="cuda")

    def finfo_ptr(self):
        return self.fin.data_ptr() + 8 * SENT

    def totals_ptr(self):
        return self.finfo_ptr() + 64 * self.nf

    def host(self):
        fin = self.fin.cpu().numpy()
        assert (fin[:SENT] == FP.FILL).all() and (fin[SENT + 8 * self.nf + 4:] == FP.FILL).all(), "finfo / totals sentinels"
        res = {"finfo": fin[SENT:SENT + 8 * self.nf].reshape(self.nf, 8), "totals": fin[SENT + 8 * self.nf:][:4]}
        listed = int(res["totals"][1])
        assert listed <= self.cap
        for key, arr in (("blk_in_off", self.off), ("blk_word", self.word), ("blk_frame", self.frame),
                         ("blk_size", self.size)):
            h = arr.cpu().numpy()
            assert (h[listed:] == FP.FILL).all(), f"{key}: written behind the {listed} listed blocks"
            res[key] = h[:listed].astype(np.uint64 if key == "blk_in_off" else np.uint32)
        return res


def index_dev(arena, off, ln, cap, **kw):
    L = Lists(off.numel(), cap)
    lz4mi.frames_index_dev(arena.data_ptr(), off.data_ptr(), ln.data_ptr(), off.numel(), L.off.data_ptr(),
                           L.word.data_ptr(), L.frame.data_ptr(), L.size.data_ptr(), cap, L.finfo_ptr(), L.totals_ptr(),
                           **kw)
    return L


def same_index(got, want, what):
    listed = int(want["totals"][1])
    assert got["totals"].tolist() == want["totals"].tolist(), what
    bad = np.nonzero((got["finfo"] != want["finfo"]).any(axis=1))[0]
    assert not bad.size, (what, int(bad[0]), got["finfo"][bad[0]].tolist(), want["finfo"][bad[0]].tolist())
    for key in ("blk_in_off", "blk_word", "blk_frame", "blk_size"):
        assert (got[key] == want[key][:listed]).all(), (what, key)


@pytest.mark.parametrize("fill", C.FILLS)
@pytest.mark.parametrize("kw", [{}, {"measure": True}, {"js_exact": True}], ids=["layout", "measure", "js_exact"])
def test_device_index_equals_host_index(fill, kw):
    a, off, ln = C.arena(fill)
    arena, d_off, d_ln = dev_arena(fill)
    for cap in (C.need_blocks(), C.need_blocks() - 1, 40):
        got = index_dev(arena, d_off, d_ln, cap, **kw).host()
        same_index(got, lz4mi.host_frames_index(a, off, ln, cap, **kw), (fill, kw, cap))
    assert (arena.cpu().numpy() == a).all()


@pytest.mark.parametrize("n", [1, 63, 64, 65, 1025])
def test_device_index_frame_counts(n):
    """One-byte contents: the lane (1), workgroup (63 / 64 / 65) and scan-carry (1025 > 4 x 256) boundaries."""
    a, off, ln = C.pack(C.tiny_frames(n))
    got = index_dev(dev(a), dev(off.astype(np.int64)), dev(ln.astype(np.int64)), n).host()
    same_index(got, lz4mi.host_frames_index(a, off, ln, n), n)
    assert got["finfo"][:, 4].tolist() == list(range(n)) and got["totals"].tolist() == [n, n, n, 0]


# ------------------------------------------------------------------------------------- both calls on the zoo
class Run:
    pass


@functools.lru_cache(maxsize=None)
def batch(fill, js_exact=False, measure=False, verify=True, short=None, index_js_exact=None):
    """Index and decompress of the whole zoo. `out` is pre-filled with a pattern, the frames' slots lie GUARD
    bytes apart at residues 1, 5, 15 (mod 16) with FP.MARGIN bytes on either side; `short`: that frame's
    capacity is one byte short of its total; index_js_exact: the index call's flag when it is not the decode's.
    A frame whose content size is above frame.content_size_bound gets no room, as in the wrapper."""
    from lz4mi.frame import content_size_bound
    t = torch_()
    a, off, ln = C.arena(fill)
    arena, d_off, d_ln = dev_arena(fill)
    r = Run()
    r.js_exact = js_exact
    L = index_dev(arena, d_off, d_ln, C.need_blocks(), measure=measure,
                  js_exact=js_exact if index_js_exact is None else index_js_exact)
    r.index = L.host()
    fi = r.index["finfo"]
    r.live = [k for k in range(len(C.NAMES)) if not fi[k, 0] and not fi[k, 7] and
              int(fi[k, 2]) <= content_size_bound(int(ln[k]))]
    r.total = {k: int(fi[k, 3]) for k in r.live}
    offs = FP.layout([r.total[k] for k in r.live], guard=GUARD)
    r.off = dict(zip(r.live, offs))
    size = FP.MARGIN + offs[-1] + r.total[r.live[-1]] + FP.MARGIN
    r.init = FP.pattern(size, 1 if fill else 0)
    out = dev(r.init)
    foff = np.zeros(len(C.NAMES), dtype=np.int64)
    fcap = np.zeros(len(C.NAMES), dtype=np.int64)
    for k in r.live:
        foff[k], fcap[k] = FP.MARGIN + r.off[k], r.total[k] - (1 if C.NAMES[k] == short else 0)
    d_foff, d_fcap = dev(foff), dev(fcap)
    lz4mi.frames_decompress_dev(arena.data_ptr(), L.off.data_ptr(), L.word.data_ptr(), L.frame.data_ptr(),
                                L.size.data_ptr(), L.cap, L.finfo_ptr(), len(C.NAMES), out.data_ptr(), d_foff.data_ptr(),
                                d_fcap.data_ptr(), js_exact=js_exact, verify_content=verify)
    t.cuda.synchronize()
    after = L.host()
    for key in ("blk_in_off", "blk_word", "blk_frame", "blk_size"):
        assert (after[key] == r.index[key]).all(), key          # the lists are read only
    assert (d_foff.cpu().numpy() == foff).all() and (d_fcap.cpu().numpy() == fcap).all()
    assert (arena.cpu().numpy() == a).all(), "`in` was written"
    r.finfo = after["finfo"]
    r.out = out.cpu().numpy()
    r.result = {C.NAMES[k]: (int(r.finfo[k, 0]), int(r.finfo[k, 7])) for k in range(len(C.NAMES))}
    return r


def frame_bytes(r, name):
    k = C.NAMES.index(name)
    return r.out[FP.MARGIN + r.off[k]:FP.MARGIN + r.off[k] + r.total[k]]


@functools.lru_cache(maxsize=None)
def alone(name, js_exact):
    """The single-frame call on that frame alone -> (status, bytes or None, route)."""
    from lz4mi import frame as F
    rep = {}
    try:
        out = F.decompress_frame_device(dev(C.zoo()[name]), js_exact=js_exact, report=rep)
        return 0, out.cpu().numpy(), rep.get("route")
    except lz4mi.Lz4miError as e:
        return e.status, None, rep.get("route")


@pytest.mark.parametrize("js_exact", [False, True], ids=["spec", "js_exact"])
@pytest.mark.parametrize("measure", [False, True], ids=["layout", "measure"])
def test_statuses_and_declines_by_name(js_exact, measure):
    """The exact status and decline code of every frame: the guard against a batch that declines everything."""
    r = batch(0x00, js_exact, measure)
    want = {n: C.expected_batch(n, js_exact, measure) for n in C.NAMES}
    assert r.result == want, {n: (r.result[n], want[n]) for n in C.NAMES if r.result[n] != want[n]}
    declined = {n for n in C.NAMES if r.result[n][1]}
    named = {n for n in C.NAMES if C.is_dependent_five(n) or n.startswith("c0_") or n.startswith("cut_")}
    named |= {"huge_size"}       # (given no room: its content size is above what its bytes can decode to)
    if js_exact:
        named |= {n for n in C.NAMES if n == "partial_unsized" or (n[0] == "c" and n.split("_")[1][1] == "u")}
        named |= {"below_start"} | set(C.FIVE_INDEPENDENT_SIZED)
    if measure:
        named |= {"decode0", "stored_past", "zero_tail", "zero_tail5", "below_start"}
    else:
        named |= {"partial_sized"}
    assert declined == named
    assert ("partial_sized" in declined) == (not measure)
    assert len(C.NAMES) - len(declined) >= (20 if js_exact else 36)


@pytest.mark.parametrize("js_exact", [False, True], ids=["spec", "js_exact"])
@pytest.mark.parametrize("fill", C.FILLS)
def test_decoded_frames_equal_the_single_frame_call_and_the_oracle(fill, js_exact):
    r = batch(fill, js_exact)
    checked = 0
    for k, name in enumerate(C.NAMES):
        st, dc = r.result[name]
        if dc:
            continue
        ast, abytes, _ = alone(name, js_exact)
        assert st == ast, (name, st, ast)
        if st:
            continue
        got = frame_bytes(r, name)
        assert r.finfo[k, 3] <= r.total[k] and got.size == abytes.size and (got == abytes).all(), name
        ost, want = O.decompress_frame(C.zoo()[name], verify_checksum=False, js_compat=js_exact)
        assert ost == 0 and want.size == got.size and (got == want).all(), name
        checked += 1
    assert checked >= (16 if js_exact else 32)
    # the zero tail: the pattern behind what the blocks wrote became zeros, up to the content size and no further
    for name, tail in (("zero_tail", 70000 - 65536), ("zero_tail5", 5)):
        k = C.NAMES.index(name)
        got = frame_bytes(r, name)
        assert r.finfo[k, 3] == 65536 and got.size == 65536 + tail and not got[65536:].any()
        assert r.init[FP.MARGIN + r.off[k] + 65536:][:tail].any()      # (the pattern there was not zeros)
    m = batch(fill, js_exact, measure=True)
    if not js_exact:
        assert m.result["partial_sized"] == (0, 0) and (frame_bytes(m, "partial_sized") == C.partial_content()).all()
        assert (frame_bytes(m, "partial_unsized") == C.partial_content()).all()


@pytest.mark.parametrize("js_exact", [False, True], ids=["spec", "js_exact"])
@pytest.mark.parametrize("measure", [False, True], ids=["layout", "measure"])
def test_bytes_written(js_exact, measure):
    """finfo[f][3] after the decode, exactly, for every frame that is not declined, failing ones included: what
    lz4mi_frame_decompress reports as written for the frames it takes (those with a content size), the oracle's
    output size for the others. The one documented difference: a stored block that fails ERR_RANGE writes and
    counts nothing here; there its bytes are copied clipped at the content size and counted."""
    r = batch(0xFF, js_exact, measure)
    seen = {"ok": 0, "failing": 0, "unsized": 0}
    for k, name in enumerate(C.NAMES):
        st, dc = r.result[name]
        if dc:
            continue
        f = dev(C.zoo()[name])
        size = int(r.finfo[k, 2])
        got = int(r.finfo[k, 3])
        if size:      # (every frame here that has a content size is one lz4mi_frame_decompress takes)
            out = torch_().empty(size, dtype=torch_().uint8, device="cuda")
            try:
                info = lz4mi.frame_decompress_dev(f.data_ptr(), f.numel(), out.data_ptr(), size, js_exact=js_exact)
            except lz4mi.Lz4miError as e:      # the partial-block frame, measured: not the layout route's frame
                assert e.status == lz4mi.ERR_ARG and name == "partial_sized" and measure and st == 0
                assert got == C.partial_content().size
                continue
            assert info["status"] == (0 if st == C.ERR_CHECKSUM else st), name
            if name == "stored_past":
                assert (got, info["written"]) == (0, 100)
            else:
                assert got == info["written"], (name, got, info["written"])
            if info["status"] == 0:
                ost, want = O.decompress_frame(C.zoo()[name], verify_checksum=False, js_compat=js_exact)
                nz = np.nonzero(want)[0]
                assert ost == 0 and got <= want.size and (nz.size == 0 or got > nz[-1]), name
            seen["failing" if st and st != C.ERR_CHECKSUM else "ok"] += 1
        elif st:      # a header error: nothing was written
            assert got == 0 and name in ("bad_magic", "bad_version"), name
        else:
            ost, want = O.decompress_frame(C.zoo()[name], verify_checksum=False)
            assert ost == 0 and got == want.size == r.total[k], (name, got, want.size)
            seen["unsized"] += 1
    assert seen["ok"] >= 10 and (js_exact or seen["unsized"] >= 10)
    if not js_exact and not measure:
        assert seen["failing"] >= 3                     # decode0, stored_past, below_start
        assert r.finfo[C.NAMES.index("decode0"), 3] == C.content("five").size      # its blocks 1 to 4 decoded
        assert r.finfo[C.NAMES.index("below_start"), 3] == 0


def test_js_exact_given_to_the_decode_only_declines_unsized_frames():
    """The index ran without LZ4MI_JS_EXACT, so unsized frames were measured; the decode call with the flag declines
    them itself (a contiguous reference-mode decode is not the reference's window decode) and writes none of them."""
    r = batch(0x00, True, index_js_exact=False)
    want = {n: C.expected_batch(n, True) for n in C.NAMES}
    assert r.result == want, {n: (r.result[n], want[n]) for n in C.NAMES if r.result[n] != want[n]}
    unsized = [k for k in r.live if r.result[C.NAMES[k]] == (0, C.UNSIZED_EXACT)]
    assert len(unsized) >= 15
    for k in unsized:
        lo = FP.MARGIN + r.off[k]
        assert (r.out[lo:lo + r.total[k]] == r.init[lo:lo + r.total[k]]).all(), C.NAMES[k]


def expected_image(r):
    """-> (image, care): the pre-filled pattern, the decoded frames' bytes in their slots; the slot of a frame
    with a failing block or declined after the decode (LAYOUT, DEPENDENT) is the call's to scribble in."""
    image, care = r.init.copy(), np.ones(r.init.size, dtype=bool)
    for k in r.live:
        name = C.NAMES[k]
        st, dc = r.result[name]
        lo = FP.MARGIN + r.off[k]
        if dc in (C.LAYOUT, C.DEPENDENT) or (st and st != C.ERR_CHECKSUM and not dc):
            care[lo:lo + r.total[k]] = False
        elif not dc:
            ost, want = O.decompress_frame(C.zoo()[name], verify_checksum=False, js_compat=r.js_exact)
            assert ost == 0
            image[lo:lo + want.size] = want
    return image, care


@pytest.mark.parametrize("js_exact", [False, True], ids=["spec", "js_exact"])
@pytest.mark.parametrize("fill", C.FILLS)
def test_footprint(fill, js_exact):
    r = batch(fill, js_exact)
    image, care = expected_image(r)
    regions = FP.Regions([r.off[k] for k in r.live], [r.total[k] for k in r.live])
    FP.assert_footprint(r.out, image, care, regions, f"frames batch fill {fill:#x} js_exact {js_exact}")
    # frames in error or declined by the index have no slot at all; and the check is not hollow
    assert care.mean() > 0.25 and sum(1 for n in C.NAMES if r.result[n] == (0, 0)) >= 16


def test_capacity_one_byte_short():
    ok = batch(0xFF)
    r = batch(0xFF, short="c65536_isn")
    k = C.NAMES.index("c65536_isn")
    assert r.result["c65536_isn"] == (0, C.OUT_CAP)
    assert {n: v for n, v in r.result.items() if n != "c65536_isn"} == {n: v for n, v in ok.result.items() if n != "c65536_isn"}
    lo = FP.MARGIN + r.off[k]
    assert (r.out[lo:lo + r.total[k]] == r.init[lo:lo + r.total[k]]).all(), "a declined frame's slot was written"
    rest = np.ones(r.out.size, dtype=bool)
    rest[lo:lo + r.total[k]] = False
    image, care = expected_image(ok)
    assert ((r.out == image) | ~care | ~rest).all()
    assert r.finfo[k, 3] == r.total[k]          # still the total the frame needs


def test_content_checksum():
    for fill in C.FILLS:
        r = batch(fill)
        bad = {n for n in C.NAMES if r.result[n][0] == C.ERR_CHECKSUM}
        assert bad == {"csum_flip"}
        assert (frame_bytes(r, "csum_flip") == C.content("five")).all()    # decoded all the same
    # the reference decoder's bytes of the text blocks differ, so they fail the frame's own checksum, as the
    # golden vectors record for the reference
    r = batch(0x00, True)
    assert {n for n in C.NAMES if r.result[n][0] == C.ERR_CHECKSUM} == {"text_isc"}
    assert (frame_bytes(r, "text_isc") != C.text_content()).any()
    assert batch(0x00).result["text_isc"] == (0, 0) and (frame_bytes(batch(0x00), "text_isc") == C.text_content()).all()
    # without the flag nothing is hashed
    for js_exact in (False, True):
        r = batch(0x00, js_exact, verify=False)
        assert not [n for n in C.NAMES if r.result[n][0] == C.ERR_CHECKSUM]
        assert r.result["text_isc"] == (0, 0) and (js_exact or r.result["csum_flip"] == (0, 0))


# --------------------------------------------------------------------------------------------- the wrapper
@pytest.mark.parametrize("js_exact", [False, True], ids=["spec", "js_exact"])
def test_wrapper_over_the_zoo(js_exact):
    from lz4mi import frame as F
    frames = [dev(C.zoo()[n]) for n in C.NAMES]
    rep = {}
    res = F.decompress_frames_device(frames, js_exact=js_exact, report=rep, return_errors=True)
    assert rep["index_calls"] == 1
    for k, name in enumerate(C.NAMES):
        ast, abytes, route = alone(name, js_exact)
        if ast:
            assert isinstance(res[k], lz4mi.Lz4miError) and res[k].status == ast and res[k].frame_index == k, name
        else:
            assert (res[k].cpu().numpy() == abytes).all() and res[k].numel() == abytes.size, name
        want = C.expected_batch(name, js_exact)
        assert rep["declined"][k] == want[1], name
        assert rep["routes"][k] == ("batch" if not want[1] else route), name
    assert {n for n, rt in zip(C.NAMES, rep["routes"]) if rt == "batch"} == \
        {n for n in C.NAMES if not C.expected_batch(n, js_exact)[1]}
    # batch frames are views of one allocation at 16-byte-aligned offsets
    views = [res[k] for k, rt in enumerate(rep["routes"]) if rt == "batch" and not isinstance(res[k], Exception)]
    assert len({v.untyped_storage().data_ptr() for v in views}) == 1 and all(v.data_ptr() % 16 == 0 for v in views)
    # the first failing frame raises, with its index
    first = next(k for k, x in enumerate(res) if isinstance(x, Exception))
    with pytest.raises(lz4mi.Lz4miError) as e:
        F.decompress_frames_device(frames, js_exact=js_exact)
    assert e.value.frame_index == first and e.value.status == res[first].status


def test_wrapper_offsets_form_measure_and_cap_retry():
    from lz4mi import frame as F
    arena, d_off, d_ln = dev_arena(0xFF)
    _, off, ln = C.arena(0xFF)
    rep = {}
    res = F.decompress_frames_device(arena, offsets=off.tolist(), lengths=ln.tolist(), report=rep, return_errors=True,
                                     measure=True, cap_blocks=3)
    assert rep["index_calls"] == 2          # the guess was forced low: once more with the exact need
    k = C.NAMES.index("partial_sized")
    assert rep["routes"][k] == "batch" and (res[k].cpu().numpy() == C.partial_content()).all()
    for k, name in enumerate(C.NAMES):
        ast, abytes, _ = alone(name, False)
        if ast:
            assert isinstance(res[k], lz4mi.Lz4miError) and res[k].status == ast, name
        else:
            assert (res[k].cpu().numpy() == abytes).all(), name


def test_1025_frames_through_the_wrapper_synchronise_three_times_at_most(monkeypatch):
    from lz4mi import frame as F
    torch = torch_()
    n = 1025
    tiny = C.tiny_frames(n)
    frames = [dev(f) for f in tiny[:4]]
    frames = [frames[k % 4] for k in range(n)]
    torch.cuda.synchronize()
    count = {"n": 0}

    def counted(fn):
        def wrapper(*a, **kw):
            count["n"] += 1
            return fn(*a, **kw)
        return wrapper

    monkeypatch.setattr(torch.Tensor, "cpu", counted(torch.Tensor.cpu))
    monkeypatch.setattr(torch.Tensor, "item", counted(torch.Tensor.item))
    monkeypatch.setattr(torch.Tensor, "tolist", counted(torch.Tensor.tolist))
    monkeypatch.setattr(torch.cuda.Stream, "synchronize", counted(torch.cuda.Stream.synchronize))
    monkeypatch.setattr(torch.cuda, "synchronize", counted(torch.cuda.synchronize))
    rep = {}
    res = F.decompress_frames_device(frames, report=rep)
    used = count["n"]
    monkeypatch.undo()
    assert used <= 3, used
    assert rep["routes"] == ["batch"] * n and rep["index_calls"] == 1
    got = torch.cat(res).cpu().numpy()
    assert got.tolist() == [k % 4 for k in range(n)]
