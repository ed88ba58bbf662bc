"""The device-pointer entry points with offsets beyond 4 GiB and with blocks across the 2^32 boundary
(tests/high_offsets_common.py has the arena, the placements and the cases; tests/test_high_offsets_cpu.py checks the
placement arithmetic and the expectations without a GPU).

Two arenas of 2^32 + 128 MiB bytes live on the device for the module, one for inputs and one for outputs. Every case
runs at LOW (the control), HIGH and the cross() placements its entry point names; the expected values are the
oracle's, the same at every placement. After each call the windows are compared with the expected images, then reset,
and the whole arena must hold the fill byte again: a store through an offset that lost its upper half is reported as
the alias of the slot it was meant for. Entry points: lz4mi_xxh32_blocks, lz4mi_verify_blocks, lz4mi_decoded_sizes,
lz4mi_decompress_blocks (small path, batch kernel, LZ4MI_JS_EXACT, a lone block with history, a dictionary,
LZ4MI_LINKED and LZ4MI_LINKED_EXACT with the span limit of a linked window), lz4mi_compress_blocks,
lz4mi_frames_index / lz4mi_frames_decompress and lz4mi_frames_plan / lz4mi_frames_compress.

Left out: LZ4MI_FRAMES_PACKED, which starts at position 0 of `out` by contract and so has no offset to move (`work`
keeps the plan's offsets for the same reason: the caller cannot place them); lz4mi_compress_chain and
lz4mi_frame_decompress, which take no offset arrays; lz4mi_generate_blocks, which the benchmark's batch covers. The
span-limit case whose lowest slot lies above 2^32 needs a second slot 2^30 higher and gets an arena of its own
(2^32 + 2^30 + 128 MiB) on the spread side.
"""
import numpy as np
import pytest

import footprint_common as FP
import frames_chain_common as CH
import frames_common as FC
import high_offsets_common as H
import lz4mi
import sizes_common as SZ
from test_gpu_frames_batch import Lists as IndexLists
from test_gpu_frames_compress import compress_dev, plan_dev

pytestmark = pytest.mark.gpu
SENT = FP.SENTINELS
NEED_FREE = 12 << 30


def torch_():
    import torch
    return torch


HOLD = []      # every array a call is given stays allocated until run() has synchronised: the calls are asynchronous


def dev(a, dt=np.int64):
    HOLD.append(torch_().from_numpy(np.ascontiguousarray(np.asarray(a).astype(dt))).cuda())
    return HOLD[-1]


def words32(a):
    return dev(np.asarray(a, dtype=np.uint32).view(np.int32), np.int32)


def sentinels(n):
    t = torch_()
    HOLD.append(t.full((n + SENT,), FP.FILL, dtype=t.int32, device="cuda"))
    return HOLD[-1]


@pytest.fixture(scope="module")
def arenas():
    t = torch_()
    lz4mi.init(0)
    free, _ = t.cuda.mem_get_info()
    if free < NEED_FREE:
        pytest.skip(f"{free >> 30} GiB of device memory free, the two arenas and the cases need 12")
    pair = [H.Arena(t), H.Arena(t)]
    for a in pair:
        a.fill(H.FILL)
    yield pair
    del pair[:]
    t.cuda.empty_cache()


@pytest.fixture(scope="module")
def span_arena(arenas):
    """One arena long enough for a slot 2^30 above a slot that lies above 2^32, allocated when first asked for."""
    t = torch_()
    box = []

    def get():
        if not box:
            free, _ = t.cuda.mem_get_info()
            if free < H.SPAN_ARENA + (1 << 30):
                pytest.skip(f"{free >> 30} GiB of device memory free, the span arena needs {H.SPAN_ARENA >> 30} more")
            box.append(H.Arena(t, H.SPAN_ARENA))
            box[0].fill(H.FILL)
        return box[0]
    yield get
    del box[:]
    t.cuda.empty_cache()


class Ptr:
    def __init__(self, p):
        self.p = p

    def data_ptr(self):
        return self.p


def run(pair, case, places, call, what, fill=H.FILL, sides=None):
    """Loads the case's windows at the placements, makes the call(s), and settles both arenas: the input windows must
    be unchanged and the rest of both arenas untouched. -> (call's result, the output windows, placed in, placed out)."""
    ain, aout = pair
    inp, out = sides or (case.inp, case.out)
    ain.fill(fill)
    aout.fill(fill)
    pi = H.Placed(inp, places[0])
    po = H.Placed(out, places[1]) if out is not None else None
    what = f"{what} [{H.pair_id(places) if po else H.place_id(places[0])}]"
    try:
        ain.load(pi)
        if po:
            aout.load(po)
        res = call(ain.ptr, pi, aout.ptr, po)
        torch_().cuda.synchronize()
        got_out = aout.settle(po, what + ", the output arena") if po else None
        got_in = ain.settle(pi, what + ", the input arena")
    finally:
        torch_().cuda.synchronize()
        del HOLD[:]
        ain.abandon()
        aout.abandon()
    for g, (_, d) in zip(got_in, inp.pieces):
        H.assert_image(g, d, None, pi, what + ": the input changed")
    return res, got_out, pi, po


def with_second_fill(places):
    """Every placement on the module's fill, and the HIGH one once more on the second fill."""
    return [(p, H.FILL) for p in places] + [(places[1], H.FILL2)]


def ids(pf):
    p, fill = pf
    name = H.pair_id(p) if isinstance(p[0], tuple) else H.place_id(p)
    return name + ("" if fill == H.FILL else "-fill2")


# ------------------------------------------------------------------------------------------------ XXH32
@pytest.mark.parametrize("pf", with_second_fill(H.XXH_PLACES), ids=ids)
def test_xxh32_blocks(arenas, pf):
    place, fill = pf
    case, datas = H.xxh_case()
    n = len(datas)
    combos = [(seed, std) for std in (False, True) for seed in (0, 12345)]

    def call(in_ptr, pi, _out, _po):
        off, ln = dev(pi.offs()), dev([d.size for d in datas], np.int32)
        res = []
        for seed, std in combos:
            h = sentinels(n)
            lz4mi.xxh32_blocks_dev(in_ptr, off.data_ptr(), ln.data_ptr(), h.data_ptr(), n, seed=seed, standard=std)
            res.append(h)
        return res

    res, _, pi, _ = run(arenas, case, (place, None), call, "xxh32_blocks", fill)
    for (seed, std), h in zip(combos, res):
        h = h.cpu().numpy()
        FP.assert_sentinels(h, n, "hashes[]")
        got, want = h[:n].view(np.uint32).tolist(), H.xxh_expected(datas, seed, std)
        bad = [(case.inp.slots[k][0], got[k], want[k]) for k in range(n) if got[k] != want[k]]
        assert not bad, (H.place_id(place), seed, std, bad[:4])


# ------------------------------------------------------------------------------------ block checksums
@pytest.mark.parametrize("pf", with_second_fill(H.VERIFY_PLACES), ids=ids)
def test_verify_blocks(arenas, pf):
    place, fill = pf
    case, words, stored = H.verify_case()
    n = len(words)
    for name, (side, total, want) in H.verify_variants().items():
        def call(in_ptr, pi, _out, _po):
            off = dev(pi.offs())
            end = pi.D + (side.pieces[0][1].size if total is None else total)
            res = []
            for fw in (True, False):
                st = sentinels(n)
                ln = words32(words if fw else [w & 0x7FFFFFFF for w in words])
                lz4mi.verify_blocks_dev(in_ptr, end, off.data_ptr(), ln.data_ptr(), st.data_ptr(), n, frame_words=fw)
                res.append(st)
            return res

        res, _, pi, _ = run(arenas, case, (place, None), call, f"verify_blocks {name}", fill, sides=(side, None))
        if name == "cut" and place != H.LOW:
            assert pi.D + total > 2 ** 32
        for fw, st in zip((True, False), res):
            st = st.cpu().numpy()
            FP.assert_sentinels(st, n, "status[]")
            assert st[:n].tolist() == want.tolist(), (name, H.place_id(place), fw)


# ------------------------------------------------------------------------------------------------ sizes
@pytest.mark.parametrize("place", (H.LOW, H.HIGH) + H.DECODE_IN_PLACES, ids=H.place_id)
def test_decoded_sizes(arenas, place):
    case, rows = H.decode_case()
    n = len(rows)
    want = [SZ.walk(c) for _, c, _ in rows]

    def call(in_ptr, pi, _out, _po):
        off = dev(pi.offs())
        res = []
        for fw in (False, True):
            ln, st = sentinels(n), sentinels(n)
            # (with frame words block 2 is passed as a stored block: its size is its payload's length)
            w = [c.size | (0x80000000 if fw and j == 2 else 0) for j, (_, c, _) in enumerate(rows)]
            lz4mi.decoded_sizes_dev(in_ptr, off.data_ptr(), words32(w).data_ptr(), ln.data_ptr(), st.data_ptr(), n,
                                    frame_words=fw)
            res.append((ln, st))
        return res

    res, _, _, _ = run(arenas, case, (place, None), call, "decoded_sizes", sides=(case.inp, None))
    for fw, (ln, st) in zip((False, True), res):
        ln, st = ln.cpu().numpy(), st.cpu().numpy()
        FP.assert_sentinels(ln, n, "out_len[]")
        FP.assert_sentinels(st, n, "status[]")
        exp = list(want)
        if fw:
            exp[2] = (0, rows[2][1].size)
        assert list(zip(st[:n].tolist(), ln[:n].view(np.uint32).tolist())) == exp, (H.place_id(place), fw)


# ----------------------------------------------------------------------------------------------- decode
def decode_call(rows, words=None, **kw):
    n = len(rows)

    def call(in_ptr, pi, out_ptr, po):
        ln, st = sentinels(n), sentinels(n)
        w = words32([c.size for _, c, _ in rows] if words is None else words)
        lz4mi.decompress_blocks_dev(in_ptr, dev(pi.offs()).data_ptr(), w.data_ptr(), out_ptr, dev(po.offs()).data_ptr(),
                                    words32([cap for _, _, cap in rows]).data_ptr(), ln.data_ptr(), st.data_ptr(), n,
                                    torch_().cuda.current_stream().cuda_stream, **kw)
        return ln, st
    return call


def check_status(res, n, status, lens, what):
    ln, st = (x.cpu().numpy() for x in res)
    FP.assert_sentinels(ln, n, what + " out_len[]")
    FP.assert_sentinels(st, n, what + " status[]")
    got = list(zip(st[:n].tolist(), ln[:n].view(np.uint32).tolist()))
    want = list(zip(status, lens))
    bad = [(k, got[k], want[k]) for k in range(n) if got[k] != want[k]]
    assert not bad, (what, "(status, out_len) by block: got, expected", bad[:5])


def param(*head, places, fill=H.FILL):
    name = "-".join([str(h) for h in head] + [H.pair_id(places)] + (["fill2"] if fill != H.FILL else []))
    return pytest.param(*[h[1] if isinstance(h, Named) else h for h in head], places, fill, id=name)


class Named(tuple):
    """(label, value): a parameter shown by its label."""

    def __str__(self):
        return self[0]


def _decode_params():
    out = []
    for nb in (Named(("small", None)), Named(("batch", H.SMALL_BATCH))):
        places = H.decode_places(nb[1])
        for js in (Named(("spec", False)), Named(("js_exact", True))):
            out += [param(nb, js, places=p) for p in places]
        out.append(param(nb, Named(("spec", False)), places=places[1], fill=H.FILL2))
    return out


@pytest.mark.parametrize("nb,js,places,fill", _decode_params())
def test_decompress_blocks(arenas, nb, js, places, fill):
    """The seven blocks through the small path, and repeated to SMALL_BLOCKS + 8 through the batch kernel."""
    case, rows = H.decode_case(nb)
    img, care, status, lens = H.expected_decode(case.out, rows, js)
    what = f"decompress_blocks x{len(rows)} {'js_exact' if js else 'spec'}"
    res, got, _, po = run(arenas, case, places, decode_call(rows, js_exact=js), what, fill)
    check_status(res, len(rows), status, lens, what)
    H.assert_image(got[0], img, care, po, what)


@pytest.mark.parametrize("js", (False, True), ids=("spec", "js_exact"))
@pytest.mark.parametrize("places", H.LONE_PLACES, ids=H.pair_id)
def test_lone_block_reads_the_history_below_its_slot(arenas, js, places):
    case, pay, cap = H.lone_case()
    img, st, w = H.expected_lone(js)
    what = f"lone block {'js_exact' if js else 'spec'}"
    res, got, _, po = run(arenas, case, places, decode_call([("blk", pay, cap)], js_exact=js), what)
    check_status(res, 1, [st], [w], what)
    H.assert_image(got[0], img, None, po, what)


@pytest.mark.parametrize("places", H.DICT_PLACES, ids=H.pair_id)
def test_batch_with_a_dictionary(arenas, places):
    case, rows, d = H.dict_case()
    img, care, status, lens = H.expected_decode(case.out, rows, False)
    d_dict = dev(d, np.uint8)
    res, got, _, po = run(arenas, case, places, decode_call(rows, dict_ptr=d_dict.data_ptr(), dict_len=d.size),
                          "decompress_blocks with a dictionary")
    check_status(res, len(rows), status, lens, "dictionary batch")
    H.assert_image(got[0], img, care, po, "dictionary batch")


# ---------------------------------------------------------------------------------------- linked decode
@pytest.mark.parametrize("mode", (True, "exact"), ids=("linked", "linked_exact"))
@pytest.mark.parametrize("window", (None, 2), ids=("one_window", "window2"))
@pytest.mark.parametrize("pf", with_second_fill(H.LINKED_PLACES), ids=ids)
def test_linked(arenas, mode, window, pf, monkeypatch):
    places, fill = pf
    if window:
        monkeypatch.setenv("LZ4MI_LINKED_WINDOW", str(window))
    case, pays, stored, caps = H.linked_case()
    arr, status, lens = H.expected_linked(mode == "exact")
    rows = [(n, p, c) for (n, _, _), p, c in zip(case.inp.slots, pays, caps)]
    words = [p.size | (0x80000000 if s else 0) for p, s in zip(pays, stored)]
    what = f"linked {mode} window {window}"
    res, got, _, po = run(arenas, case, places, decode_call(rows, words, frame_words=True, linked=mode), what, fill)
    check_status(res, len(rows), status, lens, what)
    H.assert_image(got[0], arr, None, po, what)


@pytest.mark.parametrize("mode", (True, "exact"), ids=("linked", "linked_exact"))
@pytest.mark.parametrize("which", ("in_under", "in_at", "out_under", "out_at"))
@pytest.mark.parametrize("place", (H.LOW, H.HIGH), ids=H.place_id)
def test_linked_span_limit(arenas, span_arena, mode, which, place):
    """Two blocks of one linked call, `in` or `out` spread by just under and by at least 2^30 as
    lz4mi_linked_prep_kernel counts it (include/lz4mi.h, LZ4MI_LINKED): under it both decode, at it the second block
    is LZ4MI_ERR_ARG with out_len 0 and nothing written."""
    case = H.span_case(which)
    r0, r1, raws = H.span_blocks()
    pair = list(arenas)
    if place == H.HIGH:
        pair[0 if which.startswith("in") else 1] = span_arena()
    images, status, lens = H.expected_span(which, mode == "exact")
    what = f"linked span {which} {mode}"
    res, got, _, po = run(pair, case, (place, place), decode_call([r0, r1], linked=mode), what)
    check_status(res, 2, status, lens, what)
    for k, (g, want) in enumerate(zip(got, images)):
        bad = np.nonzero(g != want)[0]
        assert not bad.size, (what, f"slot t{k}: {bad.size} wrong byte(s), first at its byte {int(bad[0]) - H.MARGIN}")


# ---------------------------------------------------------------------------------------- batch encode
@pytest.mark.parametrize("pf", with_second_fill(H.ENCODE_PLACES), ids=ids)
def test_compress_blocks(arenas, pf):
    places, fill = pf
    case, datas = H.encode_case()
    img, lens = H.expected_encode()
    n = len(datas)

    def call(in_ptr, pi, out_ptr, po):
        ln = sentinels(n)
        lz4mi.compress_blocks_dev(in_ptr, dev(pi.offs()).data_ptr(), words32([d.size for d in datas]).data_ptr(), out_ptr,
                                  dev(po.offs()).data_ptr(), ln.data_ptr(), n)
        return ln

    res, got, _, po = run(arenas, case, places, call, "compress_blocks", fill)
    ln = res.cpu().numpy()
    FP.assert_sentinels(ln, n, "out_len[]")
    assert ln[:n].tolist() == lens, H.pair_id(places)
    H.assert_image(got[0], img, None, po, "compress_blocks")


# ---------------------------------------------------------------------------------- frame batch decode
def _frames_params():
    out = []
    for mode in H.FRAMES_MODES:
        out += [param(mode, places=p) for p in H.frames_places(mode)]
    out.append(param("verify_content", places=(H.HIGH, H.HIGH), fill=H.FILL2))
    return out


@pytest.mark.parametrize("mode,places,fill", _frames_params())
def test_frames_decompress(arenas, mode, places, fill):
    """The zoo of tests/frames_common.py: the device index against the host index of the untranslated arena, then the
    statuses, decline codes, bytes written and bytes as tests/test_gpu_frames_batch.py expects them."""
    case, idx, live, total = H.frames_case(mode)
    img, care, want, decoded = H.expected_frames(mode)
    kw = H.FRAMES_MODES[mode]
    js, measure, verify = kw.get("js_exact", False), kw.get("measure", False), kw.get("verify", False)
    nf = len(FC.NAMES)
    _, _, ln = FC.arena(0x00)

    def call(in_ptr, pi, out_ptr, po):
        L = IndexLists(nf, FC.need_blocks())
        lz4mi.frames_index_dev(in_ptr, dev(pi.offs(list(FC.NAMES))).data_ptr(), dev(ln).data_ptr(), nf, L.off.data_ptr(),
                               L.word.data_ptr(), L.frame.data_ptr(), L.size.data_ptr(), L.cap, L.finfo_ptr(),
                               L.totals_ptr(), measure=measure, js_exact=js)
        index = L.host()
        foff, fcap = np.zeros(nf, dtype=np.int64), np.zeros(nf, dtype=np.int64)
        for k in live:
            foff[k], fcap[k] = po.pos(FC.NAMES[k]), total[k]
        lz4mi.frames_decompress_dev(in_ptr, L.off.data_ptr(), L.word.data_ptr(), L.frame.data_ptr(), L.size.data_ptr(),
                                    L.cap, L.finfo_ptr(), nf, out_ptr, dev(foff).data_ptr(), dev(fcap).data_ptr(),
                                    js_exact=js, verify_content=verify)
        torch_().cuda.synchronize()
        return index, L.host()

    what = f"frames batch {mode}"
    (index, after), got, pi, po = run(arenas, case, places, call, what, fill)
    listed = int(idx["totals"][1])
    assert index["totals"].tolist() == idx["totals"].tolist(), what
    assert (index["finfo"] == idx["finfo"]).all(), what
    assert (index["blk_in_off"] - np.uint64(pi.D + H.MARGIN) == idx["blk_in_off"][:listed]).all(), (what, "blk_in_off")
    for key in ("blk_word", "blk_frame", "blk_size"):
        assert (index[key] == idx[key][:listed]).all() and (after[key] == index[key]).all(), (what, key)
    assert (after["blk_in_off"] == index["blk_in_off"]).all()
    fin = after["finfo"]
    result = {n: (int(fin[k, 0]), int(fin[k, 7])) for k, n in enumerate(FC.NAMES)}
    assert result == want, (what, {n: (result[n], want[n]) for n in FC.NAMES if result[n] != want[n]})
    for name, dec in decoded.items():
        k = FC.NAMES.index(name)
        w = int(fin[k, 3])
        if int(fin[k, 2]):      # a content size: at most it, and behind the last byte that is not zero
            nz = np.nonzero(dec)[0]
            assert w <= dec.size and (nz.size == 0 or w > nz[-1]), (what, name, w)
        else:
            assert w == dec.size == total[k], (what, name, w)
    H.assert_image(got[0], img, care, po, what)


# ---------------------------------------------------------------------------------- frame batch encode
def _enc_params():
    out = []
    for kind in H.ENC_KINDS:
        for combo in H.ENC_COMBOS:
            c = Named((CH.combo_id(combo), combo))
            out += [param(kind, c, places=p) for p in H.enc_places(kind, combo)]
    c = Named((CH.combo_id(H.ENC_COMBOS[0]), H.ENC_COMBOS[0]))
    out.append(param("chains", c, places=(H.HIGH, H.HIGH), fill=H.FILL2))
    return out


@pytest.mark.parametrize("kind,combo,places,fill", _enc_params())
def test_frames_compress(arenas, kind, combo, places, fill):
    """Group c64k of tests/frames_chain_common.py into the caller's slots: the plan against the closed form, the
    frames against the oracle's; `work` keeps the plan's offsets."""
    t = torch_()
    case, names, written = H.enc_case(kind, combo)
    img = H.expected_enc_image(kind, combo)
    fl = H.enc_flags(kind, combo)
    need = CH.need_blocks("c64k")
    _, off, ln = CH.arena("c64k", 0x00)
    rows, totals, b_off, b_len, b_frame, b_work = H.expected_plan(kind, combo, [int(o) for o in off],
                                                                  [int(n) for n in ln], need)
    sizes = {n: H.expected_frame(n, kind, combo).size for n in written}

    def call(in_ptr, pi, out_ptr, po):
        L = plan_dev(dev(pi.offs(list(names))), dev(ln), 65536, need, fl)
        plan = L.host()
        work = t.full((int(plan["totals"][3]),), 0xA5, dtype=t.uint8, device="cuda")
        foff = [po.pos(n) if n in sizes else 0 for n in names]
        fcap = [sizes.get(n, 0) for n in names]
        fi = compress_dev(Ptr(in_ptr), L, int(plan["totals"][1]), work, Ptr(out_ptr), arenas[1].size, fl,
                          (dev(foff), dev(fcap)))
        return plan, fi, L.host()

    what = f"frames compress {kind} {CH.combo_id(combo)}"
    (plan, fi, after), got, pi, po = run(arenas, case, places, call, what, fill)
    assert plan["totals"].tolist() == totals and plan["finfo"].tolist() == rows, what
    assert (plan["blk_in_off"] - np.uint64(pi.D + H.MARGIN)).tolist() == b_off, (what, "blk_in_off")
    assert plan["blk_len"].tolist() == b_len and plan["blk_frame"].tolist() == b_frame, what
    assert plan["blk_work_off"].tolist() == b_work, what
    for key in ("blk_in_off", "blk_len", "blk_frame", "blk_work_off"):
        assert (after[key] == plan[key]).all(), (what, key, "the lists are read only")
    for k, n in enumerate(names):
        if n in sizes:
            assert fi[k, 7] == 0 and fi[k, 3] == sizes[n], (what, n, fi[k].tolist())
            assert fi[k, 5] - po.D == case.out.slot(n)[0], (what, n, "finfo[5] minus the placement's shift")
        else:
            assert fi[k, 7] == CH.DEPENDENT, (what, n, fi[k].tolist())
    H.assert_image(got[0], img, None, po, what)
