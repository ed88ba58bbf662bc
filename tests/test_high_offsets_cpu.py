"""No GPU: what tests/test_gpu_high_offsets.py rests on (tests/high_offsets_common.py). The placement arithmetic of
every case -- D a multiple of 16, 2^32 where cross() says, every window inside the arena, no window on another window
or on the alias of a high one --, the cases' expectations from the oracle alone with each case's claim asserted, and
the host twins (lz4mi_host_verify_blocks, lz4mi_host_frames_index, lz4mi_host_frames_plan / _compress) on arrays of
ARENA zero bytes at a high and a crossed placement, with the process's resident memory watched."""
import numpy as np
import pytest

import frames_chain_common as CH
import frames_common as FC
import footprint_common as FP
import high_offsets_common as H
import lz4mi
import oracle as O
import sizes_common as SZ
from linked_exact_common import parse


@pytest.fixture(scope="module")
def cases():
    return H.all_cases()


def test_every_case_is_placed_where_it_says(cases):
    crossed, names = [], set()
    for case in cases:
        assert case.name not in names
        names.add(case.name)
        assert (H.LOW, H.LOW if case.out is not None else None) in case.places, case.name
        assert (H.HIGH, H.HIGH if case.out is not None else None) in case.places, case.name
        for pin, pout in case.places:
            for side, place in ((case.inp, pin), (case.out, pout)):
                if side is None:
                    assert place is None
                    continue
                pl = H.Placed(side, place)
                p = H.check_placed(pl, case.size)
                if place[0] == "cross":
                    crossed.append((case.name, place, p, side.slot(place[1])[1]))
    # every entry point has a crossed run, and the `start` / `end` crossings are exact
    for prefix in ("xxh32", "verify_blocks", "decode7", f"decode{H.SMALL_BATCH}", "decode_lone", "linked", "encode",
                   "frames_default", "frames_verify_content", "frames_enc_chains", "frames_enc_independent"):
        assert any(n.startswith(prefix) for n, _, _, _ in crossed), prefix
    for name, place, p, size in crossed:
        if place[2] == "start":
            assert p == 0, (name, place, p)
        if place[2] == "end":
            assert p == size, (name, place, p)


def test_cross_at_and_helpers():
    assert H.ARENA == 2 ** 32 + (128 << 20) and H.alias(2 ** 32 + 5) == 5
    assert H.window(70000, 100) == (70000 - FP.MARGIN, 100 + 2 * FP.MARGIN)
    (pos, img), offs = H.translate(np.zeros(4, dtype=np.uint8), [1, 2], H.HIGH_D)
    assert pos == H.HIGH_D and offs == [H.HIGH_D + 1, H.HIGH_D + 2]
    for off in range(0, 48):
        for size in (64, 65, 70000):
            for where in H.WHERE:
                p = H.cross_at(off, size, where)
                assert (off + p) % 16 == 0 and 0 <= p <= size
                if where in ("byte1", "mid"):
                    assert 0 < p < size
    assert H.cross_at(32, 70000, "start") == 0 and H.cross_at(32, 70000, "end") == 70000
    assert H.cross_at(47, 70000, "byte1") == 1 and H.cross_at(32, 70000, "byte1") == 16
    assert (H.pattern(300, 7) == FP.pattern(307, 0)[7:]).all()
    side = H.Side.image(np.zeros(200000, dtype=np.uint8), [("a", 70000, 1000)])
    pl = H.Placed(side, H.HIGH)
    assert "alias of slot a (its byte 3" in pl.describe(H.HIGH_D + 70003 - 2 ** 32)
    assert "alias of the window" in pl.describe(H.HIGH_D - 2 ** 32 + 5)
    assert "outside every window" in pl.describe(2 ** 31)


# --------------------------------------------------------------------------------------- the oracle's expectations
def _max_offset(comp):
    return max((off for _, _, off, _ in parse(comp)), default=0)


def test_decode_blocks_are_what_they_claim():
    rows = {n: (c, cap) for n, c, cap in H.decode_blocks()}
    assert list(rows) == ["empty", "n13", "rand5000", "text70000", "tiles216", "clean", "dict_oob"]
    for name, want in (("empty", (0, 0)), ("n13", (0, 13)), ("rand5000", (0, 5000)), ("text70000", (0, 70000)),
                       ("tiles216", (0, 300000)), ("clean", (0, rows["clean"][1])), ("dict_oob", (H.DICT_OOB, None))):
        comp, cap = rows[name]
        for js in (False, True):
            st, w, _ = O.decompress_block(comp, cap, js_compat=js)
            assert st == want[0] and (st != 0 or w == want[1]), (name, js, st, w)
        if want[0] == 0:
            assert SZ.walk(comp) == want, name
            assert not FP.reads_below(comp), name
    # literal-only blocks; the tiles216 block has a match at a distance above 60000 and many parse chunks
    for name in ("n13", "rand5000"):
        assert [off for _, _, off, _ in parse(rows[name][0])] == [0], name
    assert _max_offset(rows["tiles216"][0]) > 60000 and rows["tiles216"][0].size > 20 * 1024
    assert rows["text70000"][0].size > 20 * 1024
    # the batch forms: statuses from the oracle alone, the failing block ERR_CROSS_BLOCK in a batch
    for nb in (None, H.SMALL_BATCH):
        case, brows = H.decode_case(nb)
        assert len(brows) == (nb or 7) and (nb or 7) > (0 if nb is None else lz4mi.SMALL_BLOCKS)
        for js in (False, True):
            img, care, st, ln = H.expected_decode(case.out, brows, js)
            assert st[:7] == [0, 0, 0, 0, 0, 0, H.CROSS] and ln[:7] == [0, 13, 5000, 70000, 300000, rows["clean"][1], 0]
            assert care.mean() > 0.9
    case, brows, d = H.dict_case()
    assert H.expected_decode(case.out, brows, False)[2] == [0, 0, 0, 0, 0, 0, H.CROSS, H.CROSS] and d.size == 400


def test_lone_and_linked_blocks_are_what_they_claim():
    CH.shapes()
    case, pay, cap = H.lone_case()
    assert O.decompress_block(pay, cap)[0] == H.DICT_OOB          # alone, without the history, it cannot decode
    for js in (False, True):
        img, st, w = H.expected_lone(js)
        off = case.out.slot("blk")[0]
        assert st == 0 and w == cap == 65536
        if not js:
            assert (img[off:off + cap] == CH.content("text4")[65536:131072]).all()
            assert (img[:off] == case.out.pieces[0][1][:off]).all()
    case, pays, stored, caps = H.linked_case()
    assert stored == [False] * 4 + [True, False, False] and caps == [65536] * 3 + [100] + [65536, 65536, 5000]
    offs = [o for _, o, _ in case.out.slots]
    assert all(offs[k + 1] == offs[k] + caps[k] for k in (0, 1, 2, 4, 5)) and offs[4] > offs[3] + caps[3]
    arr, st, ln = H.expected_linked(False)
    assert st == [0] * 7 and ln == caps
    assert (arr[offs[0]:offs[0] + 3 * 65536 + 100] == CH.content("text4")).all()
    assert (arr[offs[4]:offs[4] + 131072 + 5000] == CH.content("randtail")).all()
    exact, st, ln = H.expected_linked(True)
    assert st == [0] * 7 and ln == caps and (exact != arr).any()      # the reference's tail rewrite shows in the text
    # every block after a frame's first reaches into the block before it
    for k in (1, 2, 5):
        lit, off = CH.first_match(pays[k])
        assert off > lit, k


def test_span_layouts_sit_on_both_sides_of_the_limit():
    r0, r1, raws = H.span_blocks()
    for row, raw in zip((r0, r1), raws):
        st, w, out = O.decompress_block(row[1], row[2])
        assert st == 0 and w == 5000 and (out[:w] == raw).all()
    lay = H.span_layouts()
    for which, (ins, outs) in lay.items():
        in_span = ins[1] - ins[0] + r1[1].size
        out_span = outs[1] - outs[0] + r1[2] + 65536
        assert (in_span >= H.SPAN) == (which == "in_at") and (out_span >= H.SPAN) == (which == "out_at"), which
    for which in lay:
        for exact in (False, True):
            images, st, ln = H.expected_span(which, exact)
            refused = which.endswith("_at")
            assert st == [0, H.ERR_ARG if refused else 0] and ln == [5000, 0 if refused else 5000]
            assert exact or (images[0][H.MARGIN:H.MARGIN + 5000] == raws[0]).all()
            if refused:
                assert (images[1] == H.span_case(which).out.pieces[1][1]).all()      # nothing written
    assert lay["in_at"][0][1] - lay["in_under"][0][1] == 1 and lay["out_at"][1][1] - lay["out_under"][1][1] == 1
    assert H.SPAN == 2 ** 30


def test_verify_records_are_what_they_claim():
    CH.shapes()
    case, words, stored = H.verify_case()
    assert stored == [False] * 4 + [True, False, False]
    var = H.verify_variants()
    assert not var["clean"][2].any()
    k = [n for n, _, _ in case.inp.slots].index(H.VERIFY_DAMAGED)
    assert var["damaged"][2].tolist() == [H.BAD_SUM if j == k else 0 for j in range(7)]
    side, total, want = var["cut"]
    o, n = side.slots[-1][1:]
    assert o + n < total < o + n + 4 and want.tolist() == [0] * 6 + [H.BAD_SUM]       # the cut record is really cut
    for name in ("text4_b1", "randtail_b0"):
        o, n = side.slot(name)
        assert (o + n) % 16 == 0
        pl = H.Placed(side, H.cross(name, "end"))
        assert pl.D + o + n == 2 ** 32      # 2^32 lies between the payload and its checksum word
    assert H.Placed(side, H.HIGH).D + total > 2 ** 32


def test_xxh_encode_and_frame_expectations():
    case, datas = H.xxh_case()
    assert [d.size for d in datas] == [n for n in H.XXH_LENS for _ in range(4)]
    assert [o % 4 for _, o, _ in case.inp.slots] == [0, 1, 2, 3] * len(H.XXH_LENS)
    assert H.xxh_expected(datas[-4:], 0, False) != H.xxh_expected(datas[-4:], 0, True)      # the two convergences
    assert H.xxh_expected(datas[-4:], 0, False) != H.xxh_expected(datas[-4:], 12345, False)
    case, datas = H.encode_case()
    img, lens = H.expected_encode()
    assert [d.size for d in datas] == [13, 5000, 65537, 300000] * 2 + [65536]
    assert lens[8] > 65536 and lens[3] < 300000 and lens[0] == 14          # random grows; a 13-byte block is literals
    for d, n, (_, off, _) in zip(datas, lens, case.out.slots):
        st, w, out = O.decompress_block(img[off:off + n], d.size)
        assert st == 0 and w == d.size and (out[:w] == d).all()
    o, s = case.out.slot("text300000")
    assert (o + s) % 16 == 0
    for mode in H.FRAMES_MODES:
        case, idx, live, total = H.frames_case(mode)
        img, care, want, dec = H.expected_frames(mode)
        assert sum(1 for n in FC.NAMES if want[n] == (0, 0)) >= (16 if mode == "js_exact" else 30), mode
        x = H.frames_crossed(mode)
        assert care.mean() > 0.25 and x in dec and len(FC.SHAPES["five" if x == "cfive_isc" else 65537]) > 1
        o, s = case.out.slot(x)
        assert (o + s) % 16 == 0 and want[x] == (0, 0)
    assert H.expected_frames("verify_content")[2]["csum_flip"] == (FC.ERR_CHECKSUM, 0)
    assert H.expected_frames("default")[2]["csum_flip"] == (0, 0)
    for kind in H.ENC_KINDS:
        for combo in H.ENC_COMBOS:
            case, names, written = H.enc_case(kind, combo)
            multi = [n for n in names if len(CH.SHAPES[n]) > 1]
            assert (set(names) - set(written) == set(multi)) if kind == "declining" else written == list(names)
            for n in written:
                st, back = O.decompress_frame(H.expected_frame(n, kind, combo))
                assert st == 0 and (back == CH.content(n)).all(), (kind, combo, n)
    assert CH.content("tiles300k").size > 3 * CH.RING_BYTES
    assert H.enc_case("chains", (True, True, True))[0].inp.slot("text4")[0] % 16 == 0


# --------------------------------------------------------------------------------- host twins at high offsets
def _rss_mib():
    with open("/proc/self/status") as f:
        for line in f:
            if line.startswith("VmRSS:"):
                return int(line.split()[1]) / 1024.0
    raise AssertionError("no VmRSS")


def _zeros():
    """ARENA zero bytes: zero pages, untouched outside the windows a test writes."""
    return np.zeros(H.ARENA, dtype=np.uint8)


def _put(arr, placed):
    for (pos, n), (_, d) in zip(placed.windows(), placed.side.pieces):
        arr[pos:pos + n] = d


def _windows_only(arr, placed, images, what):
    for (pos, n), img in zip(placed.windows(), images):
        H.assert_image(arr[pos:pos + n], img, None, placed, what)


RSS_LIMIT_MIB = 300        # over what the process held before the arrays: "a few hundred MiB" (measured: 66)


def test_host_twins_at_high_offsets(record_property):
    before = _rss_mib()
    peak = before
    # lz4mi_host_verify_blocks
    vcase, words, _ = H.verify_case()
    for place in (H.HIGH, H.cross("text4_b1", "end")):
        for name, (side, total, want) in H.verify_variants().items():
            pl = H.Placed(side, place)
            buf = _zeros()
            _put(buf, pl)
            end = H.ARENA if total is None else pl.D + total
            got = lz4mi.host_verify_blocks(buf[:end], pl.offs(), words, frame_words=True)
            assert got.tolist() == want.tolist(), (place, name)
            peak = max(peak, _rss_mib())
            del buf
    # lz4mi_host_frames_index
    for place in (H.HIGH, H.cross(H.frames_crossed("default"), "mid")):
        case, idx, live, total = H.frames_case("default")
        pl = H.Placed(case.inp, place)
        buf = _zeros()
        _put(buf, pl)
        a, off, ln = FC.arena(0x00)
        got = lz4mi.host_frames_index(buf, pl.offs(), ln, FC.need_blocks())
        listed = int(idx["totals"][1])
        assert got["totals"].tolist() == idx["totals"].tolist() and (got["finfo"] == idx["finfo"]).all(), place
        assert (got["blk_in_off"][:listed] - np.uint64(pl.D + H.MARGIN) == idx["blk_in_off"][:listed]).all(), place
        for key in ("blk_word", "blk_frame", "blk_size"):
            assert (got[key] == idx[key]).all(), (place, key)
        for name in FC.NAMES:
            assert (got["finfo"][FC.NAMES.index(name), 0], got["finfo"][FC.NAMES.index(name), 7]) == \
                FC.expected_index(name), name
        peak = max(peak, _rss_mib())
        del buf
    # lz4mi_host_frames_plan + lz4mi_host_frames_compress
    kind, combo = "chains", (True, True, True)
    case, names, written = H.enc_case(kind, combo)
    fl = H.enc_flags(kind, combo)
    need = CH.need_blocks("c64k")
    _, off, ln = CH.arena("c64k", 0x00)
    for pin, pout in ((H.HIGH, H.HIGH), (H.cross("tiles300k", "mid"), H.cross("text4", "mid"))):
        pi, po = H.Placed(case.inp, pin), H.Placed(case.out, pout)
        src, out = _zeros(), _zeros()
        _put(src, pi)
        _put(out, po)
        plan = lz4mi.host_frames_plan(pi.offs(list(names)), ln, 65536, need, fl)
        rows, totals, b_off, b_len, b_frame, b_work = H.expected_plan(kind, combo, [int(o) for o in off],
                                                                      [int(n) for n in ln], need)
        assert plan["totals"].tolist() == totals and plan["finfo"].tolist() == rows
        assert (plan["blk_in_off"] - np.uint64(pi.D + H.MARGIN)).tolist() == b_off
        assert plan["blk_len"].tolist() == b_len and plan["blk_frame"].tolist() == b_frame
        assert plan["blk_work_off"].tolist() == b_work
        sizes = [H.expected_frame(n, kind, combo).size for n in names]
        fi = lz4mi.host_frames_compress(src, plan, out, fl, slots=(po.offs(list(names)), sizes))
        assert not fi[:, 7].any() and fi[:, 3].tolist() == sizes
        assert (fi[:, 5] - po.D).tolist() == [case.out.slot(n)[0] for n in names]
        _windows_only(out, po, [H.expected_enc_image(kind, combo)], f"host frames {pin} {pout}")
        peak = max(peak, _rss_mib())
        del src, out
    record_property("rss_before_mib", round(before))
    record_property("rss_peak_mib", round(peak))
    print(f"resident memory: {before:.0f} MiB before, {peak:.0f} MiB at most with the arrays")
    assert peak - before < RSS_LIMIT_MIB, (before, peak)
