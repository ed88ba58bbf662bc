"""The footprint model (tests/footprint_common.py) without a GPU: the claims of its block table by
the oracle alone, the conditions the GPU batches have to meet, the same arenas through the host
codec (which claims the reference's bytes, partial output included), and assert_footprint itself."""
import re

import numpy as np
import pytest

import oracle as O
import footprint_common as F

lz4mi = pytest.importorskip("lz4mi")

SMALL_BLOCKS = 192        # lz4mi.SMALL_BLOCKS without the environment


def _routes():
    """name -> the decode batches of tests/test_gpu_footprint.py."""
    r = {}
    for mode in ("spec", "js_exact"):
        for size in (3, 7):
            r[f"small{size}_{mode}"] = F.batches(size, mode, False)
        r[f"batch_{mode}"] = F.batches(SMALL_BLOCKS + 8, mode)
    for mode in ("spec", "js_exact", "js_compat"):
        r[f"lone_{mode}"] = F.lone_batches(mode)
    r["compat4"] = F.batches(4, "js_compat", False)
    for mode in F.LINKED_MODES:
        r[mode] = tuple(F.linked_batch(w, mode) for w in ("ok", "fail"))
    return r


def _expected(b, run=0):
    return F.expected_image(b.out_arena(run), b.pays, (b.offs, b.caps), b.mode, b.dictionary, b.stored)


def test_table_claims():
    """Per block and capacity, decoded at out_off 333 of a patterned array: blocks with final
    literals fail below N (Output Buffer Too Small) having written [0, min(cap, ...)) at most; blocks
    that end on their match give status 0 with out_len = N > cap, clipped at the capacity; nothing
    outside [off, off + cap) changes in any mode."""
    off = 333
    for r, cap in F.pairs(stored=False):
        for js in (False, True):
            init = F.pattern(off + cap + 500, 0)
            st, w, res = O.decompress_block(r.comp, cap, out=init[:off + cap].copy(), out_off=off, js_compat=js)
            assert np.array_equal(res[:off], init[:off]), (r.name, cap, js)
            if r.name.startswith("err_"):
                want = {"err_offset0_at_64": F.OFFSET0, "err_malformed_and_offset0": F.MALFORMED,
                        "err_far_at_64": F.DICT_OOB}           # (40 000 below a block at 333)
                assert st == want[r.name], (r.name, st)
                continue
            if cap >= r.n:
                assert st == 0 and w == r.n, (r.name, cap, st, w)
                assert np.array_equal(res[off + r.n:], init[off + r.n:off + cap]), (r.name, cap, "tail")
            elif r.ends_on_match:
                assert r.match[0] < cap < r.match[1]
                assert st == 0 and w == r.n > cap, (r.name, cap, st, w)
            else:
                assert st == F.TOO_SMALL, (r.name, cap, st)
    # spec and reference bytes differ where the table says the rewrite is
    t = F.table()
    for name in ("f1_mid", "f1_cut"):
        a = O.decompress_block(t[name].comp, t[name].n)[2]
        b = O.decompress_block(t[name].comp, t[name].n, js_compat=True)[2]
        assert not np.array_equal(a, b), name
    assert t["per_long_1"].n >= 32 * t["per_long_1"].comp.size


def test_rewrite_below_the_slot_and_history():
    """f1_first at out_off 300: the reference modes change bytes of out[297 .. 300) and nothing else
    outside the slot, spec mode changes nothing there; hist reads the caller's bytes, the dictionary,
    or fails with Dictionary Offset Out of Bounds."""
    t = F.table()
    for mode in ("spec", "js_exact", "js_compat"):
        b = F.Batch("f1", [t["f1_first"].comp], [t["f1_first"].n], mode=mode, first=300)
        image, care, st, ln = _expected(b)
        assert st == [0] and care.all()
        init = b.out_arena(0)
        diff = np.nonzero(image[:F.MARGIN + 300] != init[:F.MARGIN + 300])[0] - F.MARGIN
        if mode == "spec":
            assert diff.size == 0
        else:
            assert diff.size and set(diff.tolist()) <= {297, 298, 299}, diff
        assert np.array_equal(image[F.MARGIN + 300 + b.caps[0]:], init[F.MARGIN + 300 + b.caps[0]:])
    h = t["hist"]
    d = t["dict_spill"].dictionary
    got = {}
    for first in (0, 3, 300):
        for dictionary in (None, d):
            b = F.Batch("h", [h.comp], [h.n], first=first, dictionary=dictionary)
            got[first, dictionary is not None] = _expected(b)[2][0]
    assert got == {(0, False): F.DICT_OOB, (0, True): 0, (3, False): F.DICT_OOB, (3, True): 0, (300, False): 0,
                   (300, True): 0}
    image, care, st, ln = _expected(F.Batch("hh", [h.comp] * 2, [h.n] * 2))
    assert st == [F.DICT_OOB, F.CROSS]                 # below out[0]; inside `out` but below the block


def test_conditions_on_the_gpu_batches():
    """Conditions on the inputs of tests/test_gpu_footprint.py: don't-care bytes are at most a quarter
    of a batch's slot bytes; failing blocks are never adjacent and at most a third of a batch (batch
    kernel and small path); every row of the table with a status-0 capacity has one in every route;
    every failing status occurs; the layouts have the odd offsets and the page-crossing slot."""
    routes = _routes()
    seen = set()
    for name, bs in routes.items():
        ok_rows = set()
        for b in bs:
            image, care, st, ln = _expected(b)
            seen |= {x for s in st for x in (s if isinstance(s, tuple) else (s,))}
            assert float((~care).sum()) <= 0.25 * sum(b.caps) or b.n == 1, (name, b.name)
            assert all(o0 + c0 <= o1 for o0, c0, o1 in zip(b.offs, b.caps, b.offs[1:])), b.name
            if name.startswith(("small", "batch", "compat")):
                bad = [s != 0 for s in st]
                assert not any(x and y for x, y in zip(bad, bad[1:])) and 3 * sum(bad) <= b.n, (name, b.name)
                assert b.n == 1 or b.offs[1] % 4096 == 4095
                assert {o % 16 for o in b.offs} <= {1, 5, 15} and all(o % 2 for o in b.in_offs)
            ok_rows |= {p.tobytes() for p, s in zip(b.pays, st) if s == 0}
        if name.startswith(("small", "batch", "lone", "compat")):
            for r in F.table().values():
                if r.name.startswith("err_") or r.name == "stored_over":
                    continue
                if (r.lone_only and not name.startswith("lone")) or (r.stored and "compat" in name):
                    continue
                assert r.comp.tobytes() in ok_rows, (name, r.name)
        if name.startswith("batch"):
            assert len(bs) >= 1 and all(b.n == SMALL_BLOCKS + 8 for b in bs), name
            want = {(r.name, c) for r, c in F.pairs()}
            have = {(p.tobytes(), c) for b in bs for p, c in zip(b.pays, b.caps)}
            assert all((F.table()[n].comp.tobytes(), c) in have for n, c in want), name
    assert {0, F.TOO_SMALL, F.MALFORMED, F.OFFSET0, F.DICT_OOB, F.CROSS, F.RANGE} <= seen, seen
    # the linked cases: a guard in front of every slot but block 3's, whose rewrite lands in block 2
    c = F.linked_cases()["ok"]
    gaps = [o1 - (o0 + c0) for o0, c0, o1 in zip(c["offs"], c["caps"], c["offs"][1:])]
    assert gaps[2] == 0 and all(g >= F.GUARD for k, g in enumerate(gaps) if k != 2), gaps
    for mode in F.LINKED_MODES:
        image, care, st, ln = _expected(F.linked_batch("ok", mode))
        assert st == [0] * 5 and ln == [65536] * 5 and care.all(), (mode, st, ln)
        b = F.linked_batch("fail", mode)
        image2, care2, st, ln = _expected(b)
        assert st == [0, 0, F.TOO_SMALL, F.CROSS, F.CROSS] and ln == [65536, 65536, 0, 0, 0], (mode, st, ln)
        lo = F.MARGIN + b.offs[2] + b.caps[2]
        assert np.array_equal(image2[lo:], b.out_arena(0)[lo:]) and care2[lo:].all()
    spec = _expected(F.linked_batch("ok", "linked"))[0]
    exact = _expected(F.linked_batch("ok", "linked_exact"))[0]
    o3 = F.MARGIN + c["offs"][3]
    assert not np.array_equal(spec[o3 - 8:o3], exact[o3 - 8:o3])      # block 3's rewrite below its own slot


@pytest.mark.parametrize("mode", ["spec", "js_exact"])
def test_host_decoder_footprint(mode):
    """The batches of the small path and every lone case through the host decoder, one call per
    block on the caller's arena: the whole array equals the oracle's, partial output included."""
    lone = F.lone_batches(mode)
    special = tuple(b for b in lone if b.name.startswith(("lone_f1_", "lone_hist", "lone_dict")))
    for b in F.batches(7, mode, False)[::2] + lone[::3] + special:
        if any(b.stored):
            continue
        F.check_batch(b, lambda batch, run: F.host_decode(lz4mi, batch, run), all_care=True)


def _host_encode(batch, run):
    out, inp = batch.out_arena(run), batch.in_arena(run)
    lens = []
    for ioff, off, s in zip(batch.in_offs, batch.offs, batch.srcs):
        table = np.zeros(16384, dtype=np.int32)
        lens.append(lz4mi.host_compress_raw(inp, out, F.MARGIN + ioff, s.size, table, F.MARGIN + off))
    return out, lens


def test_host_encoder_footprint():
    """The encoder's arenas through the host encoder: the compressed bytes and nothing else."""
    b = F.encoder_batch(20)
    for run in (0, 1):
        image, lens = b.expected(run)
        got, glens = _host_encode(b, run)
        assert glens == lens
        F.assert_footprint(got, image, np.ones(image.size, dtype=bool), F.Regions(b.offs, b.bounds, lens), f"run {run}")
    assert F.encoder_batch(770).n == 770


def test_assert_footprint_names_the_region():
    b = F.batches(7, "spec", False)[0]
    image, care, st, ln = _expected(b)
    reg = F.Regions(b.offs, b.caps, ln)
    k = next(j for j in range(b.n) if st[j] == 0 and ln[j] < b.caps[j])
    bad = next(j for j in range(b.n) if st[j] != 0)
    plant = {F.MARGIN - 1: "margin below out[0]", F.MARGIN + b.offs[1] - 1: "guard before slot 1",
             F.MARGIN + b.offs[k] + b.caps[k] - 1: f"slot {k} tail", F.MARGIN + b.offs[k]: f"slot {k} head",
             F.MARGIN + b.offs[k] + 20: f"slot {k} body", image.size - 1: "margin after the last slot"}
    F.assert_footprint(image.copy(), image, care, reg)
    for pos, region in plant.items():
        got = image.copy()
        got[pos] ^= 1
        with pytest.raises(AssertionError, match=re.escape(f"position {pos} ") + ".*" + re.escape(f"in {region}: got")):
            F.assert_footprint(got, image, care, reg)
    got = image.copy()
    got[F.MARGIN + b.offs[bad] + 1] ^= 1                 # a failing block's own slot: not compared
    F.assert_footprint(got, image, care, reg)
    sent = np.full(b.n + F.SENTINELS, F.FILL, dtype=np.int32)
    sent[:b.n] = 0
    F.assert_sentinels(sent, b.n)
    sent[b.n] = 0
    with pytest.raises(AssertionError, match=f"sentinel entry {b.n} "):
        F.assert_sentinels(sent, b.n)
