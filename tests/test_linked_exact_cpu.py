"""LZ4MI_LINKED_EXACT without a GPU: the fixture recorded from the reference itself
(tests/golden/linked_exact.json, tools/golden/gen_linked_exact.mjs) pins the oracle's reference-mode
decoder run in index order on one array -- the expected value of every GPU test of the flag -- and a
NumPy model of the kernels' pointer form equals that decode on the fixture and on a seeded fuzz of
dependent blocks: the exactness argument of DESIGN §4.8 as an executable check."""
import os
import re

import numpy as np
import pytest

import oracle as O
from conftest import ROOT
from linked_exact_common import MESSAGES, dependent_blocks, fixture_cases, in_order, pointer_model

CASES = fixture_cases()


def test_fixture_covers_the_cases():
    names = {c["name"] for c in CASES}
    assert {"ll0_ml4_off8", "ll3_ml4_off8", "ll0_ml7_off9", "ll4_ml4_control", "rewritten_source",
            "pred_overlap_off1", "pred_overlap_off2", "tiny_pred_1", "tiny_pred_2", "tiny_pred_3", "stored_pred",
            "gap", "short_tail", "first_over_history", "first_at_0", "first_at_0_dict"} <= names
    # the rewrite does reach the predecessor: 4 bytes, 1 byte, none in the control
    by = {c["name"]: c for c in CASES}
    for name, want in (("ll0_ml4_off8", 4), ("ll3_ml4_off8", 1), ("ll0_ml7_off9", 1), ("ll4_ml4_control", 0)):
        c = by[name]
        alone = in_order(c["blocks"], c["out_off"], c["out_cap"], c["init"], count=1)[2]
        assert int((alone[:32] != c["after"][:32]).sum()) == want, name


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_oracle_in_order_equals_the_reference(case):
    st, ln, out = in_order(case["blocks"], case["out_off"], case["out_cap"], case["init"], case["dict"], case["stored"])
    want = [r if isinstance(r, int) else MESSAGES[r] for r in case["results"]]
    assert [n if s == 0 else s for s, n in zip(st, ln)] == want
    assert np.array_equal(out, case["after"])


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_pointer_model_equals_the_reference(case):
    assert all(isinstance(r, int) for r in case["results"])
    got = pointer_model(case["blocks"], case["out_off"], case["init"], case["dict"], case["stored"])
    assert np.array_equal(got, case["after"])


def test_pointer_model_fuzz():
    """Dependent blocks of text, copy and runs (the generators whose frames the rewrite changes),
    sizes 1..3000 and ~20 000, one carried table: model == oracle, and the rewrite does cross
    block boundaries in the set."""
    rng = np.random.default_rng(4080)
    crossing = changed = 0
    for t in range(60):
        kind = ("text", "copy", "runs")[t % 3]
        nb = int(rng.integers(2, 7))
        sizes = [int(rng.integers(19000, 21000)) if rng.random() < 0.3 else int(rng.integers(1, 3001)) for _ in range(nb)]
        data = O.generate(kind, int(rng.integers(1, 1000)), sum(sizes))
        pay = dependent_blocks(data, sizes)
        off = np.cumsum([0] + sizes[:-1]).tolist()
        init = rng.integers(0, 256, sum(sizes), dtype=np.uint8)
        st, ln, want = in_order(pay, off, sizes, init)
        assert not any(st) and ln == sizes, t
        got = pointer_model(pay, off, init)
        assert np.array_equal(got, want), (t, kind, sizes)
        changed += int(not np.array_equal(want, data))
        for b in range(1, nb):
            before = in_order(pay, off, sizes, init, count=b)[2]
            crossing += int(not np.array_equal(before[:off[b]], want[:off[b]]))
    assert changed >= 20 and crossing >= 20, (changed, crossing)


def test_real_shape_has_cross_block_rewrites():
    """The GPU suite's smallest real shape (text seed 33, 300 000 bytes, 64 KiB dependent blocks):
    the reference's result differs from the input, and blocks change their predecessor's tail."""
    data = O.generate("text", 33, 300000)
    sizes = [min(65536, 300000 - p) for p in range(0, 300000, 65536)]
    pay = dependent_blocks(data, sizes)
    off = np.cumsum([0] + sizes[:-1]).tolist()
    st, ln, want = in_order(pay, off, sizes, np.zeros(300000, dtype=np.uint8))
    assert not any(st) and int((want != data).sum()) > 0
    st, fo = O.decompress_frame(O.compress_frame(data, None, 65536, False, False, True), js_compat=True)
    assert st == 0 and np.array_equal(fo, want)
    hits = 0
    for b in range(1, len(pay)):
        before = in_order(pay, off, sizes, np.zeros(300000, dtype=np.uint8), count=b)[2]
        hits += int(not np.array_equal(before[off[b] - 4:off[b]], want[off[b] - 4:off[b]]))
    assert hits >= 1
    assert np.array_equal(pointer_model(pay, off, np.zeros(300000, dtype=np.uint8)), want)


def test_flag_value():
    lz4mi = pytest.importorskip("lz4mi")
    with open(os.path.join(ROOT, "include", "lz4mi.h")) as f:
        m = re.search(r"#define\s+LZ4MI_LINKED_EXACT\s+(0x[0-9a-fA-F]+)u", f.read())
    assert m and int(m.group(1), 16) == lz4mi.LINKED_EXACT == 0x100
    assert lz4mi._linked_flag("exact") == lz4mi.LINKED_EXACT and lz4mi._linked_flag(True) == lz4mi.LINKED
    assert lz4mi._linked_flag(False) == 0
