"""The encoder shapes of tests/enc_shapes_common.py without a GPU: every built case is what its
name says (the builders' claims, decided from the oracle alone), the host encoder -- the route the
JS layer takes for dependent frames -- equals the oracle on all of them, final table included, and
the oracle itself reproduces what the reference's compressBlock gave on the same inputs
(tests/golden/enc_shapes.json, digests recorded by tools/golden/gen_enc_shapes.mjs)."""
import json
import os

import numpy as np
import pytest

import enc_shapes_common as E
from conftest import GOLDEN

FAMILIES = "ABCDEFG"


@pytest.mark.parametrize("fam", FAMILIES)
def test_cases_are_what_they_claim(fam):
    f = E.families()[fam]
    assert len(f.cases) == E.SIZES[fam]
    assert len({c.name for c in f.cases}) == len(f.cases)
    assert callable(f.claim) and f.every
    tags = {c.name: f.claim(c) for c in f.cases}
    for name, t in tags.items():
        assert set(f.every) <= t, (name, sorted(set(f.every) - t))
    for prefix, tag in f.some:
        assert any(tag in t for name, t in tags.items() if name.startswith(prefix)), (prefix, tag)


def test_family_sizes_are_as_listed():
    assert E.SIZES == {"A": len(E.STEPS), "B": 2 * sum(1 for S in E.STEPS if 5 <= S < E.SPEC_W),
                       "C": len(E.EDGE_D) * len(E.EDGE_K) * len(E.EDGE_R), "D": 4,
                       "E": sum(S + 13 for S in E.E_NEED) + 3 * 33, "F": len(E.STARTS), "G": 234}
    assert E.STEPS == (4, 5, 8, 16, 19, 20, 64, 127, 128, 129, 273, 274, 300, 1000)
    assert E.EDGE_D == (65534, 65535, 65536, 65537) and E.CHAIN_BLOCKS == (13, 64, 1000, 4096, 65536)
    assert E.STARTS == (0, 1) + tuple(range(65519, 65554)) + (100000,)
    f = E.families()["F"]
    cats = np.concatenate([E.META[c.name]["cat"] for c in f.cases])
    assert set(cats.tolist()) == set(range(len(E.CATEGORIES)))
    for c in f.cases:      # the categories that need no luck are in every table
        assert (c.table == -(1 << 31)).any() and (c.table == (1 << 31) - 1).any() and (c.table < 0).any()
        assert (c.table > c.start + c.len).any() and (c.table == 0).any()


@pytest.mark.parametrize("fam", FAMILIES)
def test_host_encoder(fam):
    """lz4mi_host_compress_block on every case as one block and lz4mi_host_compress_chain on every
    case with its block size: bytes, return values and all 16384 table slots == the oracle's."""
    lz4mi = pytest.importorskip("lz4mi")
    for c in E.families()[fam].cases:
        (want,), want_t = E.oracle_run(c, None)
        out = np.zeros(lz4mi.compress_bound(c.len) + 7, dtype=np.uint8)
        t = np.zeros(16384, dtype=np.int32) if c.table is None else c.table.copy()
        n = lz4mi.host_compress_raw(c.src, out, c.start, c.len, t, 7)
        assert n == want.size and np.array_equal(out[7:7 + n], want), E.explain(c._replace(block_size=None), 0, out[7:7 + n], want)
        assert not out[:7].any() and np.array_equal(t, want_t), c.name
        blocks, want_t = E.expected(c.name)
        t = np.zeros(16384, dtype=np.int32) if c.table is None else c.table.copy()
        got = lz4mi.compress_chain(c.src, c.start, c.len, c.block_size or max(c.len, 1), t, host=True)
        assert len(got) == (len(blocks) if c.len else 0), c.name
        for b, (g, w) in enumerate(zip(got, blocks)):
            assert np.array_equal(g, w), E.explain(c, b, g, w)
        assert np.array_equal(t, want_t), c.name


def test_reference_pin():
    """Per case the fixture holds the XXH32 of the source and of the initial table, the length of
    each block the reference wrote, the XXH32 over the blocks' XXH32s, and the XXH32 of the
    reference's final table. A source or table digest that differs means the builders' random
    streams changed: regenerate the fixture; it never counts against the encoder."""
    with open(os.path.join(GOLDEN, "enc_shapes.json")) as f:
        pinned = json.load(f)["cases"]
    cases = E.all_cases()
    assert set(pinned) == {c.name for c in cases}, "the case list changed: regenerate tests/golden/enc_shapes.json"
    for c in cases:
        blocks, table = E.expected(c.name)
        got, want = E.digests(c, blocks, table), pinned[c.name]
        assert got[:2] == want[:2], (f"{c.name}: the built source or table is not the one the fixture was recorded "
                                     "from: regenerate tests/golden/enc_shapes.json (tools/golden/gen_enc_shapes.mjs)")
        assert got[2] == want[2], (c.name, "block lengths")
        assert got[3] == want[3], (c.name, "block bytes")
        assert got[4] == want[4], (c.name, "final table")
