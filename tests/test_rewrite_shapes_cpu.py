"""The built rewrite shapes of tests/rewrite_shapes_common.py without a GPU: every shape is what it says
(claims(), on the oracle alone), the oracle's reference-mode decode reproduces what the reference's own
decompressBlock left on the same inputs (tests/golden/rewrite_shapes.json, digests recorded by
tools/golden/gen_rewrite_shapes.mjs), and the host decoder equals the oracle in spec and in reference mode
over the whole array, the bytes below the slot included."""
import json
import os

import numpy as np
import pytest

import rewrite_shapes_common as X
from conftest import GOLDEN


def test_shapes_are_what_they_claim():
    counts = X.claims()
    assert set(counts) == set(X.FAMILIES)
    assert sum(n for n, _, _, _ in counts.values()) == len(X.shapes())
    for fam in ("chain", "rewrite_of_rewrite", "periodic", "wave_match", "dense", "rows", "chunk_edge", "cut", "segment",
                "clipped", "history"):
        assert counts[fam][2] > 0, fam
    assert counts["no_change"][2] == 0 and counts["history"][3] == 22


def test_reference_pin():
    """A block digest that differs means the builders' random streams changed: regenerate the fixture; it never
    counts against the oracle."""
    with open(os.path.join(GOLDEN, "rewrite_shapes.json")) as f:
        pinned = json.load(f)["shapes"]
    assert list(pinned) == [s.name for s in X.shapes()], \
        "the shape list changed: regenerate tests/golden/rewrite_shapes.json (tools/golden/gen_rewrite_shapes.mjs)"
    for s in X.shapes():
        got, want = X.digests(s), pinned[s.name]
        assert got[0] == want[0], (f"{s.name}: the built block is not the one the fixture was recorded from: regenerate "
                                   "tests/golden/rewrite_shapes.json (tools/golden/gen_rewrite_shapes.mjs)")
        assert got[1] == want[1], (s.name, "bytes written or the error", got[1], want[1])
        assert got[2] == want[2], (s.name, "the array the reference leaves")


@pytest.mark.parametrize("exact", X.MODES, ids=["spec", "reference"])
def test_host_decoder(exact):
    """lz4mi_host_decompress_block on the array with the history and with the dictionary: status, bytes written
    and the whole array == the oracle's."""
    lz4mi = pytest.importorskip("lz4mi")
    for s in X.shapes():
        st, w, want = X.expected(s.name, exact, None, 0x5A)
        arr = X.array_for(s, fill=0x5A)
        try:
            got = (0, lz4mi.host_decompress_raw(s.comp, 0, s.comp.size, arr, X.out_off(s), dictionary=s.dictionary,
                                                spec=not exact))
        except lz4mi.Lz4miError as e:
            got = (e.status, 0)
        assert got == (st, w), (s.name, exact, got, (st, w))
        bad = np.nonzero(arr != want)[0]
        assert bad.size == 0, (s.name, exact, f"{bad.size} bytes differ, first at {int(bad[0])} (slot at {X.out_off(s)})")
