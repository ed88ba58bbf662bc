"""The inputs of tests/test_gpu_chain_blocks.py (tests/chain_blocks_common.py), without a GPU: their claims on the
oracle, the host twin of the index call over the packed arenas, and the builders they share with
tests/test_gpu_seqtable.py and tests/literal_pieces_common.py, whose cases must stay what they were."""
import hashlib

import numpy as np
import pytest

import chain_blocks_common as B
import frames_chains_decode_common as D
import literal_pieces_common as LP
import lz4mi
import test_gpu_seqtable as S

# sha256 over (name, compressed block, capacity) of all_cases(), computed before Maker took a `base`
DIGESTS = {"test_gpu_seqtable": (246, "f35a69ec68a0f644ad72493a9b19c301f2589b84acbb51956f11990b9c5b1e93"),
           "literal_pieces_common": (113, "e7697569141e063efd6bcb9c71771abba4b8ee5ad337992c80e92685af16d211")}
# cases left out of that identity check because their construction needs position - offset < 0 at base 0: none
NOT_COMPARED = ()


def test_claims_hold_on_the_oracle():
    counts = B.claims()
    assert set(counts) == {"boundary", "history_fill", "pieces_after_history", "tiny", "flagged_independent",
                           "rewrite", "errors"}
    for family, (frames, blocks, differ) in counts.items():
        assert frames and blocks > frames and differ, family
    # the reference's bytes differ from the spec's in every family, so a spec decode cannot pass for both modes


@pytest.mark.parametrize("mod", [S, LP], ids=["seqtable", "literal_pieces"])
def test_base_0_cases_are_the_parents(mod):
    h = hashlib.sha256()
    cases = mod.all_cases()
    for name, c in cases.items():
        assert name not in NOT_COMPARED
        h.update(name.encode())
        h.update(c[0].tobytes())
        h.update(str(int(c[1])).encode())
    assert (len(cases), h.hexdigest()) == DIGESTS[mod.__name__]


def test_rebuilt_cases_keep_their_shape_and_change_their_offsets():
    n = 0
    for name, (comp0, comp, size, opts) in B.rebuilt_cases().items():
        assert comp.size == comp0.size, name
        n += int((comp != comp0).any())
    assert n >= len(B.rebuilt_cases()) - len(B.NO_SEQUENCE_BELOW)


@pytest.mark.parametrize("exact", [False, True], ids=["spec", "js_exact"])
@pytest.mark.parametrize("name", B.GROUPS)
def test_host_index_lists_every_block_at_its_size(name, exact):
    frames = B.group(name)
    for fill in D.FILLS:
        a, off, ln = B.arena(name, fill)
        assert [int(o) % 16 for o in off] == [D.RESIDUES[k % 4] for k in range(off.size)]
        # the arena and the output of the call (16-byte-aligned slots, 48 bytes between two) stay under 12 MiB
        assert a.size < 12 << 20 and sum((f.total + 48 + 15) & ~15 for f in frames) < 12 << 20
        cap = sum(len(f.blocks) for f in frames) + 8
        r = lz4mi.host_frames_index(a, off, ln, cap, measure=B.measured(name), js_exact=exact)
        fi = r["finfo"]
        assert not fi[:, 0].any() and not fi[:, 7].any(), [f.name for f, row in zip(frames, fi) if row[0] or row[7]]
        assert r["totals"][0] == r["totals"][1] == cap - 8 and r["totals"][3] == 0
        for k, f in enumerate(frames):
            first, count = int(fi[k, 4]), int(fi[k, 6])
            assert count == len(f.blocks) and fi[k, 2] == fi[k, 3] == f.total, f.name
            assert (fi[k, 1] & 0xFF) == f.data[4] and bool(fi[k, 1] >> 16 & 1) == B.measured(name), f.name
            assert r["blk_size"][first:first + count].tolist() == f.sizes, f.name
            assert (r["blk_frame"][first:first + count] == k).all(), f.name
            words = [p.size | (0x80000000 if st else 0) for p, st in f.blocks]
            assert r["blk_word"][first:first + count].tolist() == words, f.name


def test_frames_are_small():
    for name in B.GROUPS:
        for f in B.group(name):
            assert f.total <= 5 * B.BS and f.data.size <= 5 * B.BS, f.name
    assert max(len(f.blocks) for f in B.group("measured")) == 129


def test_lone_block_inputs_claims():
    assert B.lone_claims()


def test_header_states_where_a_block_ends_for_the_frame_batch():
    import os
    with open(os.path.join(os.path.dirname(lz4mi.PKG_DIR), "include", "lz4mi.h")) as f:
        header = f.read()
    doc = header[header.index(" * lz4mi_frames_decompress takes the lists"):header.index("int32_t lz4mi_frames_index(")]
    assert "A block ends where its size word says" in doc and "lz4mi_host_block_read_end" in doc
    # the input that shows it, and that it is the only one
    assert B.OVER_READ == ("st_fuzz9_measured",) and B.claims()
