"""CPU: what the blocks of mode_kernels_common claim, on the oracle alone -- the selection shapes' two decodes
differ, and the short-literal shapes put their runs where they say (token positions against the 1 KiB chunk and
its staged window, sequence indices, prefix lengths)."""
import numpy as np

import mode_kernels_common as M
import rewrite_shapes_common as X


def test_selection_shapes_decode_differently_in_the_two_modes():
    for name in M.SELECT + (M.BELOW,) + M.LONE_HISTORY + M.LONE_DICTIONARY:
        s = M.shape(name)
        (sst, sw, spec), (rst, rw, ref) = X.expected(name, False), X.expected(name, True)
        assert sst == rst == 0 and sw == rw, name
        assert (spec != ref).any(), (name, "the reference's bytes are the spec's")
        assert s.cap <= 65536 and s.comp.size <= 20 * 1024 + 512, name
    for name in M.SELECT:                           # inside a batch: both modes decode them
        assert {e: X.isolated(M.shape(name), e) for e in X.MODES} == {False: 0, True: 0}, name
    # a rewrite below the slot: ERR_CROSS_BLOCK in reference mode only
    assert {e: X.isolated(M.shape(M.BELOW), e) for e in X.MODES} == {False: 0, True: X.CROSS}
    # the lone routes: bytes below the slot change (the small path's redo launch), a history, a dictionary
    below = [int((X.expected(n, False)[2] != X.expected(n, True)[2])[:X.out_off(M.shape(n))].sum()) for n in M.LONE_HISTORY]
    assert below == [4, 0] and all(M.shape(n).history is not None for n in M.LONE_HISTORY)
    assert all(M.shape(n).dictionary is not None and X.out_off(M.shape(n)) == 0 for n in M.LONE_DICTIONARY)


def test_short_literal_shapes_are_what_they_claim():
    assert M.claims() == 15 + 2 + 30 + 2 + 6
    cs = M.all_cases()
    assert {cs[f"places_{n}"][2]["n"] for n in M.RUNS} == set(M.RUNS)
    assert {(cs[f"remap_{n}_c{c}"][2]["nl"], c) for n in M.RUNS for c in (0, 1)} == {(n, c) for n in M.RUNS for c in (0, 1)}
    assert max(c[1] for c in cs.values()) <= 65536


def test_no_short_read_reaches_the_windows_end():
    """A table sequence's token lies below CHUNK, a short run's length field is at most two bytes: its 16-byte
    stage read ends at or before CHUNK + 2 + 16, inside the staged window (and places_n holds that run)."""
    assert M.CHUNK - 1 + 2 + 16 <= M.LIM < M.STAGED
    for n in M.RUNS:
        comp, cap, says, ref = M.all_cases()[f"places_{n}"]
        tok, lp, ll, off, ml, o = M.table_of(comp)[says["at"]["last_of_chunk0"]]
        assert (tok, lp, ll) == (M.CHUNK - 1, M.CHUNK + (n == 15), n)


def test_hand_decode_matches_the_oracle():
    """The builder's own bytes (X.Block.out) are the oracle's, for a few cases."""
    for name, (seqs, fin, says) in list(M.raw_cases().items())[::7]:
        out = bytearray()
        for lits, off, ml in seqs:
            out += lits
            for _ in range(ml):
                out.append(out[-off])
        out += fin
        comp, cap, _, ref = M.all_cases()[name]
        assert np.array_equal(np.frombuffer(bytes(out), dtype=np.uint8), ref[False][2][:cap]), name
