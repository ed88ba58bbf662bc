"""Shared by tests/test_mode_kernels_cpu.py and tests/test_gpu_mode_kernels.py.

Two things of csrc/lz4mi_decompress.hip are pinned here.

Kernel selection: the batch kernel exists once per decode mode (lz4mi_decompress_kernel for LZ4 spec,
lz4mi_decompress_ref_kernel for LZ4MI_JS_EXACT, which is also the redo launch of a reference-mode small batch),
chosen by lz4mi_launch_decompress from `mode`. The blocks are built shapes of rewrite_shapes_common whose
reference decode differs from their spec decode, so a launch of the wrong instantiation shows in the bytes.

Short literals: the chunk's own literal runs of 1-15 bytes are written by the pass over the sequence table that
precedes round 1 (dealt_literals: one ballot per row, then short_literals lane-parallel), and round 1's loop
keeps no literal store: its remapped short sources go through the LitDeal list. Hand-assembled blocks put such
runs at the places where those passes can go wrong. No sequence of these blocks rewrites (every match is 8 bytes
or longer), and every block is at most 64 KiB decoded.

A short case is (sequences, final literals, says); `says` names what the block claims about itself, and
claims() proves it on the oracle's parse alone.
"""
import functools

import numpy as np

import oracle as O
import rewrite_shapes_common as X
from linked_exact_common import parse
from literal_pieces_common import tokens_of
from test_gpu_seqtable import encode

CHUNK, LIM = X.CHUNK, X.LIM
STAGED = 4 * ((LIM + 28) // 4)     # bytes of the staged window with its slack (kStageWords)
RUNS = tuple(range(1, 16))         # the short run lengths
ROW_EDGES = (63, 64, 127, 128)
LIST = 64                          # kLitRuns: entries of the remapped runs' list


# ------------------------------------------------------------------------------------------- kernel selection
SELECT = ("chain_ml4_depth3", "rows_64", "cut_run_1100_ml4", "dense_0")     # decode inside a batch in both modes
BELOW = "cond_below_a"                                                      # reference mode refuses it in a batch
LONE_HISTORY = ("history_ll0_ml4", "history_inside_a")                      # 4 bytes / none below the slot change
LONE_DICTIONARY = ("dictionary_a", "dictionary_a_ll1")


def shape(name):
    return next(s for s in X.shapes() if s.name == name)


# ---------------------------------------------------------------------------------------------- the builder
class Block(X.Block):
    """rewrite_shapes_common's builder with sequences that never rewrite."""

    def z(self, n=1, ml=None):
        """n sequences without literals: three compressed bytes, a match of 8..18."""
        for _ in range(n):
            self.seq(0, int(self.rng.integers(8, 19)) if ml is None else ml, self._off())

    def lit(self, ll, ml=None):
        """A sequence of ll literals and a match of 8..18 bytes somewhere in the output before them."""
        ml = int(self.rng.integers(8, 19)) if ml is None else ml
        if self.pos == 0:
            return self.seq(ll, ml, int(self.rng.integers(1, ll + 1)))
        return self.seq(ll, ml, self._off())

    def _off(self):
        return int(self.rng.integers(1, min(self.pos, 65535) + 1))

    def pad(self, size):
        """Sequences without literals until the block holds exactly `size` compressed bytes: three-byte ones and
        up to two four-byte ones (a match of 19..30 bytes: one length byte)."""
        rem = size - self.size
        b = rem % 3
        a = (rem - 4 * b) // 3
        assert a >= 0 and 3 * a + 4 * b == rem, (size, self.size)
        for _ in range(b):
            self.seq(0, int(self.rng.integers(19, 31)), self._off())
        self.z(a)


def _span(n):
    return 1 + (1 if n == 15 else 0) + n + 2       # compressed bytes of a sequence of n literals and a short match


def case_places(n):
    """Runs of n bytes: the block's first sequence; sequences 63, 64, 127 and 128 of the first chunk's table, alone
    in their rows (every other sequence there has no literals); the first chunk's last sequence, its token at
    chunk offset 1023 -- the highest a table sequence's token lies, so its 16-byte stage read is the farthest
    into the window a short run's can reach --; the second chunk's first sequence; and the block's n final
    literals, which end at the capacity and whose stage read runs past the staged block's end. 1500 more
    compressed bytes before the end keep the first two chunks on the fast next-token table."""
    b = Block(13000 + n)
    at = {}
    at["first"] = b.lit(n)[0]
    for k in ROW_EDGES:
        b.z(k - len(b.seqs))
        at[f"seq{k}"] = b.lit(n)[0]
    b.pad(CHUNK - 1)
    at["last_of_chunk0"] = b.lit(n)[0]
    at["first_of_chunk1"] = b.lit(n)[0]
    b.z(500)
    return b.seqs, b.lits(n), dict(kind="places", n=n, at=at)


def case_dense_row(seed, same):
    """Every sequence holds a short run: 1, 2, ... 15, 1, ... bytes (or `same` bytes each, text's usual shape),
    so all 64 lanes of the first chunk's rows do."""
    b = Block(seed)
    for k in range(260 if same else 130):
        b.lit(same or 1 + k % 15)
    return b.seqs, b.lits(3), dict(kind="dense", rows=1 if not same else 2)


def case_remap(nl, chunk):
    """A run of L = max(nl, 8) literals with a match of 24 bytes (in chunk 1: from the first chunk's output), then
    with no literals: a match of nl + 10 bytes that starts nl bytes before the run's end and goes on into the
    run's match (remap_src's result 3, a prefix of nl bytes; in chunk 0 the run's match is output of the same
    table, so the match waits for a later round), and a match of 8..L bytes wholly inside the run (result 2);
    short sequences behind them."""
    b = Block(13100 + 16 * chunk + nl)
    b.lit(30)
    if chunk:
        b.pad(CHUNK)
    else:
        b.z(3)
    L = max(nl, 8)
    a = b.pos                                            # the run's first byte
    src0 = int(b.rng.integers(0, b.pos - 24)) if chunk else None
    j = b.seq(L, 24, (a + L - src0) if chunk else int(b.rng.integers(24, a + L + 1)))[0]
    split = b.copy(0, nl + 10, a + L - nl)[0]
    inside = b.copy(0, min(L, 8 + nl % 8), a)[0]
    b.z(6)
    return b.seqs, b.lits(4), dict(kind="remap", nl=nl, chunk=chunk, run=j, split=split, inside=inside)


def case_list_flush(ml):
    """A run of 40 literals, then 100 three-byte sequences whose matches of ml bytes (16: dealt pieces; 8: one piece
    of its exact width) lie wholly inside it: 63 listed runs in the table's first row and 37 in its second, more
    than the list holds."""
    b = Block(13200 + ml)
    b.seq(40, 9, 7)
    first = len(b.seqs)
    for _ in range(100):
        b.copy(0, ml, int(b.rng.integers(0, 40 - ml + 1)))
    b.z(5)
    return b.seqs, b.lits(6), dict(kind="flush", first=first, count=100, ml=ml)


def case_slack(ml, far):
    """A remapped short source at the window's end: a token at chunk offset 900 with 184 literals, which end at
    kLim - 2, and a match of ml = 8..12 bytes at offset ml, i.e. a copy of its own last ml literals (remap_src's
    result 2). The 16-byte stage read of that source, in LitDeal::flush, starts at kLim - 2 - ml and runs past
    kLim into the stage's slack. far: 1500 more compressed bytes follow (the fast next-token table), else the
    block ends soon (the exact one)."""
    b = Block(13400 + ml + (100 if far else 0))
    b.lit(30)
    b.pad(900)
    k = b.seq(LIM - 2 - 902, ml, ml)[0]
    b.z(500 if far else 20)
    return b.seqs, b.lits(5), dict(kind="slack", index=k, ml=ml, far=far)


def raw_cases():
    out = {}
    for n in RUNS:
        out[f"places_{n}"] = case_places(n)
    out["dense_row_cycle"] = case_dense_row(13050, 0)
    out["dense_row_ones"] = case_dense_row(13051, 1)
    for chunk in (0, 1):
        for nl in RUNS:
            out[f"remap_{nl}_c{chunk}"] = case_remap(nl, chunk)
    out["list_flush"] = case_list_flush(16)
    out["list_flush_short"] = case_list_flush(8)
    for far in (True, False):
        for ml in (8, 9, 12):
            out[f"slack_{ml}_{'far' if far else 'near'}"] = case_slack(ml, far)
    return out


@functools.lru_cache(maxsize=None)
def all_cases():
    """name -> (compressed block, capacity = decoded size, says, {js: the oracle's (status, written, bytes)})."""
    done = {}
    for name, (seqs, fin, says) in raw_cases().items():
        comp = encode(seqs, fin)
        st, cap, _ = O.decompress_block(comp, 1 << 16)
        assert st == 0 and cap <= (1 << 16), name
        ref = {js: O.decompress_block(comp, cap, js_compat=js) for js in (False, True)}
        done[name] = (comp, cap, says, ref)
    return done


# ---------------------------------------------------------------------------------------------------- claims
def table_of(comp):
    """The oracle's parse: [(token offset, literals' offset, literal length, match offset, match length, output
    start)] per sequence."""
    toks, out, pos = tokens_of(comp), [], 0
    for k, (lp, ll, off, ml) in enumerate(parse(comp)):
        out.append((toks[k], lp, ll, off, ml, pos))
        pos += ll + ml
    return out


def chunks_of(seqs, size):
    """The batch kernel's chunks on a block no sequence of which overruns its window: [(start, [indices of the
    sequences whose tokens lie in [start, start + CHUNK)])]; the next chunk starts where the last one ends."""
    out, k = [], 0
    while k < len(seqs):
        start, idx = seqs[k][0], []
        while k < len(seqs) and seqs[k][0] < start + CHUNK:
            end = seqs[k + 1][0] if k + 1 < len(seqs) else size
            assert end - start <= LIM or k + 1 == len(seqs), "a sequence overruns its window"
            idx.append(k)
            k += 1
        out.append((start, idx))
    return out


@functools.lru_cache(maxsize=None)
def claims():
    """Every `says`, on the oracle's parse. -> the number of cases."""
    for name, (comp, cap, says, ref) in all_cases().items():
        seqs = table_of(comp)
        chunks = chunks_of(seqs, int(comp.size))
        assert ref[False][0] == 0 and ref[True][0] == 0 and ref[False][1] == cap <= 65536, name
        assert not [q for q in seqs if q[3] >= 8 and 4 <= q[4] < 8], (name, "a sequence rewrites")
        assert np.array_equal(ref[False][2], ref[True][2]), name
        kind = says["kind"]
        if kind == "places":
            n, at = says["n"], says["at"]
            (c0, i0), (c1, i1) = chunks[0], chunks[1]
            assert c0 == 0 and at["first"] == i0[0] == 0, name
            for k in ROW_EDGES:                                # their table index is their index in the block
                assert at[f"seq{k}"] == k and k in i0, name
            with_lits = [k for k in i0 if seqs[k][2]]
            assert with_lits == [0, *ROW_EDGES, i0[-1]] and all(seqs[k][2] == n for k in with_lits), name
            last = seqs[at["last_of_chunk0"]]
            assert at["last_of_chunk0"] == i0[-1] and last[0] == CHUNK - 1, name
            # no short run's stage read reaches further: a table sequence's token lies below CHUNK
            assert last[1] == CHUNK + (n == 15) and last[1] + 16 <= LIM, name
            assert at["first_of_chunk1"] == i1[0] and c1 == last[0] + _span(n) and seqs[i1[0]][2] == n, name
            assert comp.size - c1 > X.FAST_REM, name
            fin = seqs[-1]
            assert fin[3] == 0 and fin[2] == n and fin[5] + n == cap, name
            assert fin[1] - chunks[-1][0] + 16 > comp.size - chunks[-1][0], (name, "the last read stays inside the block")
        elif kind == "dense":
            c0, i0 = chunks[0]
            assert len(i0) >= 64 * says["rows"] and all(1 <= seqs[k][2] <= 15 for k in i0[:64 * says["rows"]]), name
            assert {seqs[k][2] for k in i0[:64]} == ({1} if says["rows"] == 2 else set(RUNS)), name
        elif kind == "remap":
            nl, c = says["nl"], says["chunk"]
            start, idx = chunks[c]
            assert len(chunks) == c + 1 and (start == CHUNK if c else start == 0), (name, start)
            j, sp, ins = says["run"], says["split"], says["inside"]
            assert {j, sp, ins} <= set(idx) and idx.index(sp) < 256, name      # (the split is taken in rows 0..3)
            tok, lp, ll, off, ml, o = seqs[j]
            assert nl <= ll <= 15 and ll >= 8, name
            first_out = seqs[idx[0]][5]                       # the chunk's first output byte
            assert o + ll - off + ml <= first_out if c else o + ll - off < o + ll, name   # chunk 1: from finished output
            t = seqs[sp]
            src = t[5] + t[2] - t[3]
            assert src == o + ll - nl and src + t[4] <= o + ll + ml and t[4] > nl, name
            t = seqs[ins]
            src = t[5] + t[2] - t[3]
            assert o <= src and src + t[4] <= o + ll and 8 <= t[4] < 16, name
        elif kind == "flush":
            c0, i0 = chunks[0]
            run = seqs[0]
            listed = [k for k in i0 if seqs[k][4] == says["ml"] and k >= says["first"] and seqs[k][5] - seqs[k][3] >= run[5]
                      and seqs[k][5] - seqs[k][3] + seqs[k][4] <= run[5] + run[2]]
            assert run[2] == 40 and len(listed) == says["count"] > LIST, name
            assert sum(k < 64 for k in listed) <= LIST < len(listed) and max(listed) < 128, name
        elif kind == "slack":
            (c0, i0), (c1, i1) = chunks[0], chunks[1]
            k, ml = says["index"], says["ml"]
            tok, lp, ll, off, m, o = seqs[k]
            assert c0 == 0 and k == i0[-1] and tok == 900 and lp + ll == LIM - 2 and c1 == LIM, name
            assert off == m == ml and 8 <= ml < 16, name                 # the source: its own last ml literals
            src = lp + ll - off                                          # ... at this stage index
            assert src + 16 > LIM and src + 16 <= STAGED, (name, src)
            assert (comp.size - c1 > X.FAST_REM) == says["far"] and (says["far"] or comp.size <= X.FAST_REM), name
        else:
            raise AssertionError(name)
    return len(all_cases())
