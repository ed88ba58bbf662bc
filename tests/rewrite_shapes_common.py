"""Shared by tests/test_rewrite_shapes_cpu.py and tests/test_gpu_rewrite_shapes.py: raw blocks BUILT to put
the reference decoder's double-copy-tail rewrite (after a match at s with offset >= 8 and length
ml < 8, out[p] = out[p - off] for p in [s + ml - 8, s)) at chosen places inside a block, instead of meeting it
by chance in random streams. Five decoders reproduce the rewrite in reference mode: the batch kernel's step 7
(csrc/lz4mi_decompress.hip: f1_changes, f1_table, f1_fixup, cut_match), the small path's pointer pass
(csrc/lz4mi_expand.hip: lz4mi_xf1ptr_kernel, with redo[] back to the batch kernel), its linked variant, the
serial kernel and the host decoder.

A shape is (name, family, compressed block, capacity, history bytes or None, dictionary or None, says):
with a history the block is decoded at out_off = len(history) of an array that holds those bytes; `says` is
what the shape claims about itself, and claims() proves every word of it on the CPU oracle alone, through
walk(), a pure-Python walk of the block's sequences. The blocks are assembled with test_gpu_seqtable's
encode / Maker; Block keeps the reference's bytes while it builds, so that an offset can be chosen for which
a rewrite changes bytes. Literal bytes are random, so a stale or misplaced byte shows.

Families (each builder's docstring says more): cond, no_change, chain, rewrite_of_rewrite, periodic,
wave_match, dense, rows, chunk_edge, cut, segment, clipped, history, dictionary.
"""
import collections
import functools
import json
import os

import numpy as np

import oracle as O
from linked_exact_common import MESSAGES, parse
from literal_pieces_common import tokens_of
from test_gpu_seqtable import Maker, encode

CHUNK = 1024              # compressed bytes the batch kernel parses per step
LIM = CHUNK + 64          # kLim: chunk-relative bytes a table sequence may touch; one that ends past it is cut
FAST_REM = 1024 + 64 + 300  # kFastRem: the fast next-token table (and `defer`) is in use this far from the end
OK, DICT_OOB, CROSS = 0, -4, -9
MODES = (False, True)     # js_compat of the oracle: spec, the reference decoder's bytes
NAIVE = ("chain", "rewrite_of_rewrite", "periodic", "cut")     # families a naive replay must get wrong
FAMILIES = ("cond", "no_change", "chain", "rewrite_of_rewrite", "periodic", "wave_match", "dense", "rows",
            "chunk_edge", "cut", "segment", "clipped", "history", "dictionary")

Shape = collections.namedtuple("Shape", "name family comp cap history dictionary says")


def frozen(a):
    a = np.ascontiguousarray(np.frombuffer(bytes(a), dtype=np.uint8) if isinstance(a, (bytes, bytearray)) else a,
                             dtype=np.uint8)
    a.setflags(write=False)
    return a


def _ext(v):
    return 0 if v < 15 else 1 + (v - 15) // 255


def seg_geom(in_len):
    """csrc/lz4mi_decompress.h seg_geom: S segments of L compressed bytes (the small path's waves)."""
    s = max(1, min(256, -(-in_len // 8192)))
    return s, max(4096, (-(-in_len // s) + 1023) & ~1023)


# ------------------------------------------------------------------------------------------------ the builder
class Block(Maker):
    """A block under construction. `out` is the whole array as the reference decoder leaves it after the
    sequences so far (the history first), `pos` the block's own bytes so far, `size` its compressed bytes so
    far: the next sequence's token offset. Positions handed in and out are relative to the block's start."""

    def __init__(self, seed, history=None, dictionary=None):
        super().__init__(seed)
        self.history = None if history is None else bytes(history)
        self.dictionary = None if dictionary is None else bytes(dictionary)
        self.h = len(self.history or b"")
        self.out = bytearray(self.history or b"")
        self.seqs, self.size, self.says = [], 0, {}

    def seq(self, ll, ml, off, lits=None):
        """One sequence -> (its index, its token offset, where its match starts)."""
        lits = self.lits(ll) if lits is None else bytes(lits)
        assert len(lits) == ll and 1 <= off <= 65535 and ml >= 4
        idx, tok = len(self.seqs), self.size
        self.out += lits
        s = len(self.out)
        if s - off < 0:                               # the reference's dictionary branch: no rewrite
            d = self.dictionary or b""
            nd, di = min(off - s, ml), len(d) + s - off
            assert di >= 0, "the builder's dictionary is too short"
            self.out += d[di:di + nd]
            for _ in range(nd, ml):
                self.out.append(self.out[len(self.out) - off])
        else:
            for _ in range(ml):
                self.out.append(self.out[-off])
            if off >= 8 and ml < 8:
                for p in range(max(0, s + ml - 8), s):
                    self.out[p] = self.out[p - off] if p - off >= 0 else 0
        self.seqs.append((lits, off, ml))
        self.size += 1 + _ext(ll) + ll + 2 + _ext(ml - 4)
        self.pos = len(self.out) - self.h
        return idx, tok, s - self.h

    def lead(self, ll=16):
        """The block's first sequence: `ll` literals (>= 8 and more than any rewrite that follows reads back,
        so that the block decodes inside a batch) and a match of 9 bytes inside them."""
        return self.seq(ll, 9, int(self.rng.integers(1, ll + 1)))

    def fill(self, n, hi=19):
        """n four-byte sequences that never rewrite: one literal and a match of 8 .. hi - 1 bytes."""
        for _ in range(n):
            self.seq(1, int(self.rng.integers(8, hi)), int(self.rng.integers(1, min(self.pos + 1, 65535) + 1)))

    def pad_to(self, size):
        """Up to three three-byte sequences (no literal), then four-byte ones until the block holds exactly `size`
        compressed bytes; none of them rewrites."""
        rem = size - self.size
        b = (3 * rem) % 4
        a = (rem - 3 * b) // 4
        assert a >= 0 and 4 * a + 3 * b == rem, (size, self.size)
        for _ in range(b):
            self.seq(0, int(self.rng.integers(8, 15)), int(self.rng.integers(1, min(self.pos, 65535) + 1)))
        self.fill(a, 15)

    def rw(self, ll, ml, off=None, lo=8, hi=None, inside=True):
        """A rewriting sequence (ml < 8, off >= 8, source in the array) whose rewrite changes EVERY byte of its
        region: the offset (or, with a given offset, the literals) is drawn until it does. inside: the match's
        and the rewrite's sources stay inside the block. -> (index, token offset, match start, region start)."""
        assert 4 <= ml < 8
        for _ in range(256):
            lits = self.lits(ll)
            tail = self.out + lits
            s = len(tail)
            p0 = s + ml - 8
            o = off
            if o is None:
                top = min(65535, p0 - (self.h if inside else 0), hi or 65535)
                assert top >= lo, (ll, ml, s, "no room for an offset")
                o = int(self.rng.integers(lo, top + 1))
            if all(tail[p] != (tail[p - o] if p - o >= 0 else 0) for p in range(max(p0, 0), s)):
                idx, tok, sr = self.seq(ll, ml, o, lits)
                return idx, tok, sr, sr + ml - 8
        raise AssertionError("no draw makes the rewrite change its whole region")

    def copy(self, ll, ml, src):
        """A sequence whose match copies from block position `src` (negative: the history)."""
        return self.seq(ll, ml, self.pos + ll - src)

    def shape(self, name, family, fin=5, cap=None, dictionary="own", **says):
        fl = None if fin is None else self.lits(fin)
        comp = encode(self.seqs, fl)
        assert comp.size == self.size + (0 if fin is None else 1 + _ext(fin) + fin), name
        n = self.pos + (fin or 0)
        says = dict(self.says, **says)
        d = self.dictionary if dictionary == "own" else dictionary
        return Shape(name, family, frozen(comp), int(n if cap is None else cap),
                     None if self.history is None else frozen(self.history), None if d is None else frozen(d), says)


# --------------------------------------------------------------------------------------------------- families
def cases_cond():
    """The edges of the rewrite's condition, (offset, match length): (8,7) (8,4) (9,4) (8,5) (8,6) (20,4) rewrite,
    (7,7) and (8,8) do not; (65535,4) behind 64 KiB of output; dictbranch: offset 16, length 5 through the
    dictionary branch, where the reference rewrites nothing; below_a / below_b: the rewrite's source starts
    below the block (the reference reads 0 there; batched, reference mode refuses the block)."""
    out = []
    for i, (off, ml, n) in enumerate(((8, 7, 1), (8, 4, 1), (7, 7, 0), (8, 8, 0), (9, 4, 1), (8, 5, 1), (8, 6, 1), (20, 4, 1))):
        b = Block(11000 + i)
        if n:
            k, tok, s, p0 = b.rw(24, ml, off=off)
            b.copy(1, 12, p0 - 2)
            keys = [(k, tok)]
        else:
            b.seq(24, ml, off)
            b.fill(1)
            keys = []
        out.append(b.shape(f"cond_off{off}_ml{ml}", "cond", rewrites=n, changed=bool(n), keys=keys))
    b = Block(11020)
    b.seq(3000, 270, 2000)
    while b.pos < 65545:
        b.seq(int(b.rng.integers(0, 3)), 270, int(b.rng.integers(300, 3000)))
    k, tok, s, p0 = b.rw(1, 4, off=65535)
    b.copy(1, 12, p0 - 2)
    out.append(b.shape("cond_off_65535", "cond", rewrites=1, changed=True, keys=[(k, tok)]))
    b = Block(11021, dictionary=Maker(11022).lits(64))
    b.seq(10, 5, 16)                                   # starts 6 bytes below out[0]: all 5 bytes from the dictionary
    b.fill(3)
    out.append(b.shape("cond_dictbranch", "cond", rewrites=0, changed=False, keys=[]))
    for name, ll, off, ml in (("below_a", 9, 8, 4), ("below_b", 10, 10, 5)):
        b = Block(11030 + ll)
        k, tok, s, p0 = b.rw(ll, ml, off=off, inside=False)
        b.copy(1, 12, p0 - 1)
        out.append(b.shape(f"cond_{name}", "cond", rewrites=1, changed=True, keys=[(k, tok)], reads_below=True))
    return out


def cases_no_change():
    """Rewrites whose region already equals its source: constant data, periods 2 and 4 with offsets that are
    multiples of the period, and a region inside a run of one byte. The reference's bytes are the spec's."""
    out = []
    for name, per, moves in (("const", b"\x37", ((0, 4, 8), (0, 5, 9), (1, 7, 12))),
                             ("per2", b"\x11\xE2", ((0, 4, 8), (0, 6, 10), (2, 4, 12))),
                             ("per4", b"\x01\x02\x03\x04", ((0, 4, 8), (0, 4, 12), (4, 4, 16)))):
        b = Block(11100)
        first = (per * 24)[:24]
        for j, (ll, ml, off) in enumerate(moves):
            at = b.pos
            lits = first if j == 0 else bytes((per * 32)[(at + t) % len(per)] for t in range(ll))
            b.seq(24 if j == 0 else ll, ml, off, lits)
        out.append(b.shape(f"no_change_{name}", "no_change", fin=None, rewrites=3, changed=False, keys=[]))
    b = Block(11101)
    b.seq(10, 40, 1)
    b.seq(0, 5, 9)
    b.fill(2)
    out.append(b.shape("no_change_run", "no_change", rewrites=1, changed=False, keys=[]))
    return out


def cases_chain():
    """A region, a later match of the same chunk that copies it, a match that copies that copy, ...: depths 1, 2,
    3 and 8, for a region of 4 bytes (ml 4) and of 1 byte (ml 7)."""
    out = []
    for ml in (4, 7):
        for depth in (1, 2, 3, 8):
            b = Block(11200 + 10 * ml + depth)
            b.lead()
            k, tok, s, p0 = b.rw(1, ml)
            src, deps = p0 - 1, []
            for _ in range(depth):
                d, _, ds = b.copy(1, 10, src)
                deps.append(d)
                src = ds
            out.append(b.shape(f"chain_ml{ml}_depth{depth}", "chain", rewrites=1, changed=True, keys=[(k, tok)], deps=deps,
                               where="chunk0"))
    return out


def cases_rewrite_of_rewrite():
    """A later rewrite whose source is an earlier region R0 = [p0, p0 + 4): both -- its region reads R0's first
    half and its match R0's second half; region_only -- its region reads exactly R0; one_byte -- ml 7, a region
    of one byte that reads R0. Each followed by a match that copies the later region."""
    out = []
    for i, (name, ml1, d) in enumerate((("both", 4, 2), ("region_only", 4, 4), ("one_byte", 7, 2))):
        b = Block(11300 + i)
        b.lead()
        k0, t0, s0, p0 = b.rw(1, 4)
        b.fill(2)
        k1, t1, s1 = b.seq(1, ml1, b.pos + 1 - (p0 + d))
        dep, _, _ = b.copy(1, 10, s1 + ml1 - 8 - 1)
        out.append(b.shape(f"rewrite_of_rewrite_{name}", "rewrite_of_rewrite", rewrites=2, changed=True,
                           keys=[(k0, t0), (k1, t1)], deps=[k1, dep], where="chunk0"))
    return out


def cases_periodic():
    """fwd: behind a rewriting match a periodic one (offset q in 5..7, q < length, 40..300 bytes) whose period
    starts inside the region: the t % off recopy of step 7. rev: a run of period q in 1..3 (a match of 100
    bytes), then with no literals a rewriting match of 4 whose region is the run's last 4 bytes and whose source
    is no multiple of q away (inside the run), or lies in the literals before the run; then a match that copies
    the region."""
    out = []
    for i, (ml0, ll1, q, n) in enumerate(((4, 0, 5, 40), (4, 0, 7, 300), (4, 1, 6, 64), (4, 2, 7, 41), (5, 0, 6, 300),
                                          (5, 0, 7, 130), (6, 0, 7, 257))):
        b = Block(11400 + i)
        b.lead()
        k, tok, s, p0 = b.rw(1, ml0)
        d, _, ds = b.seq(ll1, n, q)
        assert p0 <= ds - q < s
        out.append(b.shape(f"periodic_fwd_ml{ml0}_ll{ll1}_q{q}_n{n}", "periodic", rewrites=1, changed=True, keys=[(k, tok)],
                           deps=[d], where="chunk0", period=(d, q)))
    for i, (q, off) in enumerate(((1, 106), (2, 9), (2, 107), (3, 10), (3, 31), (3, 108))):
        b = Block(11450 + i)
        lits = bytearray(b.lits(12))
        for t in range(1, 4):                           # the period's bytes all differ
            lits[-t] = (lits[-t] & 0xFC) | t
        _, _, m0 = b.seq(12, 100, q, lits)
        k, tok, s, p0 = b.rw(0, 4, off=off)
        assert p0 >= m0 and (off % q or s - off < m0)
        d, _, _ = b.copy(1, 10, p0 - 1)
        out.append(b.shape(f"periodic_rev_q{q}_off{off}", "periodic", rewrites=1, changed=True, keys=[(k, tok)], deps=[d],
                           where="chunk0", run=(m0, q)))
    return out


def cases_wave_match():
    """The region is the tail of a match of more than 256 bytes (the whole wave writes it), no literals before
    the rewriting match; then a match that copies the region."""
    out = []
    for i, (n, ml) in enumerate(((257, 4), (257, 7), (300, 5), (1000, 4), (1000, 6))):
        b = Block(11500 + i)
        b.lead(n + 150)
        b.seq(2, n, n + 40)
        k, tok, s, p0 = b.rw(0, ml)
        d, _, _ = b.copy(1, 10, p0 - 1)
        out.append(b.shape(f"wave_match_n{n}_ml{ml}", "wave_match", rewrites=1, changed=True, keys=[(k, tok)], deps=[d],
                           long_match=n))
    return out


def cases_dense():
    """600 sequences of 0 or 1 literals, a match of 4..7 bytes and an offset of 8..40, over three chunks."""
    out = []
    for seed in (11600, 11601):
        b = Block(seed)
        b.seq(48, int(b.rng.integers(4, 8)), int(b.rng.integers(8, 41)))
        for _ in range(599):
            b.seq(int(b.rng.integers(0, 2)), int(b.rng.integers(4, 8)), int(b.rng.integers(8, 41)))
        out.append(b.shape(f"dense_{seed - 11600}", "dense", rewrites=600, changed=True, keys=[], chunks=3))
    return out


def cases_rows():
    """The rewriting sequence at index 62, 63, 64, 65, 127 or 128 of the first chunk's sequence table (row i
    holds sequences 64 i .. 64 i + 63), a match that copies its region right behind it (the same row, but for
    63 and 127) and one in the next row."""
    out = []
    for at in (62, 63, 64, 65, 127, 128):
        b = Block(11700 + at)
        b.lead()
        b.fill(at - 1)
        k, tok, s, p0 = b.rw(1, 4 + at % 4)
        d1, _, _ = b.copy(1, 10, p0 - 1)
        nxt = 64 * (at // 64 + 1) + 5
        b.fill(nxt - len(b.seqs))
        d2, _, _ = b.copy(1, 10, p0 - 2)
        b.fill(3)
        out.append(b.shape(f"rows_{at}", "rows", rewrites=1, changed=True, keys=[(k, tok)], deps=[d1, d2], where="chunk0",
                           index=at))
    return out


def cases_chunk_edge():
    """last_T: the rewriting sequence's token at compressed offset T = 1020..1023, the last of the first 1 KiB
    chunk, the matches that copy its region in the second chunk. first_T: its token at T = 1024..1027, the first
    of the second chunk, no literals: its region is output of the first chunk."""
    out = []
    for T in (1020, 1021, 1022, 1023, 1024, 1025, 1026, 1027):
        b = Block(11800 + T)
        b.lead()
        b.pad_to(T)
        k, tok, s, p0 = b.rw(1 if T < CHUNK else 0, 4 + T % 4)
        d1, _, _ = b.copy(1, 10, p0 - 1)
        b.fill(20)
        d2, _, _ = b.copy(1, 10, p0 - 2)
        b.fill(5)
        kind = "last_of_chunk0" if T < CHUNK else "first_of_chunk1"
        out.append(b.shape(f"chunk_edge_{'last' if T < CHUNK else 'first'}_{T}", "chunk_edge", rewrites=1, changed=True,
                           keys=[(k, tok)], deps=[d1, d2], where=kind))
    return out


def cases_cut():
    """run_R_mlM: the cut sequence itself rewrites -- a literal run of R = 1100..1500 bytes from the first chunk
    past the staged window, then a match of M < 8 at an offset >= 8; its region is the run's last bytes; matches
    that copy the region follow. deferred_T: a run of 600 literals from a token at chunk offset T = 900 / 1000,
    far from the block's end: the batch kernel leaves it to the next chunk, which starts at it. reads_region: a
    rewrite in the table, then a cut sequence whose match (12 bytes; and 5 bytes, rewriting too) copies that
    region."""
    out = []
    for i, (R, ml) in enumerate(((1100, 4), (1200, 5), (1300, 6), (1500, 7), (1400, 4), (1150, 7))):
        b = Block(11900 + i)
        b.lead()
        b.fill(8)
        k, tok, s, p0 = b.rw(R, ml)
        d1, _, _ = b.copy(1, 10, p0 - 1)
        b.fill(5)
        d2, _, _ = b.copy(1, 10, p0 - 2)
        out.append(b.shape(f"cut_run_{R}_ml{ml}", "cut", rewrites=1, changed=True, keys=[(k, tok)], deps=[d1, d2], where="cut"))
    for T, ml in ((900, 4), (1000, 6)):
        b = Block(11950 + ml)
        b.lead()
        b.pad_to(T)
        k, tok, s, p0 = b.rw(600, ml)
        d1, _, _ = b.copy(1, 10, p0 - 1)
        b.fill(450)
        out.append(b.shape(f"cut_deferred_{T}_ml{ml}", "cut", rewrites=1, changed=True, keys=[(k, tok)], deps=[d1], where="deferred"))
    for ml in (12, 5):
        b = Block(11960 + ml)
        b.lead()
        b.fill(8)
        k, tok, s, p0 = b.rw(1, 4)
        b.fill(3)
        c, ctok, cs = b.copy(1200, ml, p0 - 2 if ml >= 8 else p0)
        d1, _, _ = b.copy(1, 10, cs - 3)
        b.fill(4)
        keys = [(k, tok)] + ([(c, ctok)] if ml < 8 else [])
        out.append(b.shape(f"cut_reads_region_ml{ml}", "cut", rewrites=len(keys), changed=True, keys=keys, deps=[c, d1],
                           where="cut", cut_index=c))
    return out


def cases_segment():
    """Blocks of 9000 (two small-path segments of 5120) and 17000 compressed bytes (three of 6144): the
    rewriting sequence is the first token at or past k L (k L + delta, delta 0..2), no literals: its region is the
    previous segment's output; a match that copies the region follows."""
    out = []
    for n in (9000, 17000):
        S, L = seg_geom(n)
        for delta in (0, 1, 2):
            b = Block(12000 + n + delta)
            b.lead()
            keys, deps = [], []
            for k in range(1, S):
                b.pad_to(k * L + delta)
                kk, tok, s, p0 = b.rw(0, 4 + (k + delta) % 4)
                d, _, _ = b.copy(1, 10, p0 - 1)
                keys.append((kk, tok))
                deps.append(d)
            b.pad_to(n - 6)
            out.append(b.shape(f"segment_{n}_d{delta}", "segment", rewrites=S - 1, changed=True, keys=keys, deps=deps,
                               where="segment", size=n))
    return out


def cases_clipped():
    """The block ends on a rewriting match of ml bytes; the capacity cuts 0, 1 and ml - 1 bytes off it: status 0,
    out_len above the capacity. The region lies before the match, among bytes that must fit: it is never clipped."""
    out = []
    for ml in (4, 5, 7):
        for cut in (0, 1, ml - 1):
            b = Block(12100 + ml)
            b.lead()
            b.fill(6)
            k, tok, s, p0 = b.rw(2, ml)
            out.append(b.shape(f"clipped_ml{ml}_cut{cut}", "clipped", fin=None, cap=b.pos - cut, rewrites=1, changed=True,
                               keys=[(k, tok)], clip=cut, match_start=s))
    return out


HISTORY = 300


def _history(seed):
    return bytes(np.random.default_rng(seed).integers(1, 256, HISTORY, dtype=np.uint8))     # no zero byte


def cases_history():
    """The block decodes at out_off = 300 behind 300 bytes of history. ll_L_ml_M: the first sequence has L = 0..3
    literals, a match of M = 4..7 and an offset >= 8 inside the history, L + M < 8: 8 - M - L bytes below the slot
    change. inside_*: the region lies in the slot, its source in the history. first_byte_*: the offset is exactly
    L + 300, the array's first byte, so the rewrite reads below the array: zeros (2 of them below the slot in _a)."""
    out = []
    for ml in (4, 5, 6, 7):
        for ll in range(8 - ml):
            b = Block(12200 + 10 * ml + ll, history=_history(12200))
            k, tok, s, p0 = b.rw(ll, ml, hi=280, inside=False)
            b.copy(1, 10, p0 - 1)
            b.fill(4)
            out.append(b.shape(f"history_ll{ll}_ml{ml}", "history", rewrites=1, changed=True, keys=[(k, tok)], below=8 - ml - ll))
    for name, ll, ml, back in (("inside_a", 9, 4, 20), ("inside_b", 12, 7, 100)):
        b = Block(12290 + ll, history=_history(12201))
        k, tok, s, p0 = b.rw(ll, ml, off=ll + back, inside=False)
        b.copy(1, 10, p0 - 1)
        b.fill(4)
        out.append(b.shape(f"history_{name}", "history", rewrites=1, changed=True, keys=[(k, tok)], below=0))
    for name, ll, ml, below in (("first_byte_a", 2, 4, 2), ("first_byte_b", 9, 5, 0)):
        b = Block(12295 + ll, history=_history(12202))
        k, tok, s, p0 = b.rw(ll, ml, off=ll + HISTORY, inside=False)
        b.copy(1, 10, p0 - 1)
        b.fill(4)
        out.append(b.shape(f"history_{name}", "history", rewrites=1, changed=True, keys=[(k, tok)], below=below))
    return out


def cases_dictionary():
    """out_off 0 and a dictionary. a: 9 literals and a match of 4 at offset 8, whose rewrite of out[5, 9) reads
    positions -3 .. 0 and gets the reference's 0 for the three below the array, not dictionary bytes; then a match
    that starts 20 bytes inside the dictionary and spills over out[0, 12), the rewritten region included
    (f1_fixup's lane-0 branch). a_ll1: the spill behind one literal. b: the same spill with no rewrite before it
    (a match of 8). c_exact / c_short: a's block with a dictionary of exactly the 20 bytes the spill needs, and of
    19: the oracle's ERR_DICT_OOB."""
    out = []
    d = Maker(12300).lits(64)
    for name, ml0, ll1 in (("a", 4, 0), ("a_ll1", 4, 1), ("b", 8, 0)):
        b = Block(12301 + ml0 + ll1, dictionary=d)
        if ml0 < 8:
            k, tok, s, p0 = b.rw(9, ml0, off=8, inside=False)
        else:
            b.seq(9, ml0, 8)
        sp, _, ss = b.seq(ll1, 32, b.pos + ll1 + 20)
        b.copy(1, 10, ss + 20 + 4)                      # the spill's copy of out[4, 14)
        b.fill(3)
        says = dict(rewrites=1 if ml0 < 8 else 0, changed=ml0 < 8, keys=[(k, tok)] if ml0 < 8 else [], spill=sp)
        out.append(b.shape(f"dictionary_{name}", "dictionary", **says))
        if name == "a":
            out.append(out[-1]._replace(name="dictionary_c_exact", dictionary=frozen(d[-20:])))
            out.append(out[-1]._replace(name="dictionary_c_short", dictionary=frozen(d[-19:]), says=dict(says, status=DICT_OOB)))
    return out


BUILDERS = (cases_cond, cases_no_change, cases_chain, cases_rewrite_of_rewrite, cases_periodic, cases_wave_match,
            cases_dense, cases_rows, cases_chunk_edge, cases_cut, cases_segment, cases_clipped, cases_history,
            cases_dictionary)


@functools.lru_cache(maxsize=None)
def shapes():
    out = tuple(s for fn in BUILDERS for s in fn())
    assert len({s.name for s in out}) == len(out)
    return out


def by_family(fam):
    return [s for s in shapes() if s.family == fam]


# ------------------------------------------------------------------------------------------------- the oracle
def out_off(shape):
    return 0 if shape.history is None else int(shape.history.size)


def array_for(shape, cap=None, fill=0):
    """The caller's array: the history, then `cap` bytes of `fill`."""
    cap = shape.cap if cap is None else cap
    a = np.full(out_off(shape) + cap, fill, dtype=np.uint8)
    if shape.history is not None:
        a[:shape.history.size] = shape.history
    return a


@functools.lru_cache(maxsize=None)
def expected(name, exact, cap=None, fill=0):
    """The oracle's (status, written, whole array) of the shape decoded alone on array_for(shape, cap, fill)."""
    shape = next(s for s in shapes() if s.name == name)
    st, w, arr = O.decompress_block(shape.comp, 0, out=array_for(shape, cap, fill), out_off=out_off(shape),
                                    dictionary=shape.dictionary, js_compat=exact)
    arr.setflags(write=False)
    return int(st), int(w) if st == 0 else 0, arr


def walk(shape):
    """The block's sequences in block-relative output positions, from the compressed bytes alone:
    [(index, token offset, literals, offset, match length, match start)]; a final literal-only sequence has
    offset 0."""
    toks, out, pos = tokens_of(shape.comp), [], 0
    for k, (lp, ll, off, ml) in enumerate(parse(shape.comp)):
        out.append((k, toks[k], ll, off, ml, pos + ll))
        pos += ll + ml
    return out


def rewrites_of(shape):
    """The rewrites the reference performs: [(index, token offset, match start s, offset, match length)] of the
    sequences with ml < 8, offset >= 8 and a source inside the array (not the dictionary branch)."""
    h = out_off(shape)
    return [(k, tok, s, off, ml) for k, tok, ll, off, ml, s in walk(shape)
            if off >= 8 and 4 <= ml < 8 and h + s - off >= 0]


def naive_replay(shape):
    """The spec decode, then every region rewrite applied once in order, with no match copied again: what a
    decoder gives that rewrites the regions but never recopies a match that read one."""
    h = out_off(shape)
    st, w, arr = expected(shape.name, False)
    arr = arr.copy()
    for k, tok, s, off, ml in rewrites_of(shape):
        for p in range(max(0, h + s + ml - 8), min(h + s, arr.size)):
            arr[p] = arr[p - off] if p - off >= 0 else 0
    return arr


def isolated(shape, exact):
    """The status the block must get inside a batch of independent blocks: ERR_CROSS_BLOCK exactly when some
    match's source starts below the block or, in reference mode, when some rewriting match (source not below the
    block) has s + ml - 8 - off below the block; otherwise the oracle's status of the block alone, without history
    or dictionary."""
    for k, tok, ll, off, ml, s in walk(shape):
        if off and s - off < 0:
            return CROSS
        if exact and off >= 8 and 4 <= ml < 8 and s + ml - 8 - off < 0:
            return CROSS
    return O.decompress_block(shape.comp, shape.cap, js_compat=exact)[0]


# ----------------------------------------------------------------------------------------------------- claims
@functools.lru_cache(maxsize=None)
def claims():
    """Everything the shapes say of themselves, on the oracle alone. -> {family: (shapes, shapes with
    isolated == 0 in reference mode, bytes the rewrites change, of those below the slot)}."""
    counts = {}
    assert 80 <= len(shapes()) <= 150 and {s.family for s in shapes()} == set(FAMILIES)
    for sh in shapes():
        name, says, h = sh.name, sh.says, out_off(sh)
        assert sh.comp.size <= 20 * 1024 + 512, name
        assert sh.cap <= 65536 or name == "cond_off_65535", name
        assert sh.cap < 32 * sh.comp.size, (name, "the small path exports blocks of ratio < 32 only")
        seqs = walk(sh)
        (sst, sw, spec), (rst, rw, ref) = expected(name, False), expected(name, True)
        want = says.get("status", OK)
        assert sst == want and rst == want, (name, sst, rst)
        if want == OK:
            assert sw == rw == sum(ll + ml for _, _, ll, _, ml, _ in seqs) and (sw > sh.cap) == bool(says.get("clip")), name
        # the number of rewrites, where the named ones lie, and the bytes they change
        rws = rewrites_of(sh)
        assert len(rws) == says["rewrites"], (name, len(rws))
        assert set(says["keys"]) <= {(k, tok) for k, tok, _, _, _ in rws}, (name, says["keys"], rws[:4])
        diff = np.nonzero(spec != ref)[0]
        assert bool(diff.size) == says["changed"], (name, diff.size)
        if says["changed"] and want == OK:
            assert 1 <= diff.size <= 3518, (name, diff.size)
        below = int((diff < h).sum())
        assert below == says.get("below", 0), (name, below)
        if h:                                       # with history only [out_off - 4, out_off) may differ from it
            assert (ref[:h - 4] == sh.history[:h - 4]).all() and (spec[:h] == sh.history).all(), name
        changed = set(diff.tolist())
        for k, tok in says["keys"]:                 # every named rewrite changes bytes of its region
            _, _, s, off, ml = next(r for r in rws if r[0] == k)
            assert changed & set(range(max(0, h + s + ml - 8), h + s)), (name, k)
        # the dependents read bytes the rewrites changed
        for d in says.get("deps", ()):
            _, tok, ll, off, ml, s = seqs[d]
            reads = set(range(h + s - off, h + min(s - off + ml, s)))
            if off >= 8 and ml < 8:                 # a rewriting dependent: its rewrite's source too
                reads |= set(range(h + s + ml - 8 - off, h + s - off))
            assert changed & reads, (name, d)
        if sh.family in NAIVE:
            assert (naive_replay(sh) != ref).any(), (name, "a naive replay gives the reference's bytes")
        _where(sh, seqs)
        # isolated
        iso = {e: isolated(sh, e) for e in MODES}
        if h or sh.dictionary is not None or says.get("reads_below"):
            assert iso[True] == CROSS, name
        else:
            assert iso == {False: want, True: want}, (name, iso)
        n, z, nd, nb = counts.get(sh.family, (0, 0, 0, 0))
        counts[sh.family] = (n + 1, z + int(iso[True] == OK), nd + int(diff.size), nb + below)
    for fam, (n, z, nd, nb) in counts.items():
        if fam not in ("history", "dictionary"):
            assert 2 * z >= n, (fam, n, z)
    _family_claims()
    return counts


def _where(sh, seqs):
    """The token offsets against CHUNK / LIM and the segment geometry."""
    name, says, where = sh.name, sh.says, sh.says.get("where")
    ends = [seqs[k + 1][1] if k + 1 < len(seqs) else int(sh.comp.size) for k in range(len(seqs))]
    toks = [q[1] for q in seqs]
    if where == "chunk0":                        # the rewriting sequences and their dependents: table sequences of chunk 0
        for k in [k for k, _ in says["keys"]] + list(says["deps"]):
            assert toks[k] < CHUNK and ends[k] <= LIM, (name, k)
    if where == "last_of_chunk0":
        (k, tok), = says["keys"]
        assert tok < CHUNK <= ends[k] <= LIM and all(toks[d] >= CHUNK for d in says["deps"]), name
    if where == "first_of_chunk1":
        (k, tok), = says["keys"]
        assert toks[k - 1] < CHUNK <= tok and ends[k - 1] <= LIM and seqs[k][2] == 0, name
        assert all(toks[d] >= CHUNK for d in says["deps"]), name
    if where == "cut":                           # starts in the first chunk, ends past the staged window
        k = says.get("cut_index", says["keys"][0][0])
        assert toks[k] < CHUNK and ends[k] > LIM and 1100 <= seqs[k][2] <= 1500, name
        assert all(toks[j] < CHUNK and ends[j] <= LIM for j in range(k)), name
        assert all(toks[d] >= toks[k] for d in says["deps"]), name
    if where == "deferred":                      # overruns the window of its chunk, fits one it starts, far from the end
        (k, tok), = says["keys"]
        assert 896 <= tok < CHUNK and ends[k] > LIM and ends[k] - tok <= LIM and sh.comp.size - ends[k] > FAST_REM, name
    if where == "segment":
        S, L = seg_geom(int(sh.comp.size))
        assert sh.comp.size == says["size"] > 8192 and S == len(says["keys"]) + 1 and S in (2, 3), name
        for j, (k, tok) in enumerate(says["keys"]):
            assert toks[k - 1] < (j + 1) * L <= tok <= (j + 1) * L + 2 and seqs[k][2] == 0, (name, k, tok)
    if "index" in says:
        (k, tok), = says["keys"]
        d1, d2 = says["deps"]
        assert k == says["index"] and d1 == k + 1 and d2 // 64 == k // 64 + 1, name
        assert (d1 // 64 == k // 64) == (k % 64 != 63), name
    if "chunks" in says:
        assert sh.comp.size > (says["chunks"] - 1) * CHUNK, name
        assert all(ll in (0, 1) and 4 <= ml <= 7 and 8 <= off <= 40 for _, _, ll, off, ml, _ in seqs[1:-1]), name
    if "period" in says:
        d, q = says["period"]
        (k, _), = says["keys"]
        s0, ml0 = seqs[k][5], seqs[k][4]
        _, _, ll, off, ml, s = seqs[d]
        assert off == q and 1 <= q <= 7 and q < ml and 40 <= ml <= 300 and s0 + ml0 - 8 <= s - q < s0, name
    if "run" in says:
        m0, q = says["run"]
        (k, _), = says["keys"]
        _, _, ll, off, ml, s = seqs[k]
        assert seqs[k - 1][3] == q and seqs[k - 1][5] == m0 and ll == 0 and ml == 4 and s - 4 >= m0, name
        assert off % q != 0 or s - off < m0, name
    if "long_match" in says:
        (k, _), = says["keys"]
        assert seqs[k - 1][4] == says["long_match"] > 256 and seqs[k - 1][3] > seqs[k - 1][4] and seqs[k][2] == 0, name
    if "clip" in says:
        assert seqs[-1][3] and seqs[-1][5] == says["match_start"] <= sh.cap == sum(q[2] + q[4] for q in seqs) - says["clip"], name
    if "spill" in says:
        _, _, ll, off, ml, s = seqs[says["spill"]]
        assert off - s == 20 and ml - 20 >= 9 and sh.dictionary.size >= 20 - (says.get("status") == DICT_OOB), name


def _family_claims():
    """What a family must hold as a whole."""
    names = {s.name for s in shapes()}
    assert {f"cond_off{o}_ml{m}" for o, m in ((8, 7), (8, 4), (7, 7), (8, 8), (9, 4))} | {"cond_off_65535", "cond_dictbranch"} <= names
    assert sorted(int(s.name.rsplit("depth", 1)[1]) for s in by_family("chain") if "ml4" in s.name) == [1, 2, 3, 8]
    assert [s.says["index"] for s in by_family("rows")] == [62, 63, 64, 65, 127, 128]
    assert sorted((s.says["below"], s.name) for s in by_family("history") if "_ll" in s.name)[-1][0] == 4
    got = {(walk(s)[0][2], walk(s)[0][4]) for s in by_family("history") if "_ll" in s.name}
    assert got == {(ll, ml) for ml in (4, 5, 6, 7) for ll in range(8 - ml)}
    for s in by_family("history"):
        if "first_byte" in s.name:
            _, _, ll, off, ml, st = walk(s)[0]
            assert off == ll + HISTORY
    st, w, ref = expected("dictionary_a", True)
    assert list(ref[5:8]) == [0, 0, 0] and ref[8] == ref[0]          # the reference's 0, not dictionary bytes
    assert [s.says.get("status", 0) for s in by_family("dictionary")].count(DICT_OOB) == 1
    assert {s.says["clip"] for s in by_family("clipped")} == {0, 1, 3, 4, 6}


# ------------------------------------------------------------------------------------------ the reference pin
def digests(shape):
    """What tests/golden/rewrite_shapes.json holds per shape: XXH32 of the block, the bytes written or the error's
    message, XXH32 of the whole array afterwards (array_for(shape): the history, then zeros) -- here from the
    oracle's reference-mode decode."""
    st, w, arr = expected(shape.name, True)
    msg = {v: k for k, v in MESSAGES.items()}
    return ["%08x" % O.xxh32(shape.comp), w if st == 0 else msg[st], "%08x" % O.xxh32(arr)]


def dump(directory):
    """The shapes for tools/golden/gen_rewrite_shapes.mjs: shapes.json and one file per distinct block, history
    and dictionary (named by its XXH32 and size)."""
    os.makedirs(directory, exist_ok=True)
    rows, written = [], set()

    def put(arr):
        if arr is None:
            return None
        name = "%08x_%d.bin" % (O.xxh32(arr), arr.size)
        if name not in written:
            np.ascontiguousarray(arr).tofile(os.path.join(directory, name))
            written.add(name)
        return name

    for s in shapes():
        rows.append({"name": s.name, "comp": put(s.comp), "out_off": out_off(s), "cap": s.cap, "history": put(s.history),
                     "dictionary": put(s.dictionary)})
    with open(os.path.join(directory, "shapes.json"), "w") as f:
        json.dump(rows, f)
    return len(rows)
