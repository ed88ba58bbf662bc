"""Shared by tests/test_literal_pieces_cpu.py and tests/test_gpu_literal_pieces.py: hand-assembled
raw blocks around the decoder's literal output (csrc/lz4mi_decompress.hip, step 6: the chunk's
literal runs of >= 16 bytes are cut into 16-byte pieces and dealt to the lanes, dealt_literals;
shorter ones go out in 8/4/2/1-byte pieces) and around the edge of the staged window (a sequence
that starts in the 1 KiB chunk and ends past the kLim = 1088 bytes staged for it is the cut
sequence, parsed from memory).

Every block's first chunk starts at compressed offset 0, so chunk-relative positions in the first
chunk are the block's own. The blocks are assembled with test_gpu_seqtable's encode/Maker; literal
bytes are random, so a misplaced piece shows.
"""
import functools

import numpy as np

import oracle as O
from test_gpu_seqtable import Maker as _Maker, encode

CHUNK = 1024              # compressed bytes parsed per step
LIM = CHUNK + 64          # kLim: chunk-relative bytes a regular sequence may touch
OK, TOO_SMALL, MALFORMED, OFFSET0 = 0, -1, -2, -3
LADDER = (1, 15, 16, 17, 31, 32, 33, 48, 255, 256, 257, 300)
LONG_ML = 4 + 15 + 255 + 40          # a match length field of two extension bytes


class Maker(_Maker):
    """test_gpu_seqtable's Maker, with the drawn offsets kept clear of the block's first bytes
    where the reference's tail rewrite (offset >= 8, match length < 8) would read below the block's
    start: batched, the reference modes refuse such a block (ERR_CROSS_BLOCK); these decode.
    With a `base` the offset is drawn a second time, from a generator of its own, over the history
    from the frame's start (the rule then holds for the frame's start): the first draw keeps the
    block's lengths and literals those of base 0."""

    def seq(self, ll, ml, off=None):
        start = self.pos + ll
        drawn = off is None
        while off is None:
            off = int(self.rng.integers(1, min(start, 65535) + 1))
            if off >= 8 and ml < 8 and start - off < 8 - ml:
                off = None
        while drawn and self.base:
            off = int(self.far.integers(1, min(self.base + start, 65535) + 1))
            drawn = off >= 8 and ml < 8 and self.base + start - off < 8 - ml
        self.pos = start + ml
        return (self.lits(ll), off, ml)


def size_of(seqs):
    return int(encode(seqs, None).size)


# ------------------------------------------------------------------------------------ length ladder
def cases_ladder(base=0):
    """Literal runs of every LADDER length, each followed by a short match into older output:
    all of them in one block, and each alone at the head of a block of its own."""
    out = {}
    m = Maker(7000, base)
    seqs = []
    for n in LADDER:
        seqs.append(m.seq(n, int(m.rng.integers(4, 19))))
    out["ladder_all"] = (seqs + m.short(4), m.lits(5), None)
    for n in LADDER:
        m = Maker(7000 + n, base)
        out[f"ladder_{n}"] = (m.short(3) + [m.seq(n, 6)] + m.short(5), m.lits(3), None)
    return out


# -------------------------------------------------------------------------------------- list limits
def cases_limits(base=0):
    """max_runs: the most runs of >= 16 bytes a chunk can hold (16 literals and a 4-byte match:
    20 compressed bytes, 52 tokens in the first KiB). late_runs: a 4-byte sequence, 256 three-byte
    ones, then ten with 17 literals -- the literal-bearing sequences lie in row 4 (index >= 256),
    all in the first chunk. mixed_rows: runs of 16..80 bytes among short ones over three rows."""
    out = {}
    m = Maker(7100, base)
    out["max_runs"] = ([m.seq(16, 4) for _ in range(60)], m.lits(16), None)
    m = Maker(7101, base)
    seqs = [m.seq(1, 8)] + [m.seq(0, int(m.rng.integers(4, 19))) for _ in range(256)]
    seqs += [m.seq(17, 5) for _ in range(10)]
    out["late_runs"] = (seqs, m.lits(4), None)
    m = Maker(7102, base)
    seqs = []
    for k in range(150):
        seqs.append(m.seq(int(m.rng.integers(16, 81)), 5) if k % 13 == 5 else m.seq(1, 7))
    out["mixed_rows"] = (seqs, m.lits(20), None)
    return out


# ------------------------------------------------------------------------------------- output edges
FINALS = (16, 17, 23, 31, 32, 33, 40, 100, 250)


def cases_edges(base=0):
    """A final literal-only sequence of n bytes that ends exactly at out_cap (the decoded size),
    after a few short sequences; and the same behind a 37-byte run."""
    out = {}
    for n in FINALS:
        m = Maker(7200 + n, base)
        out[f"final_{n}"] = (m.short(5), m.lits(n), None)
        m = Maker(7300 + n, base)
        out[f"final_{n}_after_run"] = (m.short(2) + [m.seq(37, 4)], m.lits(n), None)
    return out


# --------------------------------------------------------------------- remap into dealt literal runs
def _remap(seed, ml, nl, second_chunk, base=0):
    """A literal run of `run` bytes at output a, its own match, then a match of ml bytes whose source
    starts nl bytes before the run's end: nl = None -> wholly inside the run; else it goes on into
    the run's own match (the split case). second_chunk: 256 four-byte sequences first, so the
    chunk in question starts at compressed offset 1024 and the run's own match reads output
    finished by the chunk before."""
    m = Maker(seed, base)
    seqs = m.short(256 if second_chunk else 3)
    run = max(64, ml + 8) if nl is None else 64
    a = m.pos
    own = max(24, ml)                                   # the run's own match
    seqs.append(m.seq(run, own, off=int(m.rng.integers(run + own, a + run + 1)) if second_chunk else None))
    ms = m.pos + 1                                      # where the remapped match starts
    src = a + 3 if nl is None else a + run - nl
    seqs.append(m.seq(1, ml, off=ms - src))
    return seqs + m.short(6), m.lits(4), None


def cases_remap(base=0):
    out = {}
    for chunk in (0, 1):
        for ml in (16, 17, 40, 255):
            out[f"remap_inside_{ml}_c{chunk}"] = _remap(7400 + ml + chunk, ml, None, bool(chunk), base)
            for nl in (5, 16, 40):
                if nl < ml:
                    out[f"remap_split_{ml}_{nl}_c{chunk}"] = _remap(7500 + ml + 3 * nl + chunk, ml, nl, bool(chunk), base)
    return out


# ------------------------------------------------------------------------- errors on a mid-length run
def cases_errors(base=0):
    """Valid four-byte sequences, then a 100-byte literal run that overruns the input (-2), that
    the capacity cuts one byte short and in its middle (-1), and whose match has offset 0 (-3)."""
    out = {}
    m = Maker(7600, base)
    head = m.short(20)
    before = m.pos
    seqs = head + [m.seq(100, 6)] + m.short(5)
    fin = m.lits(4)
    out["run_overruns_input"] = (seqs, fin, m.pos + 4, {"truncate": size_of(head) + 2 + 50, "want": MALFORMED})
    out["cap_one_short_of_run"] = (seqs, fin, before + 99, {"want": TOO_SMALL})
    out["cap_in_middle_of_run"] = (seqs, fin, before + 50, {"want": TOO_SMALL})
    m = Maker(7601, base)
    seqs = m.short(20) + [m.seq(100, 6, off=0)] + m.short(5)
    out["offset0_after_run"] = (seqs, m.lits(4), m.pos + 4, {"want": OFFSET0})
    return out


# -------------------------------------------------------------------------------------- window edge
TOKENS = (1023, 1000, 828)
LANDS = (LIM - 1, LIM, LIM + 1, LIM + 40)


def head_to(m, size):
    """Four-byte sequences, then up to three three-byte ones: `size` compressed bytes in all."""
    b = (3 * size) % 4                                   # 4 a + 3 b = size
    a = (size - 3 * b) // 4
    assert a >= 1 and 4 * a + 3 * b == size, size
    return m.short(a) + [m.seq(0, int(m.rng.integers(4, 19))) for _ in range(b)]


def edge_seq(m, span, ml):
    """A sequence with literals that takes `span` compressed bytes."""
    mlx = 0 if ml - 4 < 15 else 1 + (ml - 19) // 255
    for ll in range(1, 2000):
        if 1 + (0 if ll < 15 else 1 + (ll - 15) // 255) + ll + 2 + mlx == span:
            return m.seq(ll, ml)
    raise AssertionError((span, ml))


def cases_window(base=0):
    """Tokens at chunk offset 1023, 1000 and 828 whose literal sequence puts the next token at
    kLim - 1, kLim, kLim + 1 and kLim + 40: followed by more sequences, last in the block (before
    the final literals, and ending the block on its match), and with a match length field of two
    extension bytes (away from the block's end: the fast next-token table's redo). twice_*: two such
    sequences in consecutive chunks. first_too_long: a 1100-byte literal run at chunk offset 0,
    which no window holds."""
    out = {}
    for tok in TOKENS:
        for land in LANDS:
            for kind in ("mid", "last", "ends", "ml2"):
                m = Maker(7700 + tok + 7 * land + len(kind), base)
                seqs = head_to(m, tok) + [edge_seq(m, land - tok, LONG_ML if kind == "ml2" else 9)]
                if kind in ("mid", "ml2"):
                    seqs += m.short(450)
                fin = None if kind == "ends" else m.lits(5)
                out[f"edge_{tok}_{land}_{kind}"] = (seqs, fin, None, {"token": tok, "land": land})
    for tok in (1000, 828):
        m = Maker(7800 + tok, base)
        seqs = head_to(m, tok) + [edge_seq(m, LIM + 40 - tok, 9)]      # the next chunk starts at LIM + 40 ...
        seqs += head_to(m, tok) + [edge_seq(m, LIM + 1 - tok, 9)]      # ... or, deferred, at the token: tok + 100 more
        out[f"twice_{tok}"] = (seqs + m.short(300), m.lits(5), None, {})
    m = Maker(7900, base)
    out["first_too_long"] = ([m.seq(1100, 8)] + m.short(70), m.lits(6), None, {"token": 0, "land": 1 + 5 + 1100 + 2})
    return out


# ----------------------------------------------------------------------------------------- all of them
def raw_cases(base=0):
    """name -> (sequences, final literals, capacity or None, options)."""
    cases = {}
    for group in (cases_ladder(base), cases_limits(base), cases_edges(base), cases_remap(base), cases_errors(base),
                  cases_window(base)):
        for name, c in group.items():
            assert name not in cases
            cases[name] = c if len(c) == 4 else c + ({},)
    return cases


@functools.lru_cache(maxsize=None)
def all_cases():
    """name -> (compressed block, capacity, options, {js: the oracle's (status, written, bytes)})."""
    done = {}
    for name, (seqs, fin, cap, opts) in raw_cases().items():
        comp = encode(seqs, fin, opts.get("truncate"))
        if cap is None:
            st, cap, _ = O.decompress_block(comp, 1 << 17)
            assert st == 0 and cap <= (1 << 17), name
        ref = {js: O.decompress_block(comp, cap, js_compat=js) for js in (False, True)}
        done[name] = (comp, cap, opts, ref)
    return done


def expected_bytes(seqs, fin):
    """What the sequences say, decoded by hand (byte-wise match copies)."""
    out = bytearray()
    for lits, off, ml in seqs:
        out += lits
        for _ in range(ml):
            out.append(out[-off])
    if fin is not None:
        out += fin
    return np.frombuffer(bytes(out), dtype=np.uint8)


def tokens_of(comp):
    """Compressed offsets of the block's tokens."""
    c = [int(x) for x in comp]
    ip, toks = 0, []
    while ip < len(c):
        toks.append(ip)
        tok = c[ip]
        ip += 1
        ll = tok >> 4
        if ll == 15:
            while True:
                b = c[ip]
                ip += 1
                ll += b
                if b != 255:
                    break
        ip += ll
        if ip >= len(c):
            break
        ip += 2
        if tok & 15 == 15:
            while c[ip] == 255:
                ip += 1
            ip += 1
    return toks
