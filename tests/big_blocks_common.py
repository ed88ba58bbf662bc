"""Shared by tests/test_big_blocks_cpu.py and tests/test_gpu_big_blocks.py: raw blocks far above the reference's
4 MiB block size, up to LZ4MI_MAX_BLOCK = 2^31 - 1 decoded bytes (include/lz4mi.h: "raw calls may pass more").

The batch decoder (csrc/lz4mi_decompress.hip) keeps block-relative output positions in int32 and packs remapped match
sources into tagged 32-bit fields (SeqInfo::rsrc: kMemoBase, kSplitBase), so a block is placed with its interesting
part -- the body -- across the positions where those fields change meaning.

A block is hand-assembled, so its compressed form stays at a few MiB:
    prefix  one sequence: `per` random literals, then a match at offset `per` of target - per bytes. It brings the
            output to exactly `target` bytes of a periodic image, np.resize(literals, target). per = 64, or 65535 (a
            period longer than the decoder's LDS pattern buffer: periodic_run's phase slices);
    body    the oracle encoder's block of 1 to 2 MiB of tiles216 (split remaps), text (short sequences, deep chains)
            or copy (reference tail rewrites that change bytes), appended verbatim: its offsets are relative, so the
            concatenation is a valid block of n = target + body_n bytes.
target = T - body_n // 2 + an odd number puts the body across a threshold T (THRESHOLDS); `inside` puts it wholly
inside [2^29, 2^29 + 2^27), where a split mapping's tagged value lay inside the whole-match memo window; `top` ends
the body on byte 2^31 - 2, the last one the ABI allows (n == out_cap == 0x7FFFFFFF).

The expected image, by construction: np.resize(literals, target), then the oracle's decode of the body alone over a
64 KiB history window holding the image's last 64 KiB (Block.tail). tests/test_big_blocks_cpu.py checks that claim
against a full oracle decode of the assembled block, in spec and reference mode.
"""
import functools

import numpy as np

import oracle as O
from linked_exact_common import parse

OK, TOO_SMALL = 0, -1
MAX_BLOCK = 0x7FFFFFFF
PERIODS = (64, 65535)
# kind -> (body bytes: 1 to 2 MiB, no multiple of 16; generator seed)
BODIES = {"tiles216": ((1 << 20) + 12345, 9), "text": ((1 << 20) + (1 << 19) + 777, 4), "copy": ((2 << 20) - 5, 6)}
KINDS = tuple(BODIES)
assert all((1 << 20) <= n <= (2 << 20) and n % 16 for n, _ in BODIES.values())
THRESHOLDS = {"2^27": 1 << 27, "2^29-64K": (1 << 29) - 65536, "2^29+2^27": (1 << 29) + (1 << 27), "2^30": 1 << 30}
# case -> its blocks (kind, period); both periods and all three kinds at every threshold
CASES = {"2^27": (("tiles216", 64), ("text", 65535), ("copy", 64)),
         "2^29-64K": (("tiles216", 65535), ("text", 64), ("copy", 65535)),
         "2^29+2^27": (("tiles216", 64), ("text", 65535), ("copy", 64)),
         "2^30": (("tiles216", 65535), ("text", 64), ("copy", 65535)),
         "inside": (("tiles216", 64), ("tiles216", 65535), ("text", 64))}
TOP = (("text", 64), ("tiles216", 65535))       # two blocks at most: 2 GiB each
FILLER_N = 13


def len_field(v):
    """Extension bytes of an LZ4 length field whose value beyond the token's 15 is v."""
    return np.concatenate([np.full(v // 255, 255, dtype=np.uint8), np.array([v % 255], dtype=np.uint8)])


@functools.lru_cache(maxsize=None)
def body(kind):
    """-> (source, the oracle encoder's block of it)."""
    n, seed = BODIES[kind]
    src = O.generate(kind, seed, n)
    return src, O.compress_block_bytes(src)


@functools.lru_cache(maxsize=None)
def literals(per):
    return O.generate("random", 100 + per, per)


def prefix(per, target):
    lits = literals(per)
    assert per >= 15 and target - per >= 19
    return np.concatenate([np.array([0xFF], dtype=np.uint8), len_field(per - 15), lits,
                           np.array([per & 255, per >> 8], dtype=np.uint8), len_field(target - per - 19)])


def one_more_literal(comp):
    """The block with one more byte in its last (literal-only) sequence."""
    lp, ll, off, ml = parse(comp)[-1]
    assert off == 0 and ml == 0 and lp + ll == comp.size and ll >= 5
    tok = lp - 1 - ((ll - 15) // 255 + 1 if ll >= 15 else 0)
    lits = np.concatenate([comp[lp:], np.array([0x5A], dtype=np.uint8)])
    head = [min(ll + 1, 15) << 4]
    ext = len_field(ll + 1 - 15) if ll + 1 >= 15 else np.zeros(0, dtype=np.uint8)
    return np.concatenate([comp[:tok], np.array(head, dtype=np.uint8), ext, lits])


class Block:
    """One assembled block: comp, n = target + body_n decoded bytes, and the pieces of its expected image."""

    def __init__(self, kind, per, target, longer=False):
        self.kind, self.per, self.target = kind, per, int(target)
        src, comp = body(kind)
        self.body_src = src
        self.body = one_more_literal(comp) if longer else comp
        self.body_n = src.size + (1 if longer else 0)
        self.n = self.target + self.body_n
        self.comp = np.concatenate([prefix(per, self.target), self.body])
        self.name = f"{kind}/per{per}@{self.target}"
        self._tails = {}

    def history(self):
        """The last 64 KiB of the periodic image below the body."""
        assert self.target >= 65536
        return literals(self.per)[(self.target - 65536 + np.arange(65536, dtype=np.int64)) % self.per]

    def tail(self, js):
        """The body's decoded bytes: the oracle's decode of the body alone behind history()."""
        js = bool(js)
        if js not in self._tails:
            hist = self.history()
            buf = np.concatenate([hist, np.zeros(self.body_n, dtype=np.uint8)])
            st, w, out = O.decompress_block(self.body, 0, out=buf, out_off=65536, js_compat=js)
            assert st == 0 and w == self.body_n, (self.name, st, w)
            assert np.array_equal(out[:65536], hist), (self.name, "the decode changed bytes below the body")
            self._tails[js] = out[65536:].copy()
        return self._tails[js]

    def image(self, js):
        """The whole expected image (small targets only)."""
        return np.concatenate([np.resize(literals(self.per), self.target), self.tail(js)])

    def where(self, pos):
        """An output position, named: in the prefix (with its phase), or the body's sequence that wrote it."""
        if pos < self.target:
            return f"prefix image, phase {pos % self.per} of {self.per}"
        at, k = self.target, 0
        for k, (lp, ll, off, ml) in enumerate(parse(self.body)):
            if pos < at + ll + ml:
                part = "literals" if pos < at + ll else "match"
                return (f"body byte {pos - self.target}, sequence {k} ({part}): out {at}, ll {ll}, off {off}, ml {ml}, "
                        f"match at {at + ll}, source {at + ll - off}")
            at += ll + ml
        return f"past the body's last sequence {k}"


def _odd(k):
    return 1 + 2 * (k % 3)


def target_at(T, kind, k=0):
    """The body of `kind` astride T."""
    return T - BODIES[kind][0] // 2 + _odd(k)


@functools.lru_cache(maxsize=None)
def case(name):
    """-> the blocks of a case (THRESHOLDS, "inside", "top")."""
    if name == "top":
        return tuple(Block(kind, per, MAX_BLOCK - BODIES[kind][0]) for kind, per in TOP)
    if name == "inside":
        return tuple(Block(kind, per, (1 << 29) + (1 << 26) + _odd(k)) for k, (kind, per) in enumerate(CASES[name]))
    return tuple(Block(kind, per, target_at(THRESHOLDS[name], kind, k)) for k, (kind, per) in enumerate(CASES[name]))


def check_case(name):
    """The placement a case's name promises."""
    for b in case(name):
        lo, hi = b.target, b.n
        if name == "top":
            assert hi == MAX_BLOCK
        elif name == "inside":
            assert (1 << 29) <= lo and hi <= (1 << 29) + (1 << 27)
        else:
            T = THRESHOLDS[name]
            assert lo + 65536 < T < hi - 65536, (name, b.name)


def too_long():
    """The first block of `top` with one more byte in the body's last literal run: 2^31 bytes, one more than any
    capacity."""
    kind, per = TOP[0]
    b = Block(kind, per, MAX_BLOCK - BODIES[kind][0], longer=True)
    assert b.n == MAX_BLOCK + 1
    return b


@functools.lru_cache(maxsize=None)
def filler():
    """-> (source, block) of a 13-byte block."""
    src = O.generate("text", 3, FILLER_N)
    return src, O.compress_block_bytes(src)


def small_block(kind, per, k=0):
    """The same construction at target ~ 2^20, for the construction claim."""
    return Block(kind, per, (1 << 20) + 3 + 2 * k)
