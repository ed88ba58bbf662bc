"""Shared inputs of the decoded-size tests (test_sizes_cpu.py, test_gpu_sizes.py): an
independent pure-Python token walker restating blockDecompress.js:55-139 without the copies,
a sequence emitter for hand-built streams, and the prefix / mutation sets of two blocks."""
import functools
import re

import numpy as np

import oracle as O

MAX_BLOCK = 0x7FFFFFFF
GENERATOR_KINDS = ("tiles216", "random", "repetitive", "text", "copy", "runs")
SOURCE_SIZES = (0, 1, 12, 13, 64, 1000, 65536, 777777)


_RUN255 = re.compile(b"\xff*")


def _field_at(b, pos, n):
    """(sum, position after) of the length-field tail at pos: a run of 255s and the byte ending it."""
    if pos >= n:
        return 0, pos + 1
    end = _RUN255.match(b, pos).end()
    return 255 * (end - pos) + (b[end] if end < n else 0), end + 1


def walk(comp):
    """(status, size) of one block: the reference's loop, bytes past the end read as 0
    (`undefined | 0`), lengths unbounded; above 2^31 - 1: (-1, 0x7FFFFFFF)."""
    b = bytes(comp)
    n = len(b)
    pos = total = 0
    st = 0
    while pos < n:
        tok = b[pos]
        pos += 1
        ll = tok >> 4
        if ll == 15:
            s, pos = _field_at(b, pos, n)
            ll += s
        if pos + ll > n:
            st = -2
            break
        total += ll
        pos += ll
        if pos >= n:
            break
        if b[pos] == 0 and (b[pos + 1] if pos + 1 < n else 0) == 0:
            st = -3
            break
        pos += 2
        ml = tok & 15
        if ml == 15:
            s, pos = _field_at(b, pos, n)
            ml += s
        total += ml + 4
    if total > MAX_BLOCK:
        return -1, MAX_BLOCK
    return st, total


def _field(n):
    """The extension bytes of a length field whose nibble is 15 (n >= 15)."""
    n -= 15
    return b"\xff" * (n // 255) + bytes([n % 255])


def seq(ll, ml=None, off=1, fill=0x41):
    """One sequence: ll literal bytes, then (ml is not None) a match of ml >= 4 bytes at `off`."""
    code = 0 if ml is None else ml - 4
    out = bytearray([(min(ll, 15) << 4) | min(code, 15)])
    if ll >= 15:
        out += _field(ll)
    out += bytes([fill]) * ll
    if ml is not None:
        out += bytes([off & 255, off >> 8])
        if code >= 15:
            out += _field(code)
    return bytes(out)


def ext_len(k, last=7):
    """A length whose field has exactly k extension bytes (k = 0: the nibble alone)."""
    return 9 if k == 0 else 15 + 255 * (k - 1) + last


def arr(b):
    return np.frombuffer(bytes(b), dtype=np.uint8)


@functools.lru_cache(maxsize=None)
def base_blocks():
    """The two blocks the prefixes and mutations are made from (5 301 and 6 258 bytes)."""
    return tuple(O.compress_block_bytes(O.generate(kind, 11, 8192)) for kind in ("text", "tiles216"))


@functools.lru_cache(maxsize=None)
def prefixes():
    """Every prefix of the two blocks, from the empty one to the whole block (11 561 in all)."""
    return tuple(c[:n] for c in base_blocks() for n in range(c.size + 1))


@functools.lru_cache(maxsize=None)
def mutations():
    """2 000 copies of each block with 1-3 random byte replacements: (text ones, tiles216 ones)."""
    rng = np.random.default_rng(7)
    out = []
    for c in base_blocks():
        muts = []
        for _ in range(2000):
            m = c.copy()
            for _ in range(int(rng.integers(1, 4))):
                m[int(rng.integers(0, m.size))] = int(rng.integers(0, 256))
            muts.append(m)
        out.append(tuple(muts))
    return tuple(out)


def _pad_to(out, target):
    """Short sequences (3 to 5 bytes each) until len(out) == target (target - len(out) >= 3)."""
    while len(out) < target:
        d = target - len(out)
        out += seq(0, 4, 1) if d == 3 or d >= 6 else seq(d - 3, 4, 1)
    assert len(out) == target


@functools.lru_cache(maxsize=None)
def chunk_edge_blocks():
    """Blocks in which one sequence's token, literal-length field, offset or match-length field
    starts at a compressed offset around a 1 KiB chunk edge or the end of its 64-byte lookahead,
    at the first edge (1024) and the second (1026 + 1024: runs of 3-byte sequences put the
    second chunk's first token at 1026), with length fields of 0, 1, 2 and 300 extension bytes."""
    blocks = []
    for base in (0, 1026):
        for t in [base + x for x in (*range(1020, 1029), *range(1084, 1093))]:
            for which in range(4):
                for k in (0, 1, 2, 300):
                    kl = k if which < 2 else 0
                    ll = ext_len(kl) if kl else 2
                    # token | literal field (kl) | literals (ll) | offset (2) | match field (k)
                    start = t - (0, 1, 1 + kl + ll, 3 + kl + ll)[which]
                    out = bytearray()
                    _pad_to(out, start)
                    out += seq(ll, ext_len(k) + 4, 3)
                    out += seq(1, 5, 2) + seq(3)
                    blocks.append(arr(out))
    return tuple(blocks)
