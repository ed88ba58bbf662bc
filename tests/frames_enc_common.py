"""Shared by tests/test_frames_compress_cpu.py and tests/test_gpu_frames_compress.py: a zoo of contents for the
frame batch encoder (lz4mi_frames_plan / lz4mi_frames_compress and their host twins), read-only, their block
shapes asserted against the CPU oracle so that a change in the oracle cannot hollow the tests out.

  group "b64k" (block_max 65536): lengths 0, 1, 12, 13 and 40 (no block / one stored block); text of 100, 300 and
      4000 bytes and repetitive of 600 (one compressed block); random of 65536 (stored); tiles216 of 65535, 65536
      and 65537 (the last a compressed block plus a stored block of one byte); verify_common.data() (five blocks,
      one of them stored);
  group "b4m" (block_max 4194304): tiles216 of 4 MiB + 1 (two blocks), text of 300;
  group "b256k" (block_max 65537, which resolves to 256 KiB): tiles216 of 256 KiB + 1 (two blocks), text of 4000.
arena(group, fill): the group's sources in one array at start residues 0 - 3 (mod 4) in turn, 5 to 8 filler bytes
between two. expected(...): the frame the reference writes (the oracle's), or with block checksums the frame
assembled from frame.header and the oracle's blocks; None for a dependent frame of more than one block.
"""
import functools
import itertools

import numpy as np

import oracle as O
import verify_common as V
from lz4mi import frame as F
from lz4mi import shard

FILLS = (0x00, 0xFF)
(CAP_BLOCKS, PAST_END, EMPTY, UNSIZED_EXACT, MEASURE, SIZE_MISMATCH, OUT_CAP, LAYOUT, DEPENDENT, HASH_4G) = range(1, 11)
# name -> (generator, seed, length); "five" is verify_common.data()
CONTENTS = {"n0": ("text", 3, 0), "n1": ("text", 3, 1), "n12": ("text", 3, 12), "n13": ("text", 3, 13),
            "n40": ("text", 3, 40), "text100": ("text", 3, 100), "text300": ("text", 3, 300),
            "text4000": ("text", 3, 4000), "rep600": ("repetitive", 1, 600), "rand64k": ("random", 2, 65536),
            "tiles65535": ("tiles216", 45, 65535), "tiles65536": ("tiles216", 46, 65536),
            "tiles65537": ("tiles216", 47, 65537), "five": None,
            "tiles4m1": ("tiles216", 5, 4194305), "tiles256k1": ("tiles216", 6, 262145)}
# group -> (block_max as the caller passes it, the resolved block size, the contents in arena order)
GROUPS = {"b64k": (65536, 65536, ("n0", "n1", "n12", "n13", "n40", "text100", "text300", "text4000", "rep600",
                                   "rand64k", "tiles65535", "tiles65536", "tiles65537", "five")),
          "b4m": (4194304, 4194304, ("tiles4m1", "text300")),
          "b256k": (65537, 262144, ("tiles256k1", "text4000"))}
# the blocks of each content at its group's block size, as stored flags (asserted in shapes())
SHAPES = {"n0": (), "n1": (True,), "n12": (True,), "n13": (True,), "n40": (True,), "text100": (False,),
          "text300": (False,), "text4000": (False,), "rep600": (False,), "rand64k": (True,),
          "tiles65535": (False,), "tiles65536": (False,), "tiles65537": (False, True),
          "five": (False, False, True, False, False), "tiles4m1": (False, True), "tiles256k1": (False, True)}
# (independent, content_checksum, add_content_size, block_checksum)
COMBOS = tuple(itertools.product((True, False), (False, True), (True, False), (False, True)))


def combo_id(c):
    return "".join(ch if on else "-" for ch, on in zip("icsb", c))


@functools.lru_cache(maxsize=None)
def content(name):
    c = V.data() if CONTENTS[name] is None else O.generate(*CONTENTS[name])
    c = np.ascontiguousarray(c, dtype=np.uint8)
    c.setflags(write=False)
    return c


def _le32(x):
    return np.array([x & 0xFFFFFFFF], dtype="<u4").view(np.uint8)


@functools.lru_cache(maxsize=None)
def records(name, bs):
    """[(size word, payload)] of the content's independent blocks, by the oracle's block encoder."""
    c, recs = content(name), []
    for p in range(0, c.size, bs):
        raw = c[p:p + bs]
        comp = O.compress_block_bytes(raw)
        recs.append((comp.size, comp) if 0 < comp.size < raw.size else (raw.size | 0x80000000, raw))
    return recs


@functools.lru_cache(maxsize=None)
def expected(name, bs, combo):
    indep, csum, sized, bsum = combo
    c = content(name)
    if not indep and c.size > bs:
        return None
    if not bsum:
        f = O.compress_frame(c, None, bs, indep, csum, sized)
    else:
        parts = [np.frombuffer(F.header(bs, indep, csum, c.size if sized else None, None, True), dtype=np.uint8)]
        for word, pay in records(name, bs):
            parts += [_le32(word), pay, _le32(O.xxh32_std(pay))]
        parts.append(_le32(0))
        if csum:
            parts.append(_le32(O.xxh32(c)))
        f = np.concatenate(parts)
    f = np.ascontiguousarray(f, dtype=np.uint8)
    f.setflags(write=False)
    return f


@functools.lru_cache(maxsize=None)
def shapes():
    """Asserts the zoo's shapes on the oracle's frames; -> {name: compressed sizes of its blocks}."""
    sizes = {}
    for group, (_, bs, names) in GROUPS.items():
        for name in names:
            f = expected(name, bs, (True, True, True, False))
            info, blocks = shard.frame_blocks(f)
            assert tuple(st for _, _, st in blocks) == SHAPES[name], (group, name, blocks)
            assert info["block_max"] == bs and info["content_size"] == content(name).size, (group, name)
            # the reference's default (dependent blocks) writes the same single-block frame but for FLG and HC
            if content(name).size <= bs:
                d = expected(name, bs, (False, True, True, False))
                assert d.size == f.size and d[4] == f[4] ^ 0x20 and set(np.nonzero(d != f)[0].tolist()) <= {4, 14}, (group, name)
            sizes[name] = [n for _, n, _ in blocks]
    assert (sizes["text100"], sizes["text300"], sizes["text4000"]) == ([92], [243], [2671])
    assert sizes["tiles65537"][1] == 1 and sizes["tiles4m1"][1] == 1 and sizes["tiles256k1"][1] == 1
    return sizes


@functools.lru_cache(maxsize=None)
def arena(group, fill):
    """-> (arena, offsets, lengths): the group's sources at start residues 0, 1, 2, 3 (mod 4) in turn."""
    names = GROUPS[group][2]
    offs, at = [], 64
    for k, name in enumerate(names):
        at += 5
        at += (k % 4 - at) % 4
        offs.append(at)
        at += content(name).size
    a = np.full(at + 64, fill, dtype=np.uint8)
    for o, name in zip(offs, names):
        a[o:o + content(name).size] = content(name)
    a.setflags(write=False)
    return a, np.array(offs, dtype=np.uint64), np.array([content(n).size for n in names], dtype=np.uint64)


def slot_bytes(n):
    return (n + n // 255 + 16 + 15) & ~15


def closed_form_plan(lens, offs, bs, combo, cap):
    """lz4mi_frames_plan in a few lines: -> (finfo rows, totals, blk_in_off, blk_len, blk_frame, blk_work_off)."""
    indep, csum, sized, bsum = combo
    flg = 0x40 | (0x20 if indep else 0) | (0x10 if bsum else 0) | (0x08 if sized else 0) | (0x04 if csum else 0)
    bd = {65536: 4, 262144: 5, 1048576: 6, 4194304: 7}[bs] << 4
    rows, lists, first, slot, out = [], ([], [], [], []), 0, 16, 0
    for f, (n, off) in enumerate(zip(lens, offs)):
        count = -(-n // bs)
        decline = DEPENDENT if (not indep and count > 1) else HASH_4G if (csum and n >= 2 ** 32) else 0
        rows.append([0, flg | bd << 8, n, 23 + n + 8 * count, first, 0, count, decline])
        if decline:
            continue
        if first + count <= cap:
            for k in range(count):
                ln = min(bs, n - k * bs)
                for lst, v in zip(lists, (off + k * bs, ln, f, slot + sum(slot_bytes(min(bs, n - j * bs)) for j in range(k)))):
                    lst.append(v)
        elif count:
            rows[-1][7] = CAP_BLOCKS
        first += count
        slot += sum(slot_bytes(min(bs, n - k * bs)) for k in range(count))
    totals = [first, len(lists[0]), sum(r[3] for r in rows if not r[7]), slot]
    return (rows, totals) + lists
