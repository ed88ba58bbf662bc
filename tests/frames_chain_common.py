"""Shared by tests/test_frames_chains_cpu.py and tests/test_gpu_frames_chains.py: a zoo of contents for the chains
of the frame batch encoder (LZ4MI_FRAMES_DEPENDENT | LZ4MI_FRAMES_CHAINS: a dependent frame of more than one block,
one hash table carried across its blocks), read-only, each content's claim asserted on the CPU oracle's own frame
so that a change in the oracle cannot hollow the tests out.

  group "c64k" (block_max 65536), chains and batch-encoder frames in turn:
      text4       text of 3 x 65536 + 100: matches reach into the block before (the dependent frame is shorter than
                  the independent one and differs beyond FLG / HC);
      rep2        repetitive of 131072 + 13: block 1 starts with a match whose source lies in block 0, the 13-byte
                  last block is stored;
      randtail    65536 random bytes, their last 30000 again, then text up to 131072 + 5000: block 0 is stored and
                  block 1 matches into the stored block's raw bytes;
      r65535x3    65535 random bytes three times over: every cross-block candidate at distance 65535, the largest
                  offset; blocks 1 and 2 are compressed;
      r65536x3    65536 random bytes three times over: distance 65536, one past the window; every block stored;
      tiles300k   tiles216 of 300000: more than three laps of the chain kernel's 88 KiB source ring, at a base
                  that is not 16-aligned;
      n0, n13, text300, rand64k: no block / one block (the batch encoder's frames in the same call);
  group "c256k" (block_max 65537, which resolves to 256 KiB): n13, text of 262144 + 4000;
  group "c4m" (block_max 4194304): text300, tiles216 of 4194304 + 70000.
arena(group, fill): the group's sources in one array at start residues 0, 1, 7, 15 (mod 16) in turn, at least 5
filler bytes between two (5 to 20: the residue is exact, so the gap follows from the lengths).
expected(name, bs, combo): the frame the reference writes with blockIndependence = false (the oracle's), or with
block checksums that frame's records behind frame.header(block_checksum=True), each followed by the spec XXH32 of
its payload.
"""
import functools
import itertools

import numpy as np

import oracle as O
from lz4mi import frame as F
from lz4mi import shard

FILLS = (0x00, 0xFF)
RESIDUES = (0, 1, 7, 15)
RING_BYTES = 88 * 1024   # the chain kernels' source ring (csrc/lz4mi_compress.hip kRingBytes)
(CAP_BLOCKS, PAST_END, EMPTY, UNSIZED_EXACT, MEASURE, SIZE_MISMATCH, OUT_CAP, LAYOUT, DEPENDENT, HASH_4G) = range(1, 11)
# group -> (block_max as the caller passes it, the resolved block size, the contents in arena order)
GROUPS = {"c64k": (65536, 65536, ("text4", "n0", "rep2", "randtail", "n13", "r65535x3", "text300", "r65536x3",
                                   "rand64k", "tiles300k")),
          "c256k": (65537, 262144, ("n13", "text266k")),
          "c4m": (4194304, 4194304, ("text300", "tiles4m70k"))}
# the blocks of each content in its group's dependent frame, as stored flags (asserted in shapes())
SHAPES = {"text4": (False, False, False, False), "n0": (), "rep2": (False, False, True),
          "randtail": (True, False, False), "n13": (True,), "r65535x3": (True, False, False), "text300": (False,),
          "r65536x3": (True, True, True), "rand64k": (True,), "tiles300k": (False,) * 5,
          "text266k": (False, False), "tiles4m70k": (False, False)}
# (content_checksum, add_content_size, block_checksum)
COMBOS = tuple(itertools.product((False, True), (True, False), (False, True)))


def combo_id(c):
    return "".join(ch if on else "-" for ch, on in zip("csb", c))


def _build(name):
    g = O.generate
    if name == "text4":
        return g("text", 11, 3 * 65536 + 100)
    if name == "rep2":
        return g("repetitive", 1, 131072 + 13)
    if name == "randtail":
        r = g("random", 21, 65536)
        return np.concatenate([r, r[-30000:], g("text", 12, 131072 + 5000 - 65536 - 30000)])
    if name == "r65535x3":
        return np.tile(g("random", 22, 65535), 3)
    if name == "r65536x3":
        return np.tile(g("random", 23, 65536), 3)
    if name == "tiles300k":
        return g("tiles216", 48, 300000)
    if name == "text266k":
        return g("text", 13, 262144 + 4000)
    if name == "tiles4m70k":
        return g("tiles216", 7, 4194304 + 70000)
    return g(*{"n0": ("text", 3, 0), "n13": ("text", 3, 13), "text300": ("text", 3, 300),
               "rand64k": ("random", 2, 65536)}[name])


@functools.lru_cache(maxsize=None)
def content(name):
    c = np.ascontiguousarray(_build(name), dtype=np.uint8)
    c.setflags(write=False)
    return c


def _le32(x):
    return np.array([x & 0xFFFFFFFF], dtype="<u4").view(np.uint8)


def _frozen(f):
    f = np.ascontiguousarray(f, dtype=np.uint8)
    f.setflags(write=False)
    return f


@functools.lru_cache(maxsize=None)
def oracle_frame(name, bs, indep, csum, sized):
    return _frozen(O.compress_frame(content(name), None, bs, indep, csum, sized))


@functools.lru_cache(maxsize=None)
def expected(name, bs, combo):
    csum, sized, bsum = combo
    f = oracle_frame(name, bs, False, csum, sized)
    if not bsum:
        return f
    c = content(name)
    _, blocks = shard.frame_blocks(f)
    parts = [np.frombuffer(F.header(bs, False, csum, c.size if sized else None, None, True), dtype=np.uint8)]
    for pos, n, st in blocks:
        pay = f[pos:pos + n]
        parts += [f[pos - 4:pos], pay, _le32(O.xxh32_std(pay))]
    parts.append(_le32(0))
    if csum:
        parts.append(_le32(O.xxh32(c)))
    return _frozen(np.concatenate(parts))


def first_match(payload):
    """(literal count, offset) of a compressed block's first sequence."""
    p = 1
    lit = int(payload[0]) >> 4
    if lit == 15:
        while True:
            v = int(payload[p])
            p += 1
            lit += v
            if v != 255:
                break
    p += lit
    return lit, int(payload[p]) | int(payload[p + 1]) << 8


@functools.lru_cache(maxsize=None)
def shapes():
    """Asserts every content's claim on the oracle's frames; -> {name: [(payload size, stored)] of its blocks}."""
    res = {}
    for group, (_, bs, names) in GROUPS.items():
        for name in names:
            c = content(name)
            f = oracle_frame(name, bs, False, True, True)
            info, blocks = shard.frame_blocks(f)
            assert tuple(st for _, _, st in blocks) == SHAPES[name], (group, name, blocks)
            assert len(blocks) == -(-c.size // bs) and info["block_max"] == bs and info["content_size"] == c.size
            assert not f[4] & 0x20, name
            st, back = O.decompress_frame(f)
            assert st == 0 and np.array_equal(back, c), name
            res[name] = [(n, s) for _, n, s in blocks]
            if len(blocks) > 1:   # a chain: some block after the first begins with a match into the block before
                pays = [f[p:p + n] for p, n, s in blocks]
                reach = [k for k in range(1, len(blocks)) if not blocks[k][2]
                         and first_match(pays[k])[1] > first_match(pays[k])[0]]
                assert reach or name == "r65536x3", name
    bs = 65536
    # text4: shorter than its independent twin, and different beyond FLG / HC
    d, i = oracle_frame("text4", bs, False, True, True), oracle_frame("text4", bs, True, True, True)
    assert d.size < i.size and not np.array_equal(d[15:d.size], i[15:d.size])
    # rep2: block 1 starts with a match from block 0 and is nearly that one match
    f = oracle_frame("rep2", bs, False, True, True)
    _, blocks = shard.frame_blocks(f)
    lit, off = first_match(f[blocks[1][0]:blocks[1][0] + blocks[1][1]])
    assert lit == 0 and off > 0 and off % 251 == 0 and blocks[1][1] < 300 and blocks[2][1:] == (13, True)
    # randtail: block 1's first match lies in the stored block 0's raw bytes, 30000 back
    f = oracle_frame("randtail", bs, False, True, True)
    _, blocks = shard.frame_blocks(f)
    lit, off = first_match(f[blocks[1][0]:blocks[1][0] + blocks[1][1]])
    assert lit < 4 and off == 30000 and blocks[0][2]
    # r65535x3: the largest offset; r65536x3: one past it, nothing matches
    f = oracle_frame("r65535x3", bs, False, True, True)
    _, blocks = shard.frame_blocks(f)
    for k in (1, 2):
        assert first_match(f[blocks[k][0]:blocks[k][0] + blocks[k][1]])[1] == 65535 and blocks[k][1] < 600, k
    assert content("tiles300k").size > 3 * RING_BYTES
    return res


def chain_names(group):
    return [n for n in GROUPS[group][2] if len(SHAPES[n]) > 1]


def need_blocks(group):
    return sum(len(SHAPES[n]) for n in GROUPS[group][2])


@functools.lru_cache(maxsize=None)
def arena(group, fill):
    """-> (arena, offsets, lengths): the group's sources at start residues 0, 1, 7, 15 (mod 16) in turn."""
    names = GROUPS[group][2]
    offs, at = [], 64
    for k, name in enumerate(names):
        at += 5
        at += (RESIDUES[k % 4] - at) % 16
        offs.append(at)
        at += content(name).size
    a = np.full(at + 64, fill, dtype=np.uint8)
    for o, name in zip(offs, names):
        a[o:o + content(name).size] = content(name)
    a.setflags(write=False)
    return a, np.array(offs, dtype=np.uint64), np.array([content(n).size for n in names], dtype=np.uint64)


def slot_bytes(n):
    return (n + n // 255 + 16 + 15) & ~15


def closed_form_plan(lens, offs, bs, combo, cap, chains=True):
    """lz4mi_frames_plan with LZ4MI_FRAMES_DEPENDENT (| LZ4MI_FRAMES_CHAINS) in a few lines: -> (finfo rows, totals,
    blk_in_off, blk_len, blk_frame, blk_work_off)."""
    csum, sized, bsum = combo
    flg = 0x40 | (0x10 if bsum else 0) | (0x08 if sized else 0) | (0x04 if csum else 0)
    bd = {65536: 4, 262144: 5, 1048576: 6, 4194304: 7}[bs] << 4
    rows, lists, first, slot = [], ([], [], [], []), 0, 16
    for f, (n, off) in enumerate(zip(lens, offs)):
        count = -(-n // bs)
        decline = DEPENDENT if count > 1 and (not chains or n >= 0x7FFFFFFF) else HASH_4G if (csum and n >= 2 ** 32) else 0
        rows.append([0, flg | bd << 8, n, 23 + n + 8 * count, first, 0, count, decline])
        if decline:
            continue
        if first + count <= cap:
            at = slot
            for k in range(count):
                ln = min(bs, n - k * bs)
                for lst, v in zip(lists, (off + k * bs, ln, f, at)):
                    lst.append(v)
                at += slot_bytes(ln)
        elif count:
            rows[-1][7] = CAP_BLOCKS
        first += count
        slot += (count - 1) * slot_bytes(bs) + slot_bytes(n - (count - 1) * bs) if count else 0
    totals = [first, len(lists[0]), sum(r[3] for r in rows if not r[7]), slot]
    return (rows, totals) + lists
