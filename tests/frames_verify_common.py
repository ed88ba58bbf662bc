"""Shared by tests/test_frames_verify_cpu.py and tests/test_gpu_frames_verify.py: a zoo of frames for
lz4mi_frames_verify_blocks / lz4mi_host_frames_verify_blocks (block checksums, FLG 0x10, of a frame batch), built on
the CPU by lz4mi.host_frames_plan / host_frames_compress with 64 KiB blocks, read-only, its shapes asserted.

  - random contents at the edges of the hashing code (one stored block each, payload = content): the tail loops,
    the 8-stripe loop, the entry of the 128-stripe pipeline and its first full iteration, a whole block; each with
    and without a content size;
  - compressible contents of one, two and five blocks (tiles216) and verify_common.data() with its stored block;
  - every content again without FLG 0x10, the empty frame with it, one hand-assembled frame without a content size;
  - damaged copies: a flipped bit in the first, a middle and the last payload byte of the first, a middle and the
    last block, inside the last 15 payload bytes, in each of the four checksum bytes; a bad magic; and the three
    frames whose own error has to give way to the block checksum (an undecodable block 0, a flipped content
    checksum, a stored block past the content size).
arena(fill): all of them at start residues 0 - 3 (mod 4) in turn, 5 to 8 filler bytes between two, and nothing
behind the last frame: the arena ends where it ends.
"""
import functools

import numpy as np

import lz4mi
import oracle as O
import verify_common as V
from lz4mi import frame as F
from lz4mi import shard

BS = 65536
FILLS = (0x00, 0xFF)
ERR_BLOCK_CHECKSUM, ERR_MAGIC = -10, -5
CAP_BLOCKS, PAST_END, EMPTY = 1, 2, 3          # the declines that leave a frame's blocks out of the lists
EDGE_LENS = (1, 3, 4, 15, 16, 17, 31, 32, 127, 128, 129, 4095, 4096, 4097, 6143, 6144, 6145, 65536)
TILES = {"tiles1": BS, "tiles2": 2 * BS, "tiles5": 5 * BS}


def _le32(x):
    return np.array([x & 0xFFFFFFFF], dtype="<u4").view(np.uint8)


@functools.lru_cache(maxsize=None)
def content(name):
    if name == "five":
        return V.data()
    if name == "empty":
        return np.zeros(0, dtype=np.uint8)
    if name in TILES:
        c = O.generate("tiles216", 60 + TILES[name] // BS, TILES[name])
    else:
        c = O.generate("random", 100 + int(name[1:]) % 89, int(name[1:]))
    c.setflags(write=False)
    return c


CONTENTS = tuple(f"r{n}" for n in EDGE_LENS) + tuple(TILES) + ("five",)


def _built(names, **kw):
    """One host plan and one packed host compress of the named contents -> the frames, in order."""
    lens = np.array([content(n).size for n in names], dtype=np.uint64)
    offs = (np.cumsum(lens) - lens).astype(np.uint64)
    src = np.concatenate([content(n) for n in names] + [np.zeros(1, dtype=np.uint8)])
    flags = lz4mi.frames_enc_flags(packed=True, **kw)
    need = int(sum(-(-int(n) // BS) for n in lens))
    plan = lz4mi.host_frames_plan(offs, lens, BS, need, flags)
    assert int(plan["totals"][1]) == need and not plan["finfo"][:, 7].any()
    out = np.zeros(int(plan["totals"][2]), dtype=np.uint8)
    fi = lz4mi.host_frames_compress(src, plan, out, flags)
    assert not fi[:, 0].any() and not fi[:, 7].any()
    return [out[int(fi[k, 5]):int(fi[k, 5]) + int(fi[k, 3])].copy() for k in range(len(names))]


def flip(f, pos, bit=0x01):
    g = f.copy()
    g[pos] ^= bit
    return g


def _unsized():
    """Hand-assembled: two compressed blocks with their checksums behind a header with FLG 0x10 and no content size."""
    c = O.generate("tiles216", 77, BS + 30000)
    parts = [np.frombuffer(F.header(BS, True, False, None, None, True), dtype=np.uint8)]
    for p in (0, BS):
        comp = O.compress_block_bytes(c[p:p + BS])
        assert 0 < comp.size < c[p:p + BS].size
        parts += [_le32(comp.size), comp, _le32(O.xxh32_std(comp))]
    return np.concatenate(parts + [_le32(0)])


def _stored_past():
    """A stored block of 200 bytes in a frame of content size 100 (the decoder's LZ4MI_ERR_RANGE), its checksum
    one bit off."""
    pay = O.generate("random", 9, 200)
    head = np.frombuffer(F.header(BS, True, False, 100, None, True), dtype=np.uint8)
    return np.concatenate([head, _le32(200 | 0x80000000), pay, _le32(O.xxh32_std(pay) ^ 0x100), _le32(0)])


@functools.lru_cache(maxsize=None)
def zoo():
    """name -> (frame, damaged: {block index} whose record must fail, or None for a frame that is not checked)."""
    z = {}
    sized = _built(CONTENTS + ("empty",), block_checksum=True, content_checksum=True)
    unsized = _built(CONTENTS[:len(EDGE_LENS)], block_checksum=True, add_content_size=False)
    plain = _built(CONTENTS, content_checksum=True)
    for name, f in zip(CONTENTS + ("empty",), sized):
        info, blocks = shard.frame_blocks(f)
        assert info["flg"] & 0x10 and info["flg"] & 0x08 and info["flg"] & 0x04, name
        if name[0] == "r":     # random content: one stored block whose payload is the content
            (p, n, st), = blocks
            assert st and n == content(name).size and np.array_equal(f[p:p + n], content(name)), name
        z[name] = (f, None if name == "empty" else set())
    assert [st for _, _, st in shard.frame_blocks(z["five"][0])[1]] == [False, False, True, False, False]
    for key, count in (("tiles1", 1), ("tiles2", 2), ("tiles5", 5)):
        assert [st for _, _, st in shard.frame_blocks(z[key][0])[1]] == [False] * count, key
    for name, f in zip(CONTENTS, unsized):
        info, blocks = shard.frame_blocks(f)
        assert info["flg"] & 0x10 and not info["flg"] & 0x08 and len(blocks) == 1 and blocks[0][1] == content(name).size
        z[name + "_u"] = (f, set())
    for name, f in zip(CONTENTS, plain):
        assert not shard.frame_blocks(f)[0]["flg"] & 0x10
        z[name + "_plain"] = (f, None)
    z["unsized2"] = (_unsized(), set())
    assert len(shard.frame_blocks(z["unsized2"][0])[1]) == 2
    # a flipped bit at the first, a middle and the last payload byte of the first, a middle and the last block
    for base in ("five", "tiles5"):
        f = z[base][0]
        blocks = shard.frame_blocks(f)[1]
        for b in (0, 2, 4):
            p, n, _ = blocks[b]
            for where, pos in (("first", p), ("mid", p + n // 2), ("last", p + n - 1)):
                z[f"{base}_b{b}_{where}"] = (flip(f, pos, 0x01 << (b + pos) % 8), {b})
    # inside the last 15 payload bytes (the bytes behind the last stripe), at every distance from the end
    for base, d in (("r31", 15), ("r4095", 2), ("r4095", 9), ("r6143", 4), ("r6143", 15)):
        f = z[base][0]
        (p, n, _), = shard.frame_blocks(f)[1]
        assert n % 16 == 15
        z[f"{base}_tail{d}"] = (flip(f, p + n - d, 0x10), {0})
    # (without a content size: declined as UNSIZED_EXACT by an index call with LZ4MI_JS_EXACT, and still checked)
    f = z["r129_u"][0]
    (p, n, _), = shard.frame_blocks(f)[1]
    z["r129_u_mid"] = (flip(f, p + 64, 0x02), {0})
    # each of the four checksum bytes of the second block of two
    f = z["tiles2"][0]
    p, n, _ = shard.frame_blocks(f)[1][1]
    for k in range(4):
        z[f"tiles2_sum{k}"] = (flip(f, p + n + k, 0x04 << k), {1})
    # header errors come first: not checked
    z["bad_magic"] = (flip(z["five"][0], 0), None)
    # the three frames whose own error gives way
    five = V.frame(True, True, True, True)
    assert np.array_equal(five, z["five"][0]), "the host encoder's frame is the oracle's"
    z["pre_decode0"] = (V.damaged(five, "decode0"), {0})
    p, n, _ = V.blocks_of(five)[4]
    z["pre_content"] = (flip(flip(five, five.size - 2, 0x40), p + n + 1, 0x08), {4})
    z["pre_stored_past"] = (_stored_past(), {0})
    for f, _ in z.values():
        f.setflags(write=False)
    return z


NAMES = tuple(zoo())
PRECEDENCE = ("pre_decode0", "pre_content", "pre_stored_past")


def records():
    """The number of records the call has to hash."""
    return sum(len(shard.frame_blocks(f)[1]) for f, dmg in zoo().values() if dmg is not None)


def need_blocks():
    return sum(len(shard.frame_blocks(f)[1]) for n, (f, _) in zoo().items() if n not in ("bad_magic", "empty"))


@functools.lru_cache(maxsize=None)
def arena(fill):
    """-> (arena, offsets, lengths): the zoo at start residues 0, 1, 2, 3 (mod 4) in turn; the arena ends with
    the last frame."""
    z = zoo()
    offs, at = [], 64
    for k, name in enumerate(NAMES):
        at += 5
        at += (k % 4 - at) % 4
        offs.append(at)
        at += z[name][0].size
    a = np.full(at, fill, dtype=np.uint8)
    for o, name in zip(offs, NAMES):
        a[o:o + z[name][0].size] = z[name][0]
    a.setflags(write=False)
    return a, np.array(offs, dtype=np.uint64), np.array([z[n][0].size for n in NAMES], dtype=np.uint64)


def checked(fi, nblocks):
    """The rule of include/lz4mi.h, written out: is the frame with this finfo row checked?"""
    return bool(fi[0] == 0 and fi[1] & 0x10 and fi[7] not in (CAP_BLOCKS, PAST_END, EMPTY) and fi[6] > 0 and
                fi[4] + fi[6] <= nblocks)


def yardstick(a, off, ln, index, nblocks):
    """blk_status from what exists without the call: lz4mi.host_verify_blocks(frame_words=True) over each checked
    frame alone (its in_total is the frame's length), 0 everywhere else."""
    want = np.zeros(nblocks, dtype=np.int32)
    for f in range(off.size):
        fi = index["finfo"][f]
        if not checked(fi, nblocks):
            continue
        lo, n = int(fi[4]), int(fi[6])
        frame = a[int(off[f]):int(off[f]) + int(ln[f])]
        rel = index["blk_in_off"][lo:lo + n] - off[f]
        want[lo:lo + n] = lz4mi.host_verify_blocks(frame, rel, index["blk_word"][lo:lo + n], frame_words=True)
    return want


def expected_failing():
    """By name, from the damage that was done."""
    return {n for n, (_, dmg) in zoo().items() if dmg}


# ------------------------------------------------------------------------------------ the hand-made lists
@functools.lru_cache(maxsize=None)
def handmade(fill):
    """Three intact frames with block checksums (r32, tiles2, r17: four records) in an arena of their own, indexed
    by the host, and then bent -- every position stays inside the arena:
      - frame 0's length ends just in front of its record's four checksum bytes, which still lie behind it in the
        arena and ARE the right digest: the record is cut and must fail;
      - frame 1's block 1 points at frame 0's record, below frame 1's start: a whole, correct record of another
        frame must fail;
      - frame 2's only entry names frame 3 (>= nframes) and its checksum is damaged: not checked, status 0.
    -> (arena, off, len, index dict, expected blk_status, expected finfo[:, 0])."""
    z = zoo()
    (p17, n17, _), = shard.frame_blocks(z["r17"][0])[1]
    frames = [z["r32"][0], z["tiles2"][0], flip(z["r17"][0], p17 + n17 + 1)]
    offs, at = [], 16
    for k, f in enumerate(frames):
        at += 5
        at += ((k + 1) % 4 - at) % 4
        offs.append(at)
        at += f.size
    a = np.full(at + 16, fill, dtype=np.uint8)
    for o, f in zip(offs, frames):
        a[o:o + f.size] = f
    off = np.array(offs, dtype=np.uint64)
    ln = np.array([f.size for f in frames], dtype=np.uint64)
    index = lz4mi.host_frames_index(a, off, ln, 4)
    assert index["totals"].tolist()[:2] == [4, 4] and not index["finfo"][:, 0].any() and not index["finfo"][:, 7].any()
    assert index["blk_frame"].tolist() == [0, 1, 1, 2]
    ln[0] = int(index["blk_in_off"][0]) + 32 - offs[0]        # ends in front of the checksum
    assert O.xxh32_std(a[int(index["blk_in_off"][0]):][:32]) == int(a[offs[0] + int(ln[0]):][:4].view("<u4")[0])
    index["blk_in_off"][2] = index["blk_in_off"][0]
    index["blk_word"][2] = index["blk_word"][0]
    index["blk_frame"][3] = 3
    a.setflags(write=False)
    return a, off, ln, index, np.array([ERR_BLOCK_CHECKSUM, 0, ERR_BLOCK_CHECKSUM, 0], dtype=np.int32), \
        [ERR_BLOCK_CHECKSUM, ERR_BLOCK_CHECKSUM, 0]
