"""Shared by tests/test_frames_cpu.py and tests/test_gpu_frames_batch.py: a zoo of frames for the frame batch
(lz4mi_frames_index / lz4mi_frames_decompress / lz4mi_host_frames_index), all built by the CPU oracle with
64 KiB blocks, read-only, their shapes asserted so that a change in the oracle cannot hollow the tests out.

  - contents of 0, 1, 65535, 65536 and 65537 bytes and the five-block content of verify_common.data() (one
    stored block), each as {independent, dependent} x {content size, none} x {content checksum, none}; one
    with block checksums (their words have to be skipped);
  - two hand-assembled frames with a partial block in the middle (with / without a content size), one with a
    DictID field;
  - damaged frames: wrong magic, version bits 0, cut inside the size field, cut inside a payload, block 0
    undecodable, a match of block 0 reaching below the frame's start, a flipped content-checksum byte, a
    stored block declaring more than the content size; two whose content size exceeds what the blocks give;
    a content size of 2^40.
arena(fill): all of them in one array at start residues 0 - 3 (mod 4) in turn, 5 to 8 filler bytes between two.
"""
import functools

import numpy as np

import oracle as O
import footprint_common as FP
import verify_common as V
from lz4mi import frame as F
from lz4mi import shard

BS = 65536
FILLS = (0x00, 0xFF)
SIZES = (0, 1, 65535, 65536, 65537)
# the blocks of each content, as stored flags (asserted in zoo()): one byte cannot be compressed
SHAPES = {0: (), 1: (True,), 65535: (False,), 65536: (False,), 65537: (False, True),
          "five": (False, False, True, False, False)}
# finfo[f][7] (include/lz4mi.h LZ4MI_FRAMES_DECLINE_*)
(CAP_BLOCKS, PAST_END, EMPTY, UNSIZED_EXACT, MEASURE, SIZE_MISMATCH, OUT_CAP, LAYOUT, DEPENDENT, HASH_4G) = range(1, 11)
ERR_OFFSET0, ERR_DICT_OOB, ERR_MAGIC, ERR_VERSION, ERR_CHECKSUM, ERR_RANGE = -3, -4, -5, -6, -7, -8
PARTIAL = (BS, 30000, BS)        # the hand-assembled frames' block contents


@functools.lru_cache(maxsize=None)
def content(key):
    if key == "five":
        return V.data()
    c = O.generate("tiles216", 40 + key % 7, key)
    c.setflags(write=False)
    return c


def _le32(x):
    return np.array([x & 0xFFFFFFFF], dtype="<u4").view(np.uint8)


def _assemble(head, records):
    """header + (size word, payload) records + EndMark."""
    parts = [np.frombuffer(head, dtype=np.uint8)]
    for word, pay in records:
        parts += [_le32(word), np.asarray(pay, dtype=np.uint8)]
    return np.concatenate(parts + [_le32(0)])


@functools.lru_cache(maxsize=None)
def partial_content():
    c = np.concatenate([O.generate("tiles216", 50 + k, n) for k, n in enumerate(PARTIAL)])
    c.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def text_content():
    c = np.concatenate([O.generate("random", 1, 16), O.generate("text", 1, 20000)])
    c.setflags(write=False)
    return c


def _partial(sized):
    c, recs, at = partial_content(), [], 0
    for n in PARTIAL:
        comp = O.compress_block_bytes(c[at:at + n])
        assert 0 < comp.size < n
        recs.append((comp.size, comp))
        at += n
    return _assemble(F.header(BS, True, False, c.size if sized else None), recs)


def _below_start():
    """One block: 4 literals, a match of 4 at offset 8 -- four bytes below the frame's start --, 5 literals."""
    blk = bytes([0x40]) + b"abcd" + bytes([8, 0]) + bytes([0x50]) + b"efghi"
    return _assemble(F.header(BS, True, False, 13), [(len(blk), np.frombuffer(blk, dtype=np.uint8))])


def _stored_past():
    return _assemble(F.header(BS, True, False, 100), [(200 | 0x80000000, O.generate("random", 9, 200))])


@functools.lru_cache(maxsize=None)
def zoo():
    """name -> frame (read-only uint8), in a fixed order."""
    z = {}
    for key in SIZES + ("five",):
        for indep in (True, False):
            for sized in (True, False):
                for csum in (True, False):
                    name = f"c{key}_{'i' if indep else 'd'}{'s' if sized else 'u'}{'c' if csum else 'n'}"
                    f = O.compress_frame(content(key), None, BS, indep, csum, sized)
                    info, blocks = shard.frame_blocks(f)
                    assert tuple(st for _, _, st in blocks) == SHAPES[key], (name, blocks)
                    assert bool(info["flg"] & 0x20) == indep and bool(info["flg"] & 0x04) == csum
                    assert bool(info["flg"] & 0x08) == sized and info["content_size"] == (content(key).size if sized else 0)
                    assert info["end"] + (4 if csum else 0) == f.size
                    z[name] = f
    z["five_bsum"] = V.frame(True, True, True, True).copy()
    z["partial_sized"] = _partial(True)
    z["partial_unsized"] = _partial(False)
    comp = O.compress_block_bytes(content(65536))
    z["dictid"] = _assemble(F.header(BS, True, False, 65536, 0x1234ABCD), [(comp.size, comp)])
    assert shard.frame_blocks(z["dictid"])[0]["flg"] & 0x01 and len(shard.frame_blocks(z["dictid"])[1]) == 1
    for name in ("partial_sized", "partial_unsized"):
        assert len(shard.frame_blocks(z[name])[1]) == 3
    base = z["cfive_isc"]
    blocks = shard.frame_blocks(base)[1]
    g = base.copy()
    g[0] ^= 0x01
    z["bad_magic"] = g
    g = base.copy()
    g[4] &= 0x3F
    z["bad_version"] = g
    z["cut_sizefield"] = base[:10].copy()
    z["cut_payload"] = base[:blocks[3][0] + 100].copy()
    z["decode0"] = V.damaged(base, "decode0")
    z["below_start"] = _below_start()
    g = base.copy()
    g[g.size - 2] ^= 0x40
    z["csum_flip"] = g
    z["stored_past"] = _stored_past()
    # a text block behind 16 random bytes: the reference decoder's bytes differ from the content (its tail rewrite),
    # and no rewrite reads below the block's start
    z["text_isc"] = O.compress_frame(text_content(), None, BS, True, True, True)
    (p0, n0, st0), = shard.frame_blocks(z["text_isc"])[1]
    assert not st0 and not FP.reads_below(z["text_isc"][p0:p0 + n0])
    assert (O.decompress_frame(z["text_isc"], verify_checksum=False, js_compat=True)[1] != text_content()).any()
    # a content size above what the blocks produce: the reference's result keeps its zeros behind them
    z["zero_tail"] = _assemble(F.header(BS, True, False, 70000), [(comp.size, comp)])
    z["zero_tail5"] = _assemble(F.header(BS, True, False, 65541), [(comp.size, comp)])
    # a content size no frame of this length can decode to (above frame.content_size_bound): ERR_RANGE, and nothing
    # may be sized from it
    g = z["cfive_isn"].copy()
    g[6:14] = np.frombuffer((1 << 40).to_bytes(8, "little"), dtype=np.uint8)
    z["huge_size"] = g
    for f in z.values():
        f.setflags(write=False)
    return z


NAMES = tuple(zoo())


def is_dependent_five(name):
    return name.startswith("cfive_d")


# Built on the five-block content with its blocks independent. Its text blocks (3 and 4) begin with a word they
# repeat within a few bytes: a short match whose tail rewrite, in the reference decoder, reads below the block's
# own start (footprint_common.reads_below). A batch of isolated blocks reports that as LZ4MI_ERR_CROSS_BLOCK.
FIVE_INDEPENDENT_SIZED = ("cfive_isc", "cfive_isn", "five_bsum", "decode0", "csum_flip")


@functools.lru_cache(maxsize=None)
def rewrites_below(name):
    f = zoo()[name]
    return any(not st and p + n <= f.size and FP.reads_below(f[p:p + n]) for p, n, st in shard.frame_blocks(f)[1])


# ------------------------------------------------------------------------- expectations, written out by name
def expected_index(name, js_exact=False, measure=False):
    """(finfo[0], finfo[7]) after the index call."""
    if name == "bad_magic":
        return ERR_MAGIC, 0
    if name == "bad_version":
        return ERR_VERSION, 0
    if name in ("cut_sizefield", "cut_payload"):
        return 0, PAST_END
    if name.startswith("c0_"):
        return 0, EMPTY
    unsized = name == "partial_unsized" or (name[0] == "c" and name.split("_")[1][1] == "u")
    if unsized and js_exact:
        return 0, UNSIZED_EXACT
    if name == "decode0" and measure:
        return 0, MEASURE          # block 0's size walk fails (a token 0x00 with offset 0)
    if name == "stored_past" and measure:
        return 0, SIZE_MISMATCH    # 200 stored bytes measured against a content size of 100
    if name == "huge_size" and measure:
        return 0, SIZE_MISMATCH    # 263144 bytes measured against 2^40
    if name.startswith("zero_tail") and measure:
        return 0, SIZE_MISMATCH    # 65536 bytes measured against a larger content size
    return 0, 0


def expected_batch(name, js_exact=False, measure=False, verify=True):
    """(status, decline code) after both calls: what lz4mi_frames_decompress leaves in finfo[0] and finfo[7]."""
    st, dc = expected_index(name, js_exact, measure)
    if st or dc:
        return st, dc
    if name == "huge_size":
        return 0, OUT_CAP          # the caller gives it no room (tests and wrapper alike): 2^40 bytes sized nothing
    if is_dependent_five(name):
        return 0, DEPENDENT        # block 1 (the second tiles216 block) copies from block 0
    if js_exact and name in FIVE_INDEPENDENT_SIZED:
        assert rewrites_below(name)
        return 0, DEPENDENT        # a tail rewrite reads below its block: decoded alone, in order, by the frame call
    assert not (js_exact and rewrites_below(name)), name
    if name == "partial_sized":
        return (0, 0) if measure else (0, LAYOUT)   # block 1 fills 30000 of its 65536-byte slot
    if name == "below_start" and measure and not js_exact:
        return 0, LAYOUT           # a measured frame with a failing block: the single-frame route's host case
    if name == "below_start":
        # spec: the reference's check 4 at the frame's start; a reference mode cannot tell it from a tail
        # rewrite reading below the frame and leaves the frame to the single-frame call
        return (0, DEPENDENT) if js_exact else (ERR_DICT_OOB, 0)
    if name == "decode0":
        return ERR_OFFSET0, 0      # a token 0x00 whose match has offset 0
    if name == "stored_past":
        return ERR_RANGE, 0
    if name == "csum_flip":
        return (ERR_CHECKSUM if verify else 0), 0
    if js_exact and verify and name == "text_isc":
        return ERR_CHECKSUM, 0     # the reference decoder's bytes of the text blocks differ
    return 0, 0


@functools.lru_cache(maxsize=None)
def arena(fill):
    """-> (arena, offsets, lengths): the zoo packed at start residues 0, 1, 2, 3 (mod 4) in turn."""
    z = zoo()
    offs, at = [], 64
    for k, name in enumerate(NAMES):
        at += 5
        at += (k % 4 - at) % 4
        offs.append(at)
        at += z[name].size
    a = np.full(at + 64, fill, dtype=np.uint8)
    for o, name in zip(offs, NAMES):
        a[o:o + z[name].size] = z[name]
    a.setflags(write=False)
    return a, np.array(offs, dtype=np.uint64), np.array([z[n].size for n in NAMES], dtype=np.uint64)


def need_blocks():
    return sum(len(shard.frame_blocks(zoo()[n])[1]) for n in NAMES
               if expected_index(n)[0] == 0 and expected_index(n)[1] not in (PAST_END, EMPTY))


def tiny_frames(n):
    """n frames of one byte of content each (one stored block), alternately with and without a content size."""
    fs = [O.compress_frame(np.array([k & 255], dtype=np.uint8), None, BS, True, bool(k & 2), bool(k & 1)) for k in range(4)]
    return [fs[k % 4] for k in range(n)]


def pack(frames):
    lens = np.array([f.size for f in frames], dtype=np.uint64)
    offs = np.zeros(len(frames), dtype=np.uint64)
    offs[1:] = np.cumsum(lens[:-1])
    return np.concatenate(frames), offs, lens
