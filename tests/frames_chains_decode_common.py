"""Shared by tests/test_frames_chains_decode_cpu.py and tests/test_gpu_frames_chains_decode.py: the inputs of the
decode side of LZ4MI_FRAMES_CHAINS (lz4mi_frames_decompress: frames with dependent blocks decoded in the batch, one
wave per frame in block order). Everything is built on the CPU from the oracle, read-only, and every input's claim
is asserted by claims() so that a change in the oracle cannot hollow the tests out.

  chain zoo   the dependent oracle frames (content checksum, content size) of frames_chain_common's group c64k in
              its arena order -- text4, rep2 (stored last block), randtail (a match into the stored block 0),
              r65535x3 (offset 65535), r65536x3 (all stored), tiles300k -- with the group's one-block frames between
              them, in one arena at start residues 0, 1, 7, 15 (mod 16);
  c4m         the pair of group c4m: text300 and tiles4m70k (one 4 MiB block and 70000 bytes);
  frame zoo   frames_common's zoo and arena as they are;
  damaged     frames_common's sized dependent five-block frame with block 3's payload starting 00 00 00: a token
              0x00 whose match has offset 0;
  neighbours  a decoded frame, frames_common's below_start, a decoded frame;
  many        65 two-block dependent frames of 65536 + 100 bytes of text.
want(frame, exact, verify): the oracle's (status, bytes) for a frame.
"""
import functools

import numpy as np

import oracle as O
import footprint_common as FP
import frames_chain_common as CC
import frames_common as C
from lz4mi import shard

BS = 65536
FILLS = (0x00, 0xFF)
RESIDUES = (0, 1, 7, 15)
ERR_OFFSET0, ERR_DICT_OOB, ERR_CHECKSUM = -3, -4, -7
CHAINS64 = ("text4", "rep2", "randtail", "r65535x3", "r65536x3", "tiles300k")
NAMES64 = CC.GROUPS["c64k"][2]
NAMES4M = CC.GROUPS["c4m"][2]
MANY = 65


def blocks_of(f):
    return shard.frame_blocks(f)[1]


def frozen(f):
    f = np.ascontiguousarray(f, dtype=np.uint8)
    f.setflags(write=False)
    return f


def chain_frame(name, group="c64k"):
    return CC.oracle_frame(name, CC.GROUPS[group][1], False, True, True)


def want(frame, exact, verify, cap=None):
    """The oracle's (status, bytes): the status with or without the content checksum, the bytes without it."""
    if cap is None:
        size = int.from_bytes(frame[6:14].tobytes(), "little") if frame.size >= 14 and frame[4] & 0x08 else 0
        cap = max(6 * BS, size + 64 if size < (1 << 32) else 0)
    st, _ = O.decompress_frame(frame, verify_checksum=verify, js_compat=exact, out_cap=cap)
    bst, out = O.decompress_frame(frame, verify_checksum=False, js_compat=exact, out_cap=cap)
    assert st == bst or (st == ERR_CHECKSUM and bst == 0)
    return st, out


def pack16(frames, fill):
    """-> (arena, offsets, lengths): the frames at start residues 0, 1, 7, 15 (mod 16) in turn."""
    offs, at = [], 64
    for k, f in enumerate(frames):
        at += 5
        at += (RESIDUES[k % 4] - at) % 16
        offs.append(at)
        at += f.size
    a = np.full(at + 64, fill, dtype=np.uint8)
    for o, f in zip(offs, frames):
        a[o:o + f.size] = f
    a.setflags(write=False)
    return a, np.array(offs, dtype=np.uint64), np.array([f.size for f in frames], dtype=np.uint64)


@functools.lru_cache(maxsize=None)
def chain_arena(fill, group="c64k"):
    return pack16([chain_frame(n, group) for n in CC.GROUPS[group][2]], fill)


def reaching_blocks(f):
    """The compressed blocks behind the first whose first sequence is a match into the block before."""
    res = []
    for k, (p, n, st) in enumerate(blocks_of(f)):
        if k and not st:
            lit, off = CC.first_match(f[p:p + n])
            if off > lit:
                res.append(k)
    return res


@functools.lru_cache(maxsize=None)
def damaged_five():
    """-> (frame, the undamaged frame, end of block 2): block 3 starts with a token 0x00 and offset 0."""
    base = C.zoo()["cfive_dsn"]
    b = blocks_of(base)
    g = base.copy()
    g[b[3][0]:b[3][0] + 3] = 0
    return frozen(g), base, 3 * BS


def partial_five(exact):
    """The oracle's result of the damaged frame up to its failing block: blocks 0 and 1 decoded in order on one
    array, block 2 copied."""
    g, _, end = damaged_five()
    out = np.zeros(C.content("five").size, dtype=np.uint8)
    pos = 0
    for p, n, stored in blocks_of(g)[:3]:
        if stored:
            out[pos:pos + n] = g[p:p + n]
            pos += n
        else:
            st, w, _ = O.decompress_block(g[p:p + n], BS, out=out, out_off=pos, js_compat=exact)
            assert st == 0 and w == BS
            pos += w
    assert pos == end
    return out[:end]


@functools.lru_cache(maxsize=None)
def many_frames():
    fs = [frozen(O.compress_frame(O.generate("text", 100 + k, BS + 100), None, BS, False, bool(k & 1), True))
          for k in range(MANY)]
    return tuple(fs)


@functools.lru_cache(maxsize=None)
def neighbours():
    z = C.zoo()
    return (z["c65537_isn"], z["below_start"], z["c65535_isn"])


@functools.lru_cache(maxsize=None)
def claims():
    """Every input's claim, on the oracle."""
    CC.shapes()
    for group, chains in (("c64k", CHAINS64), ("c4m", ("tiles4m70k",))):
        assert tuple(CC.chain_names(group)) == chains
        for name in chains:
            f = chain_frame(name, group)
            info, blocks = shard.frame_blocks(f)
            assert not info["flg"] & 0x20 and info["flg"] & 0x0C == 0x0C and len(blocks) > 1, name
            assert reaching_blocks(f) or name == "r65536x3", name
    assert blocks_of(chain_frame("rep2"))[-1][2] and blocks_of(chain_frame("randtail"))[0][2]
    assert all(st for _, _, st in blocks_of(chain_frame("r65536x3")))
    a, off, ln = chain_arena(0)
    assert [int(o) % 16 for o in off] == [RESIDUES[k % 4] for k in range(off.size)]
    # the frame zoo: the dependent five-block frames, and the independent ones whose text blocks rewrite below
    for name in C.NAMES:
        if C.is_dependent_five(name):
            f = C.zoo()[name]
            assert not f[4] & 0x20 and 1 in reaching_blocks(f), name
    for name in C.FIVE_INDEPENDENT_SIZED:
        f = C.zoo()[name]
        assert f[4] & 0x20 and C.rewrites_below(name), name
        below = [k for k, (p, n, st) in enumerate(blocks_of(f)) if not st and FP.reads_below(f[p:p + n])]
        assert below == [3, 4], (name, below)
    # the damaged frame: dependent, sized; block 3 fails with offset 0 alone and in the frame, blocks 0 - 2 are the
    # undamaged frame's
    g, base, end = damaged_five()
    b = blocks_of(g)
    assert not g[4] & 0x20 and g[4] & 0x08 and len(b) == 5 and b == blocks_of(base)
    assert O.decompress_block(g[b[3][0]:b[3][0] + b[3][1]], BS)[0] == ERR_OFFSET0
    assert (g[:b[3][0]] == base[:b[3][0]]).all()
    for exact in (False, True):
        assert O.decompress_frame(g, verify_checksum=False, js_compat=exact)[0] == ERR_OFFSET0
        st, whole = O.decompress_frame(base, verify_checksum=False, js_compat=exact)
        assert st == 0 and (whole[:end] == partial_five(exact)).all()
    # below_start: the reference's check 4 in both modes
    for exact in (False, True):
        assert O.decompress_frame(C.zoo()["below_start"], verify_checksum=False, js_compat=exact)[0] == ERR_DICT_OOB
    for f in many_frames():
        info, blocks = shard.frame_blocks(f)
        assert not info["flg"] & 0x20 and [st for _, _, st in blocks] == [False, False] and reaching_blocks(f) == [1]
        assert info["content_size"] == BS + 100
    return True


def expected_zoo(name, exact, verify):
    """(finfo[0], finfo[7]) of a frame of frames_common's zoo after index and decode with LZ4MI_FRAMES_CHAINS: the
    index's outcome, the two declines that stay, else the oracle's status for the frame."""
    st, dc = C.expected_index(name, exact)
    if st or dc:
        return st, dc
    if name == "huge_size":
        return 0, C.OUT_CAP
    if name == "partial_sized":
        return 0, C.LAYOUT
    return want(C.zoo()[name], exact, verify)[0], 0
