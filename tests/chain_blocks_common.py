"""Shared by tests/test_chain_blocks_cpu.py and tests/test_gpu_chain_blocks.py: hand-assembled frames whose
blocks read the blocks before them, for the chain kernel of LZ4MI_FRAMES_CHAINS (lz4mi_frames_decompress: the
one-wave decoder, block after block of a frame, each block's sources in the bytes the last one wrote). The blocks
are assembled with test_gpu_seqtable's encode / Maker and literal_pieces_common's builders at a position `base`
of the frame, so that drawn offsets range over the frame's history; the frames with frames_common._assemble and
lz4mi.frame.header. Everything is built on the CPU, read-only; claims() proves every input on the oracle alone.

Two kinds of frame, both with a content size:
  layout     every block but the last decodes to exactly 64 KiB (the reference encoder's layout): indexed without
             LZ4MI_FRAMES_MEASURE;
  measured   blocks of any size: indexed with LZ4MI_FRAMES_MEASURE.
Families (Frame.family), see each builder:
  boundary, history_fill, pieces_after_history, tiny, flagged_independent, rewrite, errors.
"""
import functools

import numpy as np

import oracle as O
import footprint_common as FP
import frames_common as C
import literal_pieces_common as LP
import test_gpu_seqtable as S
from linked_exact_common import parse
from lz4mi import frame as F
from lz4mi import shard
import lz4mi

BS = 65536
OK, TOO_SMALL, MALFORMED, OFFSET0, DICT_OOB = 0, -1, -2, -3, -4
MODES = (False, True)                 # js_compat of the oracle: spec, the reference decoder's bytes
PERIODS = (1, 2, 3, 4, 7, 8, 15, 16, 17, 63, 64)


def frozen(a):
    a = np.ascontiguousarray(a, dtype=np.uint8)
    a.setflags(write=False)
    return a


class Frame:
    """name, family, kind ('layout' | 'measured'), the frame's bytes, its blocks [(payload, stored)], the decoded
    size of each block (what the index lists as blk_size), the content size, and what the family says of it."""

    def __init__(self, name, family, kind, blocks, sizes, independent=False, csum=False, bsum=False, total=None,
                 **says):
        self.name, self.family, self.kind, self.says = name, family, kind, says
        self.blocks = [(frozen(p), bool(st)) for p, st in blocks]
        self.sizes = [int(n) for n in sizes]
        self.total = int(sum(sizes) if total is None else total)
        self.independent, self.csum = independent, csum
        recs = []
        for p, st in self.blocks:
            pay = np.concatenate([p, C._le32(O.xxh32_std(p))]) if bsum else p
            recs.append((p.size | (0x80000000 if st else 0), pay))
        f = C._assemble(F.header(BS, independent, csum, self.total, block_checksum=bsum), recs)
        if csum:             # of the content the sequences spell (spec); the reference's own bytes may differ
            st, _, out, _ = decode_blocks(self.blocks, self.total, False)
            assert st == 0, name
            f = np.concatenate([f, C._le32(O.xxh32(out))])
        self.data = frozen(f)

    def starts(self):
        """Where each block begins in the decoded frame."""
        at, res = 0, []
        for n in self.sizes:
            res.append(at)
            at += n
        return res


def decode_blocks(blocks, total, exact, zero_before=None, data=None):
    """The blocks decoded in order on one zeroed array of `total` bytes, as the reference's frame decoder does with
    a content size (each block sees the whole result as its capacity). zero_before=k: the bytes below block k are
    zeroed before it is decoded. data: the assembled frame -- the blocks are then read in place, where a cut block's
    last fields take the bytes that follow it in the frame, as in the reference. -> (status of the first failing
    block or 0, its index or None, the array, the end of each block that decoded)."""
    out = np.zeros(total, dtype=np.uint8)
    pos, ends = 0, []
    where = [q for q, _, _ in shard.frame_blocks(data)[1]] if data is not None else None
    for k, (p, stored) in enumerate(blocks):
        if zero_before == k:
            out[:pos] = 0
        if stored:
            if pos + p.size > total:
                return C.ERR_RANGE, k, out, ends
            out[pos:pos + p.size] = p
            pos += p.size
        else:
            if where is None:
                st, w, _ = O.decompress_block(p, 0, out=out, out_off=pos, js_compat=exact)
            else:
                st, w, _ = O.decompress_block(data, 0, in_off=where[k], in_size=p.size, out=out, out_off=pos,
                                              js_compat=exact)
            if st:
                return st, k, out, ends
            pos += w
        ends.append(pos)
    return 0, None, out, ends


def sequences(comp):
    """linked_exact_common.parse for a block that may be cut: the sequences that are whole."""
    for n in range(len(comp), max(len(comp) - 4, 0), -1):
        try:
            return parse(comp[:n])
        except IndexError:
            pass
    return parse(comp[:max(len(comp) - 4, 0)])


# ------------------------------------------------------------------------------------------------ block builders
def lit_block(data):
    """A compressed block of literals only."""
    return S.encode([], bytes(data))


def fill_to(m, seqs, target, tail=60):
    """Random sequences (0..40 literals, a match of 4..60 bytes, offsets over the whole history) behind `seqs`
    until the block is `tail`..`tail`+100 bytes short of `target`, then the final literals: a block of exactly
    `target` bytes."""
    seqs = list(seqs)
    while m.pos < target - tail - 100:
        seqs.append(m.seq(int(m.rng.integers(0, 41)) if seqs or m.base else int(m.rng.integers(1, 41)),
                          int(m.rng.integers(4, 61))))
    assert tail <= target - m.pos
    return S.encode(seqs, m.lits(target - m.pos))


@functools.lru_cache(maxsize=None)
def fill_block(k, size=BS, seed=0):
    """Block k (at position 64 KiB k) of a frame of random sequences: any frame with that much history takes it."""
    return frozen(fill_to(S.Maker(9000 + 16 * seed + k, k * BS), [], size))


@functools.lru_cache(maxsize=None)
def compact_history(size=BS):
    """`size` bytes that compress to a few KiB and repeat nowhere regularly: 3000 random literals, then matches of
    40..300 bytes at random offsets, 0..6 literals between them."""
    m = S.Maker(9100 + size % 97)
    seqs = [m.seq(3000, 50)]
    while m.pos < size - 400:
        seqs.append(m.seq(int(m.rng.integers(0, 7)), int(m.rng.integers(40, 301))))
    return frozen(S.encode(seqs, m.lits(size - m.pos)))


def opening(m, ll, off, ml):
    """The block's first sequence: ll literals and a match of ml bytes at an offset counted from the match."""
    assert m.pos == 0
    return [m.seq(ll, ml, off=off)]


# ------------------------------------------------------------------------------------------------------ boundary
def boundary_variants():
    """(name, literals -> (offset, match length)) of a block's first match at position `ll` of the block.
      ends_at    the source ends exactly at the block's start;
      across     it starts below the block and ends inside it, offset > match length (needs >= 2 literals);
      period_P   offset P < match length: the period copy starts below the block and runs across its start;
      oldest     offset 65535, the oldest byte a match can reach -- with a match of 5 bytes, whose rewrite in the
                 reference decoder then reads below the frame's start from block 1;
      oldest_ll  offset 65536 - literals."""
    v = [("ends_at_4", lambda ll: (ll + 4, 4)), ("ends_at_20", lambda ll: (ll + 20, 20)),
         ("across", lambda ll: (20 + 1, 20) if ll >= 2 else None),
         ("oldest", lambda ll: (65535, 5)), ("oldest_long", lambda ll: (65535, 300)),
         ("oldest_ll", lambda ll: (65536 - ll, 9) if ll else None)]
    for p in PERIODS:
        v.append((f"period_{p}", lambda ll, p=p: (p, p + 70) if p > ll else None))
    return v


@functools.lru_cache(maxsize=None)
def boundary_frames():
    """Layout frames of 3 blocks: block 1 opens with the variant behind 0 literals (where it needs some, behind 2),
    block 2 with the same behind 1..3. boundary_byte0 is measured: block 0 has 40000 bytes, and blocks 1 and 2
    open with a match at the frame's byte 0, which no block behind 64 KiB can reach."""
    out = []
    for i, (name, fn) in enumerate(boundary_variants()):
        lls = (0 if fn(0) else 2, [ll for ll in (1 + i % 3, 3, 2, 1, 0) if fn(ll)][0])
        blocks, sizes = [(fill_block(0), False)], [BS]
        for k, ll in ((1, lls[0]), (2, lls[1])):
            off, ml = fn(ll)
            m = S.Maker(9200 + 8 * i + k, k * BS)
            size = BS if k == 1 else 700 + 13 * i
            blocks.append((fill_to(m, opening(m, ll, off, ml), size), False))
            sizes.append(size)
        out.append(Frame(f"boundary_{name}", "boundary", "layout", blocks, sizes, opens=lls))
    blocks, sizes = [(fill_block(0, 40000), False)], [40000]
    for k, ll in ((1, 0), (2, 3)):
        m = S.Maker(9390 + k, sum(sizes))
        blocks.append((fill_to(m, opening(m, ll, sum(sizes) + ll, 12), 900 + k), False))
        sizes.append(900 + k)
    out.append(Frame("boundary_byte0", "boundary", "measured", blocks, sizes, opens=(0, 3)))
    return tuple(out)


# -------------------------------------------------------------------------------------------------- history_fill
@functools.lru_cache(maxsize=None)
def history_fill_frames():
    out = []
    for n, csum in ((3, False), (5, True)):
        blocks = [(fill_block(k), False) for k in range(n - 1)] + [(fill_block(n - 1, 30000 + n), False)]
        out.append(Frame(f"fill_{n}", "history_fill", "layout", blocks, [BS] * (n - 1) + [30000 + n], csum=csum))
    stored = frozen(np.random.default_rng(9300).integers(0, 256, BS, dtype=np.uint8))
    blocks = [(fill_block(0), False), (stored, True), (fill_block(2), False), (fill_block(3, 5000), False)]
    out.append(Frame("fill_stored1", "history_fill", "layout", blocks, [BS, BS, BS, 5000]))
    blocks = [(fill_block(k, seed=1), False) for k in range(2)] + [(fill_block(2, 777, seed=1), False)]
    out.append(Frame("fill_bsum", "history_fill", "layout", blocks, [BS, BS, 777], bsum=True, csum=True))
    return tuple(out)


# ----------------------------------------------------------------------------------------- pieces_after_history
@functools.lru_cache(maxsize=None)
def rebuilt_cases():
    """name -> (block at base 0, block rebuilt at base 64 KiB, decoded size, options): every case of
    literal_pieces_common ('lp_' + name) and of test_gpu_seqtable ('st_' + name) that the oracle decodes with
    status 0 in both modes at base 0 (a dictionary case with its dictionary; rebuilt, the history takes its
    place)."""
    res = {}
    lp0, lp1 = LP.all_cases(), LP.raw_cases(BS)
    for name, (comp, cap, opts, ref) in lp0.items():
        if ref[False][0] == 0 and ref[True][0] == 0:
            seqs, fin, _, o = lp1[name]
            res["lp_" + name] = (comp, frozen(S.encode(seqs, fin, o.get("truncate"))), ref[False][1], opts)
    st0 = S.all_cases()
    st1 = S.build_cases(BS)
    for i, c in enumerate(S.fuzz_blocks(BS)):
        st1[f"fuzz{i}"] = c
    for name, (comp, cap, d, ref) in st0.items():
        if ref[False][0] == 0 and ref[True][0] == 0:
            res["st_" + name] = (comp, frozen(st1[name][0]), ref[False][1], {})
    return res


@functools.lru_cache(maxsize=None)
def pieces_frames(kind):
    """layout: 64 KiB of history in one block, then the case as the last block. measured: the history in two
    blocks (65499 + 37 bytes), the case, then a short block whose first match reads the case's last 5 bytes."""
    out = []
    for name, (_, comp, cap, opts) in rebuilt_cases().items():
        if kind == "layout":
            out.append(Frame(f"{name}_layout", "pieces_after_history", kind, [(compact_history(), False), (comp, False)],
                             [BS, cap], case=name))
        else:
            m = S.Maker(9400, BS + cap)
            tail = S.encode([m.seq(1, 9, off=6)] + m.short(3), m.lits(5))
            blocks = [(compact_history(BS - 37), False), (lit_block(m.lits(37)), False), (comp, False), (tail, False)]
            out.append(Frame(f"{name}_measured", "pieces_after_history", kind, blocks, [BS - 37, 37, cap, m.pos + 5],
                             case=name))
    return tuple(out)


# ---------------------------------------------------------------------------------------------------------- tiny
def tiny_blocks(m, n):
    """n blocks of `m`'s frame: 1..3 literals and one match of 4..7 bytes with an offset >= 8 wherever the history
    has 8 bytes (else inside what there is), no final literals. Block 0 of a frame is 3 literals."""
    blocks, sizes = [], []
    for k in range(n):
        if m.base == 0:
            seqs, size = None, 3
            comp = lit_block(m.lits(3))
        else:
            ll, ml = int(m.rng.integers(1, 4)), int(m.rng.integers(4, 8))
            at = m.base + ll
            off = int(m.rng.integers(8, min(at, 65535) + 1)) if at >= 8 else int(m.rng.integers(1, at + 1))
            comp, size = S.encode([(m.lits(ll), off, ml)], None), ll + ml
        blocks.append((comp, False))
        sizes.append(size)
        m.base += size
    return blocks, sizes


@functools.lru_cache(maxsize=None)
def tiny_frames():
    """The finish pass and the chain kernel's scan go over a frame's blocks in rounds of 64: frames of 81, 65 and
    129 blocks."""
    out = []
    for n in (81, 65, 129):
        blocks, sizes = tiny_blocks(S.Maker(9500 + n), n)
        out.append(Frame(f"tiny_{n}", "tiny", "measured", blocks, sizes))
    return tuple(out)


# ------------------------------------------------------------------------------------------- flagged_independent
@functools.lru_cache(maxsize=None)
def flagged_frames():
    """70 tiny blocks under FLG 0x20. Every block is 3 literals and a match inside them (offset 1..3: no rewrite),
    but one: at index `at` the match has offset literals + 4 and reads the 4 bytes below the block. rewrite_64:
    block 64 is 9 literals and a match of 4 at offset 8 -- inside the block, but the reference's rewrite of the 4
    bytes before it reads 3 bytes below the block (a dependence in the reference modes only)."""
    out = []
    for at in (1, 63, 64, 65, 69, "rewrite_64"):
        m = S.Maker(9600 + (at if isinstance(at, int) else 64))
        blocks, sizes = [], []
        for k in range(70):
            ml = int(m.rng.integers(4, 8))
            if k == at:
                seq, size = (m.lits(3), 3 + 4, ml), 3 + ml
            elif at == "rewrite_64" and k == 64:
                seq, size = (m.lits(9), 8, 4), 13
            else:
                seq, size = (m.lits(3), int(m.rng.integers(1, 4)), ml), 3 + ml
            blocks.append((S.encode([seq], None), False))
            sizes.append(size)
        out.append(Frame(f"flagged_{at}", "flagged_independent", "measured", blocks, sizes, independent=True,
                         reaches=at if isinstance(at, int) else None, rewrite_reaches=64 if at == "rewrite_64" else at))
    return tuple(out)


# ------------------------------------------------------------------------------------------------------- rewrite
REWRITES = [(ml, ll) for ml in (4, 5, 6, 7) for ll in range(8 - ml)]       # first sequences: ll <= 7 - ml


def rewrite_opening(m, history, ll, ml):
    """A first sequence of ll literals and a match of ml < 8 bytes at an offset >= 8 for which the reference's
    rewrite of the 8 - ml bytes before the match's end changes a byte below the block: out[p] = out[p - offset]
    for p in [start + ml - 8, start), so the offset is drawn until history[p - offset] != history[p] for the first
    such p. history: the frame's bytes below the block."""
    base = history.size
    assert base == m.base and m.pos == 0 and ll + ml < 8
    p = base + ll + ml - 8
    while True:
        off = int(m.rng.integers(8, min(base + ll, 65535) + 1))
        if p - off >= 0 and history[p - off] != history[p]:
            return [m.seq(ll, ml, off=off)]


@functools.lru_cache(maxsize=None)
def rewrite_frames():
    """Layout: 3 blocks, blocks 1 and 2 open with such a sequence, every (ml, ll) once. Measured: behind 40
    literals, a predecessor block of 1, 2, 3 and 8 literals, then a block that opens with a match of 4 at 0
    literals: its rewrite covers the 4 bytes below it, the predecessor and (1, 2, 3) the end of the block before
    that; then more tiny blocks."""
    out = []
    for i in range(0, len(REWRITES), 2):
        blocks, sizes = [(fill_block(0), False)], [BS]
        for k, (ml, ll) in ((1, REWRITES[i]), (2, REWRITES[i + 1])):
            st, _, hist, _ = decode_blocks(blocks, sum(sizes), True)
            assert st == 0
            m = S.Maker(9700 + i + k, k * BS)
            size = BS if k == 1 else 500 + i
            blocks.append((fill_to(m, rewrite_opening(m, hist, ll, ml), size), False))
            sizes.append(size)
        out.append(Frame(f"rewrite_layout_{i}", "rewrite", "layout", blocks, sizes, rewrites=(1, 2)))
    for pred in (1, 2, 3, 8):
        m = S.Maker(9800 + pred)
        blocks, sizes = [(lit_block(m.lits(40)), False), (lit_block(m.lits(pred)), False)], [40, pred]
        m.base = 40 + pred
        st, _, hist, _ = decode_blocks(blocks, sum(sizes), True)
        blocks.append((S.encode(rewrite_opening(m, hist, 0, 4), None), False))
        sizes.append(4)
        m.base += 4
        more, msizes = tiny_blocks(m, 6)
        out.append(Frame(f"rewrite_pred_{pred}", "rewrite", "measured", blocks + more, sizes + msizes, rewrites=(2,)))
    return tuple(out)


# -------------------------------------------------------------------------------------------------------- errors
@functools.lru_cache(maxsize=None)
def errors_frames():
    """Layout frames of 4 blocks of random sequences with one failing block (Frame.says: fails = (index, status)):
      overrun_K    block K: 20 short sequences, then a run of 100 literals of which the block holds 50 (-2);
      offset0_K    block K: the same with the whole run and a match of offset 0 behind it (-3);
      cap_short / cap_mid  the content size ends one byte before / in the middle of a 100-byte run of the last
                   block (-1);
      clipped      the content size ends 3 bytes inside the last block's last match: status 0, the match's bytes
                   up to there.
    lp_*: the error cases of literal_pieces_common rebuilt at 64 KiB as the last block behind the history. And one
    measured frame, below_frame: block 0 has 100 bytes, block 1's match has offset 200."""
    out = []

    def failing(k, kind):
        m = S.Maker(9900 + k, k * BS)
        head = m.short(20)
        if kind == "overrun":
            return S.encode(head + [m.seq(100, 6)], None, LP.size_of(head) + 2 + 50)
        return S.encode(head + [m.seq(100, 6, off=0)] + m.short(5), m.lits(4))

    for kind, status in (("overrun", MALFORMED), ("offset0", OFFSET0)):
        for k in (1, 2, 3):
            blocks = [(failing(k, kind) if j == k else fill_block(j, BS if j < 3 else 4000), False) for j in range(4)]
            out.append(Frame(f"errors_{kind}_{k}", "errors", "layout", blocks, [BS, BS, BS, 4000], fails=(k, status)))
    m = S.Maker(9950, 3 * BS)
    seqs = m.short(20)
    before = m.pos
    last = S.encode(seqs + [m.seq(100, 6)] + m.short(5), m.lits(4))
    head = [(fill_block(j), False) for j in range(3)]
    for name, cut in (("cap_short", 99), ("cap_mid", 50)):
        out.append(Frame(f"errors_{name}", "errors", "layout", head + [(last, False)], [BS, BS, BS, before + cut],
                         fails=(3, TOO_SMALL)))
    m = S.Maker(9951, 3 * BS)
    last = S.encode(m.short(30) + [m.seq(20, 40)], None)
    out.append(Frame("errors_clipped", "errors", "layout", head + [(last, False)], [BS, BS, BS, m.pos - 3], clipped=3))
    for name, (seqs, fin, cap, opts) in LP.cases_errors(BS).items():
        comp = S.encode(seqs, fin, opts.get("truncate"))
        out.append(Frame(f"errors_lp_{name}", "errors", "layout", [(compact_history(), False), (comp, False)], [BS, cap],
                         fails=(1, opts["want"])))
    m = S.Maker(9952, 100)
    blocks = [(lit_block(m.lits(100)), False), (S.encode([m.seq(2, 8, off=200)] + m.short(3), m.lits(5)), False)]
    out.append(Frame("errors_below_frame", "errors", "measured", blocks, [100, m.pos + 5], fails=(1, DICT_OOB)))
    return tuple(out)


# -------------------------------------------------------------------------------------------------------- groups
@functools.lru_cache(maxsize=None)
def group(name):
    """The frames of one index call and one decode call."""
    if name == "layout":
        fs = boundary_frames() + history_fill_frames() + rewrite_frames() + errors_frames()
        return tuple(f for f in fs if f.kind == "layout")
    if name == "measured":
        fs = boundary_frames() + tiny_frames() + flagged_frames() + rewrite_frames() + errors_frames()
        return tuple(f for f in fs if f.kind == "measured")
    # the rebuilt cases in two halves per kind: a call's arena and its output both stay under 12 MiB
    fs = pieces_frames(name.split("_")[1])
    return fs[:len(fs) // 2] if name.endswith("_a") else fs[len(fs) // 2:]


GROUPS = ("layout", "measured", "pieces_layout_a", "pieces_layout_b", "pieces_measured_a", "pieces_measured_b")


def measured(name):
    return "measured" in name


@functools.lru_cache(maxsize=None)
def want(frame, exact):
    """What the frame batch owes for the frame, from the oracle on its blocks in order: (status, index of the
    failing block or None, the result array, the bytes written: the end of the last block that decoded, at most the
    content size). Two points are the header's contract (include/lz4mi.h, lz4mi_frames_decompress), not the
    reference's:
      - a failing block writes nothing (LZ4MI_LINKED's after-failure rule), so the array of a failing frame is that
        of the blocks before it -- the reference has already rewritten up to 4 bytes below such a block when it
        throws, and returns no result at all;
      - a block ends where its size word says and the bytes behind it read as 0 ("A block ends where its size word
        says" there), where the reference reads on in the frame: the frames of OVER_READ differ by that."""
    st, k, out, ends = decode_blocks(frame.blocks, frame.total, exact)
    if st:
        out = decode_blocks(frame.blocks[:k], frame.total, exact)[2]
    out.setflags(write=False)
    return st, k, out, min(frame.total, ends[-1] if ends else 0)


# Frames with a cut block (test_gpu_seqtable's fuzz9: its last match length field is cut off) that the reference
# decodes with status 0 by reading the byte behind the block, here the next block's size word: the reference's
# bytes (the single-frame call gives them, through its host route) differ from the batch's, see want(). In the
# layout twin the byte behind is the EndMark's 0 and both agree.
OVER_READ = ("st_fuzz9_measured",)


@functools.lru_cache(maxsize=None)
def arena(name, fill):
    import frames_chains_decode_common as D
    return D.pack16([f.data for f in group(name)], fill)


# -------------------------------------------------------------------------------------------------------- claims
def reads_history(frame, k, exact):
    """Whether block k's bytes (or status) change when everything below it is zeroed first."""
    st, kf, out, ends = decode_blocks(frame.blocks[:k + 1], frame.total, exact, data=frame.data)
    zst, zkf, zout, _ = decode_blocks(frame.blocks[:k + 1], frame.total, exact, zero_before=k, data=frame.data)
    lo = frame.starts()[k]
    return st != zst or (out[lo:] != zout[lo:]).any()


def differs_in_tail(frame, k):
    """Bytes of the 8 below block k where the reference's result differs from the spec's."""
    lo = frame.starts()[k]
    a, b = want(frame, False)[2], want(frame, True)[2]
    return int((a[max(0, lo - 8):lo] != b[max(0, lo - 8):lo]).sum())


def block_alone(comp, size, exact):
    """The oracle's status of a block decoded on its own."""
    return O.decompress_block(comp, size, js_compat=exact)[0]


@functools.lru_cache(maxsize=None)
def claims():
    """Every input's claim, on the oracle alone. -> {family: (frames, blocks, bytes where the reference's result
    differs from the spec's)}."""
    counts = {}
    for g in GROUPS:
        for f in group(g):
            # the frame decoder and the blocks in order agree, and the frame is what its kind and family say
            assert f.data[4] & 0x08 and bool(f.data[4] & 0x20) == f.independent and f.kind == ("measured" if measured(g) else "layout")
            assert len(f.blocks) == len(f.sizes) and all(0 < n <= BS for n in f.sizes), f.name
            if f.kind == "layout":
                assert all(n == BS for n in f.sizes[:-1]), f.name
            fails = f.says.get("fails")
            for exact in MODES:
                st, k, out, wrote = want(f, exact)
                ost, obytes = O.decompress_frame(f.data, verify_checksum=False, js_compat=exact, out_cap=f.total + 64)
                assert ost == st and (st, k) == ((fails[1], fails[0]) if fails else (0, None)), (f.name, exact, st, k)
                rst, rk, rout, _ = decode_blocks(f.blocks, f.total, exact, data=f.data)
                assert (rst, rk) == (st, k), f.name
                if st == 0:
                    assert obytes.size == f.total and (obytes == rout).all(), f.name
                    assert (rout != out).any() == (f.name in OVER_READ), f.name
                    if f.name in OVER_READ:
                        p, n = shard.frame_blocks(f.data)[1][2][:2]
                        assert lz4mi.host_block_read_end(f.data, p, n) == p + n + 1, f.name
                    assert wrote == f.total, f.name
                    if not f.says.get("clipped"):
                        _, _, _, ends = decode_blocks(f.blocks, f.total, exact, data=f.data)
                        assert [e - s for e, s in zip(ends, [0] + ends[:-1])] == f.sizes, f.name
                else:
                    assert wrote == sum(f.sizes[:k]), f.name
            n, nb, nd = counts.get(f.family, (0, 0, 0))
            counts[f.family] = (n + 1, nb + len(f.blocks), nd + int((want(f, False)[2] != want(f, True)[2]).sum()))
    by = lambda fam: [f for g in GROUPS for f in group(g) if f.family == fam]
    # boundary, history_fill: every block behind the first reads the blocks before it, in both modes
    for f in by("boundary") + by("history_fill"):
        for k in range(1, len(f.blocks)):
            if not f.blocks[k][1]:
                assert all(reads_history(f, k, e) for e in MODES), (f.name, k)
    for f in by("boundary"):
        for k, ll in zip((1, 2), f.says["opens"]):
            _, l0, off, ml = parse(f.blocks[k][0])[0]
            assert l0 == ll and off > ll, (f.name, k)
    names = {f.name for f in by("boundary")}
    assert {"boundary_ends_at_4", "boundary_across", "boundary_oldest", "boundary_oldest_ll", "boundary_byte0"} <= names
    assert {f"boundary_period_{p}" for p in PERIODS} <= names
    f = [f for f in by("boundary") if f.name == "boundary_byte0"][0]
    for k in (1, 2):
        _, ll, off, _ = parse(f.blocks[k][0])[0]
        assert f.starts()[k] + ll - off == 0
    f = [f for f in by("history_fill") if f.name == "fill_stored1"][0]
    assert f.blocks[1][1] and reads_history(f, 2, False)
    assert [f.data[4] & 0x14 for f in by("history_fill")] == [0, 0x04, 0, 0x14]
    # pieces_after_history: every valid case is there twice, a sequence of it reaches below the block, the
    # compressed layout (token positions, so the window-edge tokens and landings) is the base-0 case's
    cases = rebuilt_cases()
    valid = ["lp_" + n for n, c in LP.all_cases().items() if c[3][False][0] == 0 and c[3][True][0] == 0]
    valid += ["st_" + n for n, c in S.all_cases().items() if c[3][False][0] == 0 and c[3][True][0] == 0]
    assert list(cases) == valid and len(valid) >= 200
    for kind in ("layout", "measured"):
        assert [f.says["case"] for f in pieces_frames(kind)] == valid
    for name, (comp0, comp, cap, opts) in cases.items():
        assert comp.size == comp0.size and LP.tokens_of(comp) == LP.tokens_of(comp0), name
        if "token" in opts:
            toks = LP.tokens_of(comp)
            assert opts["token"] in toks and opts["land"] in toks + [int(comp.size)], name
        pos, reach = 0, False
        for _, ll, off, ml in sequences(comp):
            pos += ll
            reach = reach or off > pos
            pos += ml
        assert reach or name in NO_SEQUENCE_BELOW, name
    for name in NO_SEQUENCE_BELOW:
        assert name in cases
    for f in pieces_frames("measured"):
        _, ll, off, ml = parse(f.blocks[3][0])[0]
        assert off - ll == 5 and all(reads_history(f, 3, e) for e in MODES), f.name
    for kind in ("layout", "measured"):
        for f in pieces_frames(kind):
            k = 1 if kind == "layout" else 2
            assert f.says["case"] in NO_SEQUENCE_BELOW or all(reads_history(f, k, e) for e in MODES), f.name
    # tiny, rewrite: the reference's bytes differ from the spec's in the 8 bytes below a block
    assert [len(f.blocks) for f in by("tiny")] == [81, 65, 129]
    for f in by("tiny"):
        assert sum(1 for k in range(1, len(f.blocks)) if differs_in_tail(f, k)) >= len(f.blocks) // 4, f.name
        assert all(3 <= n <= 10 for n in f.sizes) and all(reads_history(f, k, False) for k in range(2, len(f.blocks)))
        for p, _ in f.blocks[1:]:
            (_, ll, off, ml), = parse(p)
            assert 1 <= ll <= 3 and 4 <= ml <= 7
    for f in by("rewrite"):
        for k in f.says["rewrites"]:
            _, ll, off, ml = parse(f.blocks[k][0])[0]
            assert 4 <= ml <= 7 and ll <= 7 - ml and off >= 8 and differs_in_tail(f, k), (f.name, k)
        for k in range(1, len(f.blocks)):
            if parse(f.blocks[k][0])[0][2]:          # (the measured frames' block 1 is literals only)
                assert all(reads_history(f, k, e) for e in MODES), (f.name, k)
    assert sorted(f.sizes[1] for f in by("rewrite") if f.kind == "measured") == [1, 2, 3, 8]
    seen = set()
    for f in by("rewrite"):
        if f.kind == "layout":
            seen |= {(parse(f.blocks[k][0])[0][3], parse(f.blocks[k][0])[0][1]) for k in (1, 2)}
    assert seen == set(REWRITES)
    # flagged_independent: exactly the named block reads below itself
    for f in by("flagged_independent"):
        assert len(f.blocks) == 70 and f.independent
        spec = [k for k, ((p, _), n) in enumerate(zip(f.blocks, f.sizes)) if block_alone(p, n, False) != 0]
        ref = [k for k, ((p, _), n) in enumerate(zip(f.blocks, f.sizes)) if block_alone(p, n, True) != 0 or FP.reads_below(p)]
        assert spec == ([f.says["reaches"]] if f.says["reaches"] is not None else []), (f.name, spec)
        assert ref == [f.says["rewrite_reaches"]], (f.name, ref)
        assert reads_history(f, ref[0], True)
    assert [f.says["rewrite_reaches"] for f in by("flagged_independent")] == [1, 63, 64, 65, 69, 64]
    # errors: the blocks that decode, and the failing block's head, read the blocks before them
    for f in by("errors"):
        fails = f.says.get("fails")
        for k in range(1, len(f.blocks)):
            if fails is None or k < fails[0]:
                assert all(reads_history(f, k, e) for e in MODES), (f.name, k)
    got = sorted((f.says["fails"][0], f.says["fails"][1]) for f in by("errors") if f.kind == "layout" and len(f.blocks) == 4
                 and "fails" in f.says)
    assert got == sorted([(k, s) for k in (1, 2, 3) for s in (MALFORMED, OFFSET0)] + [(3, TOO_SMALL)] * 2), got
    f = [f for f in by("errors") if f.name == "errors_clipped"][0]
    end = decode_blocks(f.blocks, f.total + 64, False)[3][-1]
    assert end == f.total + 3 and parse(f.blocks[3][0])[-1][2] != 0
    return counts


# Rebuilt cases in which no sequence's offset exceeds its position in the block: the one without any sequence.
NO_SEQUENCE_BELOW = ("st_final_at_0",)


# ------------------------------------------------------------- a lone block with history and a dictionary
# One block per call (nblocks == 1) at out_off = 64 KiB + r over the caller's bytes, a dictionary below out[0]: the
# one-wave kernel with c.dict, the path the chain never takes. boundary_oldest_r1 / _r7 / _r15 in the reference mode
# are the regression cases of the staged history of lz4mi_decompress_blocks (host pointers): the first match (offset
# 65535, 5 bytes, no literals) has a rewrite of the 3 bytes below the block that reads 65538..65536 bytes below the
# block's start, of which the call used to stage 65536 (r = 0 reads out[0] and below, which passed). The rebuilt cases' sources lie in the caller's bytes
# below the block; dict_*: a block at out_off = 40 + r whose first match starts 3 bytes (reach3), 6 bytes (reach6: more
# than the 5-byte dictionary holds, DICT_OOB with it) and 60000 bytes (far: DICT_OOB with 5 bytes) below out[0].
LONE_REBUILT = ("lp_ladder_all", "lp_max_runs", "lp_final_33_after_run", "lp_remap_split_40_16_c1",
                "lp_remap_inside_255_c0", "lp_edge_1000_1088_mid", "lp_edge_1023_1089_ends", "lp_twice_828",
                "lp_first_too_long")
LONE_BOUNDARY = (("ends_at_4", 0), ("across", 2), ("period_3", 0), ("period_16", 1), ("oldest", 0), ("oldest_ll", 3))
DICT_REACH = (("dict_reach3", 3), ("dict_reach6", 6), ("dict_far", 60000))
D_RESIDUES = (0, 1, 7, 15)


@functools.lru_cache(maxsize=None)
def lone_dictionaries():
    rng = np.random.default_rng(9960)
    return {"d64k": frozen(rng.integers(0, 256, BS, dtype=np.uint8)), "d5": frozen(rng.integers(0, 256, 5, dtype=np.uint8))}


@functools.lru_cache(maxsize=None)
def lone_inputs():
    """-> [(name, block, out_off, the caller's array: random bytes below out_off and 0xA5 from there, dictionary name)]"""
    res = []
    rng = np.random.default_rng(9961)
    below = rng.integers(0, 256, BS + 16, dtype=np.uint8)
    blocks = [(n, rebuilt_cases()[n][1]) for n in LONE_REBUILT]
    variants = dict(boundary_variants())
    for i, (name, ll) in enumerate(LONE_BOUNDARY):
        off, ml = variants[name](ll)
        m = S.Maker(9970 + i, BS)
        blocks.append(("boundary_" + name, frozen(fill_to(m, opening(m, ll, off, ml), 1500))))
    for r in D_RESIDUES:
        for name, comp in blocks:
            for dname in lone_dictionaries():
                res.append((f"{name}_r{r}_{dname}", comp, BS + r, dname))
        for i, (name, reach) in enumerate(DICT_REACH):
            m = S.Maker(9980 + i, 40 + r)
            comp = frozen(fill_to(m, opening(m, 2, 40 + r + 2 + reach, 12), 600))
            for dname in lone_dictionaries():
                res.append((f"{name}_r{r}_{dname}", comp, 40 + r, dname))
    out = []
    for name, comp, out_off, dname in res:
        size = O.decompress_block(comp, 1 << 17, dictionary=lone_dictionaries()["d64k"],
                                  out=np.zeros(out_off + (1 << 17), dtype=np.uint8), out_off=out_off)[1]
        init = np.full(out_off + size, 0xA5, dtype=np.uint8)
        init[:out_off] = below[:out_off]
        out.append((name, comp, out_off, frozen(init), dname))
    return tuple(out)


def lone_expected(item, exact):
    name, comp, out_off, init, dname = item
    st, w, arr = O.decompress_block(comp, 0, out=init.copy(), out_off=out_off, dictionary=lone_dictionaries()[dname],
                                    js_compat=exact)
    return st, w, arr


def lone_decode(item, exact):
    """One lz4mi_decompress_blocks call of one block on a copy of the caller's array. -> (status, out_len, array)"""
    name, comp, out_off, init, dname = item
    d = lone_dictionaries()[dname]
    arr = init.copy()
    one = lambda v, t: np.array([v], dtype=t)
    in_off, in_len, o_off, o_cap = one(0, np.uint64), one(comp.size, np.uint32), one(out_off, np.uint64), one(arr.size - out_off, np.uint32)
    out_len, status = np.zeros(1, dtype=np.uint32), np.zeros(1, dtype=np.int32)
    rc = lz4mi.lib().lz4mi_decompress_blocks(comp.ctypes.data, in_off.ctypes.data, in_len.ctypes.data, arr.ctypes.data,
                                             o_off.ctypes.data, o_cap.ctypes.data, d.ctypes.data, d.size,
                                             out_len.ctypes.data, status.ctypes.data, 1, lz4mi.JS_EXACT if exact else 0, None)
    assert rc == 0, (name, rc)
    return int(status[0]), int(out_len[0]), arr


def lone_mismatches():
    """Every lone input in both modes against the oracle: status, length and the whole array (the footprint rule: a
    byte the oracle did not change is unchanged); a failing block leaves the array as it was. -> list of findings"""
    lz4mi.init(0)
    wrong = []
    for item in lone_inputs():
        for exact in MODES:
            est, ew, earr = lone_expected(item, exact)
            st, n, arr = lone_decode(item, exact)
            if st != est:
                wrong.append((item[0], exact, "status", st, est))
            elif est == 0 and (n != ew or (arr != earr).any()):
                wrong.append((item[0], exact, "bytes", n, ew, int(np.argmax(arr != earr)), int((arr != earr).sum())))
            elif est != 0 and (n != 0 or (arr != item[3]).any()):
                wrong.append((item[0], exact, "a failing block wrote", n))
    return wrong


@functools.lru_cache(maxsize=None)
def lone_claims():
    items = lone_inputs()
    assert len(items) == 4 * 2 * (len(LONE_REBUILT) + len(LONE_BOUNDARY) + len(DICT_REACH))
    for item in items:
        name, comp, out_off, init, dname = item
        fail = dname == "d5" and (name.startswith("dict_reach6") or name.startswith("dict_far"))
        for exact in MODES:
            st, w, arr = lone_expected(item, exact)
            assert st == (DICT_OOB if fail else 0) and (fail or out_off + w == init.size), (name, exact, st)
            if not fail:
                # the block's bytes depend on the caller's bytes below it -- or, for dict_*, on the dictionary
                z, zd = init.copy(), lone_dictionaries()[dname]
                if name.startswith("dict_"):
                    zd = np.zeros_like(zd)
                else:
                    z[:out_off] = 0
                _, _, zarr = O.decompress_block(comp, 0, out=z, out_off=out_off, js_compat=exact, dictionary=zd)
                assert (zarr[out_off:] != arr[out_off:]).any(), (name, exact)
    return True
