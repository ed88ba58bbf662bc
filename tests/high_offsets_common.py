"""Shared by tests/test_high_offsets_cpu.py and tests/test_gpu_high_offsets.py: the device-pointer entry points
with offsets beyond 4 GiB and with blocks that lie across the 2^32 boundary.

Every device-pointer call takes a base pointer and arrays of 64-bit offsets; a kernel that drops one of them to 32
bits reads or writes at `offset mod 2^32`. The arena here is a real allocation of ARENA = 2^32 + 128 MiB bytes (two of
them on the device: inputs, outputs), so such a position lies inside the arena: the bug shows as a wrong byte or as a
stray store that the whole-arena check finds, never as a fault.

A case is a layout an existing test already builds -- an image (the bytes around the slots included) plus the slots'
offsets relative to the image -- and a placement translates it: the image goes to arena position D, every offset
becomes offset + D. D is always a multiple of 16, so that all placements take the same alignment paths and a
difference between two of them is the offset's alone:
    LOW                 D = 64 KiB: the control run (if it fails too, the cause is not the offset);
    HIGH                D = 2^32 + 64 KiB: every offset is above 2^32;
    cross(name, where)  D puts 2^32 at a position of the slot `name`: `start` (the slot begins at 2^32), `end` (it ends
                        there), `byte1` and `mid` (interior). The position is the nearest one that keeps D = 0 (mod 16)
                        -- exact where the slot's offset allows it, which the layouts here arrange for the slots they
                        cross at `start` and `end`; `byte1` of a 16-aligned slot is its byte 16. The slots below lie
                        under 2^32 and those above over it, so a crossed batch is a mixed batch as well.
The input and the output arena of a case get their own placement.

The whole-arena footprint: an arena is filled once with one byte c (0xA5; one test per entry point runs again on 0x5A,
so that a stray store cannot equal both); a case's images are written over it (windows), the call runs, the windows are
copied back and reset to c, and then no byte of the whole arena may differ from c. A stray store at `p` is reported
with the slot whose position is p + 2^32, if there is one ("alias of slot k"). The CPU test asserts for every case
that no window overlaps another window or the alias of a high one, which is what makes that diagnosis valid.

Positions in results (POSITION_FIELDS) are compared after subtracting D; everything else as it stands.
"""
import functools

import numpy as np

import footprint_common as FP
import frames_chain_common as CH
import frames_common as FC
import frames_enc_common as FE
import lz4mi
import oracle as O
import verify_common as V
from linked_exact_common import in_order
from lz4mi import frame as F
from lz4mi import shard
from test_gpu_seqtable import build_cases

B32 = 2 ** 32
ARENA = 2 ** 32 + (128 << 20)
CHUNK = 256 << 20            # the whole-arena check's piece
MARGIN = FP.MARGIN
LOW_D, HIGH_D = 65536, B32 + 65536
FILL, FILL2 = 0xA5, 0x5A
LOW, HIGH = ("low",), ("high",)
WHERE = ("start", "byte1", "mid", "end")
OK, TOO_SMALL, MALFORMED, OFFSET0, DICT_OOB, RANGE, CROSS, ERR_ARG = 0, -1, -2, -3, -4, -8, -9, -101
BAD_SUM = V.ERR_BLOCK_CHECKSUM
SPAN = 1 << 30               # csrc/lz4mi_expand.hip kSpanMax
SPAN_ARENA = B32 + SPAN + (128 << 20)   # the one case whose lowest slot lies above 2^32 with a second one 2^30 higher
SMALL_BATCH = lz4mi.SMALL_BLOCKS + 8
# the result fields that hold positions in `in` / `out` (compared after subtracting the arena's D)
POSITION_FIELDS = {"frames_index": ("blk_in_off",), "frames_plan": ("blk_in_off",), "frames_compress": ("finfo[5]",)}


def cross(name, where):
    assert where in WHERE
    return ("cross", name, where)


def place_id(p):
    return p[0] if len(p) == 1 else f"x-{p[1]}-{p[2]}"


def pair_id(pp):
    return f"in:{place_id(pp[0])}/out:{place_id(pp[1])}"


def alias(pos):
    assert pos >= B32
    return pos - B32


def window(off, size):
    """The slot and MARGIN bytes on either side -> (start, length)."""
    return off - MARGIN, size + 2 * MARGIN


def translate(image, offs, D):
    """An arena image plus offsets, moved by D -> ((position, bytes) of the image, offsets + D)."""
    assert D % 16 == 0 and D >= 0
    return (D, image), [int(o) + D for o in offs]


def pattern(n, at=0):
    """footprint_common.pattern(run 0), continued from index `at`."""
    return ((131 * (np.arange(n, dtype=np.int64) + at) + 7) & 255).astype(np.uint8)


def cross_at(off, size, where):
    """The position inside a slot at image offset `off` that cross(., where) puts 2^32 at."""
    lo, hi, want = {"start": (0, size, 0), "byte1": (1, size - 1, 1), "mid": (1, size - 1, size // 2),
                    "end": (0, size, size)}[where]
    r = (-off) % 16
    cands = [p for p in (r + 16 * j for j in range((want - r) // 16 - 1, (want - r) // 16 + 3)) if lo <= p <= hi]
    assert cands, (off, size, where)
    return min(cands, key=lambda p: (abs(p - want), p))


class Side:
    """One arena's share of a case: pieces (image offset, bytes) and named slots (name, image offset, size)."""

    def __init__(self, pieces, slots):
        self.pieces = [(int(r), np.ascontiguousarray(d, dtype=np.uint8)) for r, d in pieces]
        self.slots = [(str(n), int(o), int(s)) for n, o, s in slots]
        assert len({n for n, _, _ in self.slots}) == len(self.slots)

    @classmethod
    def image(cls, image, slots):
        return cls([(0, image)], slots)

    def slot(self, name):
        return next((o, s) for n, o, s in self.slots if n == name)

    def with_image(self, image):
        assert len(self.pieces) == 1 and image.size == self.pieces[0][1].size
        return Side([(0, image)], self.slots)


class Placed:
    def __init__(self, side, place):
        self.side, self.place = side, place
        if place == LOW:
            self.D = LOW_D
        elif place == HIGH:
            self.D = HIGH_D
        else:
            off, size = side.slot(place[1])
            self.D = B32 - off - cross_at(off, size, place[2])

    def pos(self, name):
        return self.D + self.side.slot(name)[0]

    def offs(self, names=None):
        names = [n for n, _, _ in self.side.slots] if names is None else names
        return [self.pos(n) for n in names]

    def windows(self):
        return [(self.D + r, d.size) for r, d in self.side.pieces]

    def describe(self, p):
        """An arena position, named: the alias of a slot or of a window, inside a window, or neither."""
        for n, o, s in self.side.slots:
            a = self.D + o
            if a + s > B32 and max(a, B32) - B32 <= p < a + s - B32:
                return f"arena position {p} = alias of slot {n} (its byte {p + B32 - a}; the slot lies at {a})"
        for a, n in self.windows():
            if a + n > B32 and max(a, B32) - B32 <= p < a + n - B32:
                return f"arena position {p} = alias of the window at {a} (of position {p + B32})"
        for a, n in self.windows():
            if a <= p < a + n:
                return f"arena position {p}: inside the window at {a}"
        return f"arena position {p}: outside every window and alias"


def check_placed(pl, size=ARENA):
    """The placement arithmetic the alias diagnosis rests on; -> the position of 2^32 inside the crossed slot."""
    assert pl.D % 16 == 0 and pl.D >= 0, pl.D
    wins = sorted(pl.windows())
    for a, n in wins:
        assert 0 <= a and a + n <= size, (pl.place, a, n)
    for (a, n), (b, _) in zip(wins, wins[1:]):
        assert a + n <= b, (pl.place, "windows overlap", a, n, b)
    for a, n in wins:
        if a + n > B32:
            lo, hi = max(a, B32) - B32, a + n - B32
            for b, m in wins:
                assert hi <= b or b + m <= lo, (pl.place, "the alias of a high window overlaps a window", a, b)
    for name, o, s in pl.side.slots:
        assert any(a <= pl.D + o and pl.D + o + s <= a + n for a, n in wins), (name, "slot outside its window")
    if pl.place == LOW:
        assert all(pl.D + o + s < B32 for _, o, s in pl.side.slots)
        return None
    if pl.place == HIGH:
        assert all(pl.D + o >= B32 for _, o, s in pl.side.slots)
        return None
    _, name, where = pl.place
    off, size = pl.side.slot(name)
    p = B32 - pl.D - off
    want = {"start": 0, "byte1": 1, "mid": size // 2, "end": size}[where]
    assert 0 <= p <= size and abs(p - want) < 16, (pl.place, p, want)
    if where in ("byte1", "mid"):
        assert 0 < p < size
    if (want + off) % 16 == 0:
        assert p == want
    for n, o, s in pl.side.slots:       # a mixed batch: what ends below the slot is under 2^32, what starts above over
        if o + s <= off:
            assert pl.D + o + s <= B32
        if o >= off + size:
            assert pl.D + o >= B32
    return p


def layout(sizes, guard=FP.GUARD, residues=FP.RESIDUES, pin=None, first=MARGIN):
    """Ascending slots at image offsets congruent to `residues` (mod 16) in turn, `guard` bytes apart at least;
    pin: {index: residue}."""
    pin = pin or {}
    offs, at = [], first
    for k, n in enumerate(sizes):
        r = pin.get(k, residues[k % len(residues)])
        off = at + ((r - at) % 16)
        offs.append(off)
        at = off + int(n) + guard
    return offs


def side_of(names, datas, sizes, guard, residues=FP.RESIDUES, pin=None):
    """An image of the pattern with `datas` (None: an output slot, left as pattern) at layout(sizes)."""
    offs = layout(sizes, guard, residues, pin)
    img = pattern(offs[-1] + sizes[-1] + MARGIN)
    for o, d in zip(offs, datas):
        if d is not None:
            img[o:o + d.size] = d
    return Side.image(img, list(zip(names, offs, sizes)))


class Case:
    """name, the input and output sides (either may be None), the placement pairs it runs at."""

    def __init__(self, name, inp, out, places, size=ARENA):
        self.name, self.inp, self.out, self.places, self.size = name, inp, out, list(places), size


def pairs(in_places, out_places):
    """(LOW, LOW), (HIGH, HIGH), then each cross of one arena with the other arena high."""
    return ([(LOW, LOW), (HIGH, HIGH)] + [(p, HIGH) for p in in_places] + [(HIGH, p) for p in out_places])


# ------------------------------------------------------------------------------------------------ XXH32
XXH_LENS = (0, 1, 15, 16, 17, 4095, 4096 + 5, 70000)
XXH_RES16 = (0, 1, 2, 15)          # start residues 0, 1, 2, 3 (mod 4); the first and last as cross() needs them
XXH_PLACES = (LOW, HIGH, cross("n70000_r0", "start"), cross("n70000_r3", "byte1"), cross("n70000_r0", "mid"),
              cross("n70000_r0", "end"))


@functools.lru_cache(maxsize=None)
def xxh_case():
    src = O.generate("random", 31, 70000 + 64)
    names, datas, pin = [], [], {}
    for k, n in enumerate(XXH_LENS):
        for r in range(4):
            pin[len(names)] = XXH_RES16[r]
            names.append(f"n{n}_r{r}")
            datas.append(src[(k + r) % 5:(k + r) % 5 + n])
    side = side_of(names, datas, [d.size for d in datas], 33, pin=pin)
    return Case("xxh32", side, None, [(p, None) for p in XXH_PLACES]), datas


def xxh_expected(datas, seed, standard):
    return [(O.xxh32_std if standard else O.xxh32)(d, seed) for d in datas]


# ------------------------------------------------------------------------------------ block checksums
VERIFY_FRAMES = ("text4", "randtail")
VERIFY_ALIGNED = {"text4": 1, "randtail": 0}     # the block whose payload ends at 0 (mod 16)
VERIFY_PLACES = (LOW, HIGH, cross("text4_b1", "mid"), cross("text4_b1", "end"), cross("randtail_b0", "mid"),
                 cross("randtail_b0", "end"))
VERIFY_DAMAGED = "text4_b2"


@functools.lru_cache(maxsize=None)
def verify_case():
    """The records of the two frames with block checksums -> (case, words, stored flags); the records ascend."""
    at, frames, slots, words, stored = MARGIN, [], [], [], []
    for name in VERIFY_FRAMES:
        f = CH.expected(name, 65536, (True, True, True))
        blocks = shard.frame_blocks(f)[1]
        p, n, _ = blocks[VERIFY_ALIGNED[name]]
        at += 40
        at += (-(at + p + n)) % 16
        frames.append((at, f))
        for k, (p, n, st) in enumerate(blocks):
            slots.append((f"{name}_b{k}", at + p, n))
            words.append(n | (0x80000000 if st else 0))
            stored.append(st)
        at += f.size
    img = pattern(at + MARGIN)
    for o, f in frames:
        img[o:o + f.size] = f
    return Case("verify_blocks", Side.image(img, slots), None, [(p, None) for p in VERIFY_PLACES]), words, stored


def verify_variants():
    """name -> (side, in_total relative to the image or None, expected statuses from the oracle hash alone)."""
    case, words, _ = verify_case()
    side = case.inp
    img = side.pieces[0][1]
    offs = [o for _, o, _ in side.slots]
    out = {"clean": (side, None, V.expected(img, offs, words))}
    bad = img.copy()
    o, n = side.slot(VERIFY_DAMAGED)
    bad[o + n + 1] ^= 0x20
    out["damaged"] = (side.with_image(bad), None, V.expected(bad, offs, words))
    o, n = side.slots[-1][1:]
    out["cut"] = (side, o + n + 2, V.expected(img, offs, words, o + n + 2))
    return out


# ------------------------------------------------------------------------------------------ decode
@functools.lru_cache(maxsize=None)
def decode_blocks():
    """name -> (compressed block, capacity): the seven blocks of the decode, sizes and small-path cases."""
    cases = build_cases()
    # (text behind 16 random bytes, like frames_common.text_content: no tail rewrite reads below the block's start)
    text = np.concatenate([O.generate("random", 1, 16), O.generate("text", 1, 70000 - 16)])
    rows = [("empty", np.zeros(0, dtype=np.uint8), 0)]
    for name, raw in (("n13", O.generate("text", 3, 13)), ("rand5000", O.generate("random", 5, 5000)), ("text70000", text),
                      ("tiles216", O.generate("tiles216", 9, 300000))):
        rows.append((name, O.compress_block_bytes(raw), raw.size))
    rows.append(("clean", cases["cap_exact"][0], cases["cap_exact"][1]))
    rows.append(("dict_oob", cases["far_at_64"][0], cases["far_at_64"][1]))
    return tuple(rows)


DECODE_IN_PLACES = (cross("b4_tiles216", "mid"),)
DECODE_OUT_PLACES = tuple(cross("b4_tiles216", w) for w in WHERE)


def decode_tiles(nblocks=None):
    """The index of the tiles216 block that is crossed: block 4, or its copy in the middle of a repeated batch."""
    return 4 + 7 * (nblocks // 14) if nblocks else 4


def decode_places(nblocks=None):
    name = f"b{decode_tiles(nblocks)}_tiles216"
    return pairs((cross(name, "mid"),), tuple(cross(name, w) for w in WHERE))


DICT_PLACES = pairs(DECODE_IN_PLACES[:1], DECODE_OUT_PLACES[2:3])
LONE_PLACES = ((LOW, LOW), (HIGH, HIGH), (HIGH, cross("blk", "start")))


def decode_sides(rows, tiles=4):
    """-> (input side, output side) of the blocks; slot names b<index>_<name>. The tiles216 block's output slot
    `tiles` is 16-aligned (its 300000 bytes end 16-aligned as well)."""
    names = [f"b{j}_{n}" for j, (n, _, _) in enumerate(rows)]
    inp = side_of(names, [c for _, c, _ in rows], [c.size for _, c, _ in rows], 33)
    out = side_of(names, [None] * len(rows), [cap for _, _, cap in rows], FP.GUARD, pin={tiles: 0})
    return inp, out


@functools.lru_cache(maxsize=None)
def _alone(comp, cap, js):
    return O.decompress_block(np.frombuffer(comp, dtype=np.uint8), cap, js_compat=js)


def expected_decode(out_side, rows, js):
    """A batch (more than one block) of independent blocks: -> (image, care, statuses, lengths) from the oracle's
    decode of each block alone; a reference below the block's own start lands in `out` at these offsets (the slots lie
    above 64 KiB), which the contract reports as ERR_CROSS_BLOCK where the oracle, alone, says DICT_OOB."""
    assert len(rows) > 1
    img = out_side.pieces[0][1].copy()
    care = np.ones(img.size, dtype=bool)
    status, lens = [], []
    for (name, comp, cap), (_, off, _) in zip(rows, out_side.slots):
        st, w, res = _alone(comp.tobytes(), cap, js)
        if st == DICT_OOB:
            st = CROSS      # (a tail rewrite below the block, in a reference mode, is ERR_CROSS_BLOCK too)
        assert st or not (js and FP.reads_below(comp)), name
        status.append(int(st))
        if st:
            lens.append(0)
            care[off:off + cap] = False
        else:
            lens.append(int(w))
            img[off:off + cap] = res[:cap]
    return img, care, status, lens


@functools.lru_cache(maxsize=None)
def decode_case(nblocks=None):
    rows = decode_blocks()
    if nblocks:
        rows = tuple(rows[j % 7] for j in range(nblocks))
    inp, out = decode_sides(rows, decode_tiles(nblocks))
    return Case(f"decode{nblocks or 7}", inp, out, decode_places(nblocks)), rows


@functools.lru_cache(maxsize=None)
def dict_case():
    """The seven blocks and one that reaches 300 bytes below its start, with a dictionary: below out[0] only."""
    cases = build_cases()
    comp, cap, d = cases["dict_inside"]
    rows = decode_blocks() + (("dict_inside", comp, cap),)
    inp, out = decode_sides(rows)
    return Case("decode_dict", inp, out, DICT_PLACES), rows, np.frombuffer(d, dtype=np.uint8)


@functools.lru_cache(maxsize=None)
def chain_blocks(name):
    """(payloads, stored flags, capacities) of the content's dependent frame (frames_chain_common)."""
    f = CH.oracle_frame(name, 65536, False, False, True)
    blocks = shard.frame_blocks(f)[1]
    n = CH.content(name).size
    return ([f[p:p + m] for p, m, _ in blocks], [st for _, _, st in blocks],
            [min(65536, n - k * 65536) for k in range(len(blocks))])


@functools.lru_cache(maxsize=None)
def lone_case():
    """Block 1 of text4's dependent frame alone in a call, block 0's 64 KiB of content directly below its slot."""
    pays, _, caps = chain_blocks("text4")
    hist = CH.content("text4")[:65536]
    inp = side_of(["blk"], [pays[1]], [pays[1].size], 33)
    img = pattern(MARGIN + 65536 + caps[1] + MARGIN)
    img[MARGIN:MARGIN + 65536] = hist
    out = Side.image(img, [("blk", MARGIN + 65536, caps[1])])
    return Case("decode_lone", inp, out, LONE_PLACES), pays[1], caps[1]


def expected_lone(js):
    case, pay, cap = lone_case()
    img = case.out.pieces[0][1].copy()
    off = case.out.slot("blk")[0]
    st, w, res = O.decompress_block(pay, cap, out=img[:off + cap].copy(), out_off=off, js_compat=js)
    img[:off + cap] = res
    return img, int(st), int(w)


# ---------------------------------------------------------------------------------------- linked decode
LINKED_IN_PLACES = (cross("text4_b1", "mid"),)
LINKED_OUT_PLACES = (cross("text4_b1", "mid"), cross("text4_b1", "end"))


LINKED_PLACES = pairs(LINKED_IN_PLACES, LINKED_OUT_PLACES)


@functools.lru_cache(maxsize=None)
def linked_case():
    """text4's four dependent blocks in contiguous slots, then randtail's three (block 0 stored), one linked call."""
    names, pays, stored, caps = [], [], [], []
    for name in ("text4", "randtail"):
        p, s, c = chain_blocks(name)
        names += [f"{name}_b{k}" for k in range(len(p))]
        pays += p
        stored += s
        caps += c
    inp = side_of(names, pays, [p.size for p in pays], 33)
    offs, at = [], MARGIN
    for k, n in enumerate(names):
        if n.endswith("_b0"):
            at += FP.GUARD
            at += (-at) % 16
        offs.append(at)
        at += caps[k]
    out = Side.image(pattern(at + MARGIN), list(zip(names, offs, caps)))
    return Case("linked", inp, out, LINKED_PLACES), pays, stored, caps


def expected_linked(exact):
    case, pays, stored, caps = linked_case()
    img = case.out.pieces[0][1]
    offs = [o for _, o, _ in case.out.slots]
    st, ln, arr = (in_order if exact else FP._in_order_spec)(pays, offs, caps, img, None, stored)
    return arr, st, ln


def span_layouts():
    """name -> (in offsets, out offsets) of two blocks, relative to the lowest slot: `in` and `out` spread by just
    under and by at least 2^30 as lz4mi_linked_prep_kernel counts it (in_off - lowest + len >= 2^30; out_off - lowest
    + cap + 65536 >= 2^30)."""
    _, (_, comp, cap), _ = span_blocks()
    near_in = near_out = 2 * MARGIN + 16384      # (the two windows stay apart)
    return {"in_under": ((0, SPAN - 1 - comp.size), (0, near_out)), "in_at": ((0, SPAN - comp.size), (0, near_out)),
            "out_under": ((0, near_in), (0, SPAN - 1 - cap - 65536)), "out_at": ((0, near_in), (0, SPAN - cap - 65536))}


@functools.lru_cache(maxsize=None)
def span_blocks():
    rows = tuple((f"t{k}", O.compress_block_bytes(O.generate("text", 60 + k, 5000)), 5000) for k in range(2))
    return rows[0], rows[1], [O.generate("text", 60 + k, 5000) for k in range(2)]


def span_case(which):
    """Two pieces per side, each block with MARGIN bytes of pattern around it; image offsets start at MARGIN."""
    r0, r1, _ = span_blocks()
    ins, outs = span_layouts()[which]
    sides = []
    for offs, datas, sizes in ((ins, (r0[1], r1[1]), (r0[1].size, r1[1].size)), (outs, (None, None), (r0[2], r1[2]))):
        pieces, slots = [], []
        for k, (o, d, n) in enumerate(zip(offs, datas, sizes)):
            w = pattern(n + 2 * MARGIN, o)
            if d is not None:
                w[MARGIN:MARGIN + n] = d
            pieces.append((o, w))
            slots.append((f"t{k}", o + MARGIN, n))
        sides.append(Side(pieces, slots))
    return Case(f"span_{which}", sides[0], sides[1], [(LOW, LOW), (HIGH, HIGH)], size=SPAN_ARENA)


def expected_span(which, exact):
    """-> (the output pieces' images, statuses, lengths): each block decoded by the oracle in its own window (the
    reference's bytes with `exact`), the second one refused in the `_at` layouts."""
    case = span_case(which)
    rows = span_blocks()[:2]
    refused = which.endswith("_at")
    images, status, lens = [], [], []
    for k, ((_, piece), (_, comp, cap)) in enumerate(zip(case.out.pieces, rows)):
        img = piece.copy()
        if k == 1 and refused:
            status.append(ERR_ARG)
            lens.append(0)
        else:
            st, w, res = O.decompress_block(comp, cap, out=img[:MARGIN + cap].copy(), out_off=MARGIN, js_compat=exact)
            img[:MARGIN + cap] = res
            status.append(int(st))
            lens.append(int(w))
        images.append(img)
    return images, status, lens


# ---------------------------------------------------------------------------------------- batch encode
ENCODE_PLACES = pairs((cross("text300000", "mid"),), (cross("text300000", "byte1"), cross("text300000", "end")))


@functools.lru_cache(maxsize=None)
def encode_case():
    srcs = [(f"{kind}{n}", O.generate(kind, 80 + n % 7, n)) for kind in ("text", "tiles216")
            for n in (13, 5000, 65537, 300000)]
    srcs.append(("random65536", O.generate("random", 81, 65536)))
    names = [n for n, _ in srcs]
    datas = [d for _, d in srcs]
    k = names.index("text300000")
    inp = side_of(names, datas, [d.size for d in datas], 33)
    bounds = [O.compress_bound(d.size) for d in datas]
    # (the bound of 300000 bytes is 301192 = 8 (mod 16): the slot starts at 8 so that it ends 16-aligned)
    out = side_of(names, [None] * len(names), bounds, FP.GUARD, pin={k: (-bounds[k]) % 16})
    return Case("encode", inp, out, ENCODE_PLACES), datas


def expected_encode():
    case, datas = encode_case()
    img = case.out.pieces[0][1].copy()
    lens = []
    for d, (_, off, _) in zip(datas, case.out.slots):
        c = O.compress_block_bytes(d)
        img[off:off + c.size] = c
        lens.append(int(c.size))
    return img, lens


# ---------------------------------------------------------------------------------- frame batch decode
FRAMES_MODES = {"default": {}, "measure": {"measure": True}, "js_exact": {"js_exact": True},
                "verify_content": {"verify": True}}


def frames_crossed(mode):
    """The multi-block frame that is crossed: five blocks, independent, sized, with a content checksum; in the
    reference's bytes that one is declined (a tail rewrite reads below its block), so the two-block frame."""
    return "c65537_isc" if mode == "js_exact" else "cfive_isc"


def frames_places(mode):
    x = frames_crossed(mode)
    return pairs((cross(x, "mid"),), (cross(x, "mid"), cross(x, "end")))


def padded(arena):
    """An existing input arena with MARGIN bytes of pattern on either side (offsets grow by MARGIN)."""
    img = pattern(arena.size + 2 * MARGIN)
    img[MARGIN:MARGIN + arena.size] = arena
    return img


@functools.lru_cache(maxsize=None)
def frames_case(mode):
    """The zoo of frames_common, its frames' output slots sized by the host index (tests/test_frames_cpu.py pins it to
    the oracle) as tests/test_gpu_frames_batch.py lays them out -> (case, host index, live frames, totals)."""
    from lz4mi.frame import content_size_bound
    kw = FRAMES_MODES[mode]
    a, off, ln = FC.arena(0x00)
    idx = lz4mi.host_frames_index(a, off, ln, FC.need_blocks(), measure=kw.get("measure", False),
                                  js_exact=kw.get("js_exact", False))
    fi = idx["finfo"]
    live = [k for k in range(len(FC.NAMES))
            if not fi[k, 0] and not fi[k, 7] and int(fi[k, 2]) <= content_size_bound(int(ln[k]))]
    total = {k: int(fi[k, 3]) for k in live}
    inp = Side.image(padded(a), [(n, int(o) + MARGIN, int(m)) for n, o, m in zip(FC.NAMES, off, ln)])
    crossed = frames_crossed(mode)
    x = FC.NAMES.index(crossed)
    assert x in live
    out = side_of([FC.NAMES[k] for k in live], [None] * len(live), [total[k] for k in live], 48,
                  pin={live.index(x): (-total[x]) % 16})
    return Case(f"frames_{mode}", inp, out, frames_places(mode)), idx, live, total


def expected_frames(mode):
    """-> (image, care, {name: (status, decline)}, {name: the oracle's decoded frame}) as tests/test_gpu_frames_batch.py
    expects them: frames_common.expected_batch and the oracle's frame decoder."""
    case, idx, live, total = frames_case(mode)
    kw = FRAMES_MODES[mode]
    js, measure, verify = kw.get("js_exact", False), kw.get("measure", False), kw.get("verify", False)
    img = case.out.pieces[0][1].copy()
    care = np.ones(img.size, dtype=bool)
    want = {n: FC.expected_batch(n, js, measure, verify) for n in FC.NAMES}
    written = {}
    for k in live:
        name = FC.NAMES[k]
        st, dc = want[name]
        lo = case.out.slot(name)[0]
        if dc in (FC.LAYOUT, FC.DEPENDENT) or (st and st != FC.ERR_CHECKSUM and not dc):
            care[lo:lo + total[k]] = False
        elif not dc:
            ost, dec = O.decompress_frame(FC.zoo()[name], verify_checksum=False, js_compat=js)
            assert ost == 0 and dec.size <= total[k], name
            img[lo:lo + dec.size] = dec
            if dec.size < total[k]:                 # the zero tail up to the content size
                img[lo + dec.size:lo + total[k]] = 0
            written[name] = dec
    return img, care, want, written


# ---------------------------------------------------------------------------------- frame batch encode
ENC_KINDS = ("independent", "declining", "chains")
ENC_COMBOS = ((True, True, True), (False, False, False))     # (content checksum, content size, block checksum)


def enc_places(kind, combo):
    places = [(LOW, LOW), (HIGH, HIGH)]
    if kind == "chains":
        # the chain kernel's source ring refills across 2^32; 2^32 between two blocks of a chain; and, with block
        # checksums, the store-in-place digests and the pack pass's record positions across it
        places += [(cross("tiles300k", "mid"), HIGH), (cross("text4_blk0", "end"), HIGH)]
        if combo[2]:
            places.append((HIGH, cross("text4", "mid")))
    else:
        places.append((cross("tiles300k", "mid"), cross("tiles300k" if kind == "independent" else "text300", "mid")))
    return places


def with_block_checksums(f, bs, indep, csum, n, sized):
    """An oracle frame re-assembled with FLG 0x10: every record followed by the spec XXH32 of its payload."""
    parts = [np.frombuffer(F.header(bs, indep, csum, n if sized else None, None, True), dtype=np.uint8)]
    info, blocks = shard.frame_blocks(f)
    for pos, m, _ in blocks:
        pay = f[pos:pos + m]
        parts += [f[pos - 4:pos], pay, V.le32(O.xxh32_std(pay))]
    parts.append(V.le32(0))
    if csum:
        parts.append(f[info["end"]:info["end"] + 4])
    return np.concatenate(parts)


@functools.lru_cache(maxsize=None)
def expected_frame(name, kind, combo):
    """The frame the call writes, or None where the plan declines it (a multi-block dependent frame without chains)."""
    csum, sized, bsum = combo
    if kind != "independent":
        if kind == "declining" and len(CH.SHAPES[name]) > 1:
            return None
        return CH.expected(name, 65536, combo)
    f = CH.oracle_frame(name, 65536, True, csum, sized)
    return with_block_checksums(f, 65536, True, csum, CH.content(name).size, sized) if bsum else f


def enc_flags(kind, combo):
    csum, sized, bsum = combo
    return lz4mi.frames_enc_flags(kind == "independent", csum, sized, bsum, chains=kind == "chains")


def expected_plan(kind, combo, offs, lens, cap):
    if kind == "independent":
        return FE.closed_form_plan(lens, offs, 65536, (True,) + tuple(combo), cap)
    return CH.closed_form_plan(lens, offs, 65536, combo, cap, chains=kind == "chains")


@functools.lru_cache(maxsize=None)
def enc_case(kind, combo):
    """Group c64k of frames_chain_common: the sources' arena padded, the frames in slots of exactly their size."""
    _, _, names = CH.GROUPS["c64k"]
    a, off, ln = CH.arena("c64k", 0x00)
    slots = [(n, int(o) + MARGIN, int(m)) for n, o, m in zip(names, off, ln)]
    slots.append(("text4_blk0", slots[names.index("text4")][1], 65536))
    inp = Side.image(padded(a), slots)
    written = [n for n in names if expected_frame(n, kind, combo) is not None]
    sizes = [expected_frame(n, kind, combo).size for n in written]
    out = side_of(written, [None] * len(written), sizes, 48, residues=(1, 2, 3, 0))
    return Case(f"frames_enc_{kind}_{CH.combo_id(combo)}", inp, out, enc_places(kind, combo)), names, written


def expected_enc_image(kind, combo):
    case, names, written = enc_case(kind, combo)
    img = case.out.pieces[0][1].copy()
    for n in written:
        f = expected_frame(n, kind, combo)
        lo = case.out.slot(n)[0]
        img[lo:lo + f.size] = f
    return img


# ------------------------------------------------------------------------------------------ every case
def all_cases():
    """Every case of tests/test_gpu_high_offsets.py, for the placement checks of tests/test_high_offsets_cpu.py."""
    cases = [xxh_case()[0], verify_case()[0], decode_case()[0], decode_case(SMALL_BATCH)[0], dict_case()[0],
             lone_case()[0], linked_case()[0], encode_case()[0]]
    cases += [span_case(w) for w in span_layouts()]
    cases += [frames_case(m)[0] for m in FRAMES_MODES]
    cases += [enc_case(k, c)[0] for k in ENC_KINDS for c in ENC_COMBOS]
    return cases


# ------------------------------------------------------------------------------------ the device arena
class Arena:
    """ARENA bytes on the device, every byte c except inside the windows of the case that is running."""

    def __init__(self, torch, size=ARENA):
        self.torch, self.size, self.c, self.live = torch, size, None, []
        self.t = torch.empty(size, dtype=torch.uint8, device="cuda")

    @property
    def ptr(self):
        return self.t.data_ptr()

    def fill(self, c):
        if self.c != c:
            for a in range(0, self.size, CHUNK):
                self.t[a:a + CHUNK].fill_(c)
            self.c = c
        assert not self.live

    def load(self, placed):
        for (pos, n), (_, d) in zip(placed.windows(), placed.side.pieces):
            assert 0 <= pos and pos + n <= self.size
            self.t[pos:pos + n].copy_(self.torch.from_numpy(d))
            self.live.append((pos, n))

    def abandon(self):
        """The windows back to c without a check (after a call that raised)."""
        for pos, n in self.live:
            self.t[pos:pos + n].fill_(self.c)
        self.live = []

    def settle(self, placed, what):
        """The windows' bytes (one array per piece); the windows are reset to c and the whole arena checked."""
        got = [self.t[pos:pos + n].cpu().numpy() for pos, n in placed.windows()]
        for pos, n in self.live:
            self.t[pos:pos + n].fill_(self.c)
        self.live = []
        flags = self.torch.stack([(self.t[a:a + CHUNK] != self.c).any() for a in range(0, self.size, CHUNK)]).cpu().numpy()
        if flags.any():
            k = int(np.nonzero(flags)[0][0])
            chunk = self.t[k * CHUNK:(k + 1) * CHUNK]
            bad = self.torch.nonzero(chunk != self.c).flatten()
            p = int(bad[0]) + k * CHUNK
            v = int(self.t[p])
            for a in range(0, self.size, CHUNK):        # (leave the arena clean for the tests that follow)
                self.t[a:a + CHUNK].fill_(self.c)
            raise AssertionError(f"{what}: a stray store outside the windows, fill {self.c:#x}: {placed.describe(p)}, "
                                 f"value {v}; {int(bad.numel())} such byte(s) in its 256 MiB piece, "
                                 f"{int(flags.sum())} piece(s) touched")
        return got


def assert_image(got, image, care, placed, what):
    """A window against the expected image; the first difference is named by slot."""
    bad = np.nonzero((got != image) & care)[0] if care is not None else np.nonzero(got != image)[0]
    if bad.size:
        p = int(bad[0])
        where = next((f"slot {n} byte {p - o}" for n, o, s in placed.side.slots if o <= p < o + s), "outside the slots")
        raise AssertionError(f"{what}: {bad.size} wrong byte(s), first at image offset {p} (arena position "
                             f"{placed.D + p}), {where}: got {int(got[p])}, expected {int(image[p])}; "
                             f"last at {int(bad[-1])}")
