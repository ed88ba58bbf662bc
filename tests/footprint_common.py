"""Shared by tests/test_footprint_cpu.py and tests/test_gpu_footprint.py: WHERE the codec writes.

Every call runs on caller-owned arrays whose every byte is known beforehand (an arena: 64 KiB of
margin, the slots with 1 KiB guards between them at odd offsets, 64 KiB of margin), and the whole
array afterwards is compared with the image the CPU oracle says the reference leaves
(oracle.decompress_block with out=ARRAY, which clips at the capacity like a typed array). Each
case runs twice: run 0 on the pattern P[i] = (131 i + 7) & 255 with 0x00 around the input blocks,
run 1 on ~P with 0xFF around them and a valid-looking token (0x1F) directly behind each block, so
a stray store cannot equal both pre-fills and nothing outside in[in_off .. +in_len) may matter.

The blocks are hand-assembled with test_gpu_seqtable's encode/Maker: a short body and one last
sequence, decoded at the capacities around the decoded size N and inside the last match.
"""
import functools

import numpy as np

import oracle as O
from linked_exact_common import in_order, parse
from test_gpu_seqtable import Maker, build_cases, encode, first_far_reference

MARGIN = 65536        # bytes the test owns below out[0] / in[0] and behind the last slot
GUARD = 1024          # between two slots
SENTINELS = 64        # extra entries of out_len[] / status[] / hashes[]
FILL = 77             # their value, and that of the entries a call has to overwrite
RESIDUES = (1, 5, 15)  # slot offsets mod 16, in turn
OK, TOO_SMALL, MALFORMED, OFFSET0, DICT_OOB, RANGE, CROSS = 0, -1, -2, -3, -4, -8, -9
JS_MODES = ("js_exact", "js_compat", "linked_exact")
LINKED_MODES = ("linked", "linked_exact")


def pattern(n, run):
    p = ((131 * np.arange(n, dtype=np.int64) + 7) & 255).astype(np.uint8)
    return p if run == 0 else ~p


def layout(sizes, first=None, guard=GUARD, contiguous=(), page=1):
    """Ascending, disjoint slots of `sizes` bytes -> offsets (relative to out[0]): congruent to
    1, 5, 15 (mod 16) in turn with at least `guard` bytes between two slots; slot `page` (when
    there is one past slot 0) starts at a 4 KiB boundary + 4095; a slot in `contiguous` starts
    where its predecessor ends; `first`: slot 0's offset."""
    offs, at = [], 0
    for k, size in enumerate(sizes):
        if k == 0 and first is not None:
            off = first
        elif k in contiguous and k > 0:
            off = offs[-1] + sizes[k - 1]
        elif k == page and k > 0:
            off = ((at + 4095) & ~4095) + 4095
        else:
            r = RESIDUES[k % 3]
            off = at + ((r - at) % 16)
        offs.append(int(off))
        at = off + int(size) + guard
    return offs


class Regions:
    """Names the absolute positions of an arena: the margins, the guards, and each slot's head
    (its first 16 bytes), body and tail (behind the bytes the block produced)."""

    def __init__(self, offs, caps, lens=None):
        self.offs, self.caps = list(offs), list(caps)
        self.lens = list(lens) if lens is not None else list(caps)

    def where(self, pos):
        p = pos - MARGIN
        if p < 0:
            return "margin below out[0]"
        for k, (off, cap, ln) in enumerate(zip(self.offs, self.caps, self.lens)):
            if off <= p < off + cap:
                if p >= off + min(ln, cap):
                    return f"slot {k} tail"
                return f"slot {k} head" if p < off + 16 else f"slot {k} body"
            if p < off:
                return f"guard before slot {k}"
        return "margin after the last slot"


def assert_footprint(got, image, care, regions, what=""):
    """The whole array against the expected image wherever care is set; reports the first
    differing absolute position and the region it lies in."""
    assert got.shape == image.shape == care.shape, (what, got.shape, image.shape)
    bad = np.nonzero((got != image) & care)[0]
    if bad.size:
        p = int(bad[0])
        raise AssertionError(f"{what}: {bad.size} stray or wrong byte(s), first at arena position {p} "
                             f"(out[{p - MARGIN}]), in {regions.where(p)}: got {int(got[p])}, expected {int(image[p])}; "
                             f"last at {int(bad[-1])} in {regions.where(int(bad[-1]))}")


def assert_sentinels(arr, n, what=""):
    """Entries >= n of an out_len[] / status[] / hashes[] array still hold FILL."""
    bad = np.nonzero(np.asarray(arr)[n:] != FILL)[0]
    if bad.size:
        raise AssertionError(f"{what}: sentinel entry {n + int(bad[0])} (of {n} blocks) was written: "
                             f"{int(np.asarray(arr)[n + int(bad[0])])}")


# ---------------------------------------------------------------------------------------- the blocks
class Row:
    """One block of the table: name, compressed bytes, decoded size N, the capacities to decode it
    at, [start, end) of its last match (None: no match), whether it ends on that match (no final
    literals), its dictionary, and whether it is a stored block of a frame (payload = raw bytes)."""

    def __init__(self, name, comp, n, caps, match=None, ends_on_match=False, dictionary=None, stored=False,
                 lone_only=False, first=None):
        self.name, self.comp, self.n, self.caps = name, comp, n, caps
        self.match, self.ends_on_match, self.dictionary, self.stored = match, ends_on_match, dictionary, stored
        self.lone_only, self.first = lone_only, first


def _caps(n, match=None):
    caps = [n, n - 1, n - 15, n - 16, n - 17]
    if match is not None:
        caps += [match[0] + 1, match[0] + 16, match[1] - 1]
    out = []
    for c in caps:
        if c not in out:
            out.append(c)
    return out


def reads_below(comp):
    """Whether a rewrite of the reference's tail copy (offset >= 8, match length < 8) reads bytes below
    the block's own start: in a batch of independent blocks the reference modes report
    ERR_CROSS_BLOCK for such a block, like any back-reference out of the block."""
    pos = 0
    try:
        for _, ll, off, ml in parse(comp):
            pos += ll
            if off == 0:
                break
            if off >= 8 and ml < 8 and 0 <= pos - off < 8 - ml:
                return True
            pos += ml
    except IndexError:                                # (a truncated block)
        pass
    return False


def _row(name, seed, body, last, final, **kw):
    """body: number of four-byte sequences; last: (literals, match length, offset) or None;
    final: number of final literals or None. (The seed moves on until no rewrite reads below the
    block: the lone-only row f1_src_below has that case.)"""
    while reads_below(encode(Maker(seed).short(body), None)):
        seed += 1000
    m = Maker(seed)
    seqs = m.short(body)
    match = None
    if last is not None:
        ll, ml, off = last
        if off > m.pos + ll:
            ll = off - m.pos + 5                    # enough literals for the offset to stay inside the block
        seqs.append(m.seq(ll, ml, off=off))
        match = (m.pos - ml, m.pos)
    fin = None if final is None else m.lits(final)
    n = m.pos + (final or 0)
    return Row(name, encode(seqs, fin), n, _caps(n, match), match, ends_on_match=final is None, **kw)


@functools.lru_cache(maxsize=None)
def table():
    """name -> Row, see the module docstring and each group's comment."""
    rows = []
    # literal pieces; long_literals' last piece overlaps its predecessor
    for k, name in ((9, "lit_short"), (300, "lit_300"), (5000, "lit_5000")):
        rows.append(_row(name, 600 + k % 97, 70, None, k))
    # 16-byte match pieces at the capacity; match_end: status 0 with out_len > cap, the reference's clip
    rows.append(_row("match_plain", 610, 70, (20, 200, 1000), 6))
    rows.append(_row("match_end", 611, 70, (20, 200, 1000), None))
    # periodic matches: the two-window pieces
    for per in (1, 3, 15, 17, 300):
        rows.append(_row(f"per_{per}", 620 + per % 89, 70, (2, 3000, per), None))
        rows.append(_row(f"per_{per}_fin", 640 + per % 89, 70, (2, 3000, per), 6))
    # one long run and nothing else (ratio >= 32: one wave decodes it): the absolute 16-byte grid and
    # its head piece at an odd out_off
    for per, final in ((1, None), (7, 6), (251, None)):
        m = Maker(660 + per)
        m.pos = 0
        ll = 20 if per <= 20 else per + 5
        seqs = [m.seq(ll, 60000, off=per)]
        fin = None if final is None else m.lits(final)
        n = m.pos + (final or 0)
        match = (m.pos - 60000, m.pos)
        rows.append(Row(f"per_long_{per}", encode(seqs, fin), n, _caps(n, match), match, ends_on_match=final is None))
    # the rewrite of the reference's tail copy (reference modes) in the second row of the sequence
    # table, and as the sequence a chunk is cut at
    m = Maker(670)
    seqs = m.short(80) + [m.seq(1, 4, off=24)] + m.short(10)
    rows.append(Row("f1_mid", encode(seqs, m.lits(9)), m.pos + 9, _caps(m.pos + 9)))
    m = Maker(671)
    seqs = m.short(64) + [m.seq(1400, 4, off=24)]
    match = (m.pos - 4, m.pos)
    seqs += m.short(70)
    rows.append(Row("f1_cut", encode(seqs, m.lits(6)), m.pos + 6, _caps(m.pos + 6) + [match[0] + 1, match[1] - 1]))
    # failing blocks
    cases = build_cases()
    for name in ("offset0_at_64", "malformed_and_offset0", "far_at_64"):
        comp, cap, _ = cases[name]
        rows.append(Row("err_" + name, comp, None, [cap]))
    # stored blocks of a frame (LZ4MI_FRAME_WORDS): the stored copy's tail; one that does not fit
    rng = np.random.default_rng(680)
    for n in (0, 1, 15, 16, 17, 4099):
        rows.append(Row(f"stored_{n}", rng.integers(0, 256, n, dtype=np.uint8), n, [n, n + 3] if n else [0], stored=True))
    rows.append(Row("stored_over", rng.integers(0, 256, 100, dtype=np.uint8), 100, [99], stored=True))
    # lone blocks only: a reference below the block's start
    m = Maker(690)
    seqs = [m.seq(3, 150, off=103)] + m.short(70)          # starts 100 bytes below out[0]: in the dictionary
    d = Maker(691).lits(400)
    rows.append(Row("dict_spill", encode(seqs, m.lits(9)), m.pos + 9, _caps(m.pos + 9, (3, 153)),
                    dictionary=np.frombuffer(d, dtype=np.uint8), lone_only=True, first=0))
    m = Maker(692)
    seqs = [m.seq(1, 4, off=50)] + m.short(70)             # reference modes rewrite out[297 .. 300) too
    rows.append(Row("f1_first", encode(seqs, m.lits(9)), m.pos + 9, _caps(m.pos + 9), lone_only=True, first=300))
    m = Maker(694)
    seqs = [m.seq(10, 5, off=10)] + m.short(70)             # reference modes: out[7 .. 10) = out[-3 .. 0)
    rows.append(Row("f1_src_below", encode(seqs, m.lits(9)), m.pos + 9, _caps(m.pos + 9), lone_only=True))
    m = Maker(693)
    seqs = m.short(10)
    seqs += [m.seq(1, 40, off=m.pos + 1 + 200)] + m.short(50)   # 200 bytes below the block's start
    rows.append(Row("hist", encode(seqs, m.lits(9)), m.pos + 9, _caps(m.pos + 9), lone_only=True))
    return {r.name: r for r in rows}


def pairs(stored=True, lone=False):
    """Every (row, capacity) of the table; roomy slots (N + 1, N + 16, N + 5000) of three of them."""
    out = []
    for r in table().values():
        if (r.stored and not stored) or (r.lone_only and not lone):
            continue
        out += [(r, c) for c in r.caps]
    t = table()
    out += [(t["lit_short"], t["lit_short"].n + 1), (t["match_end"], t["match_end"].n + 16),
            (t["per_3_fin"], t["per_3_fin"].n + 5000), (t["per_long_1"], t["per_long_1"].n + 5000)]
    return out


# ------------------------------------------------------------------------------------------ a call
class Batch:
    """One decode call: the blocks' payloads, their slots (offsets relative to out[0]) and the mode:
    spec, js_exact, js_compat, linked or linked_exact."""

    def __init__(self, name, pays, caps, offs=None, mode="spec", dictionary=None, stored=None, frame_words=False,
                 first=None, contiguous=()):
        self.name, self.mode, self.dictionary, self.frame_words = name, mode, dictionary, frame_words
        self.pays = [np.ascontiguousarray(p, dtype=np.uint8) for p in pays]
        self.caps = [int(c) for c in caps]
        self.offs = layout(self.caps, first=first, contiguous=contiguous) if offs is None else [int(o) for o in offs]
        self.stored = [False] * len(pays) if stored is None else [bool(s) for s in stored]
        assert frame_words or not any(self.stored)
        self.n = len(pays)
        self.span = self.offs[-1] + self.caps[-1]
        self.in_offs = layout([p.size for p in self.pays], guard=33, page=-1)
        self.in_span = self.in_offs[-1] + self.pays[-1].size

    @classmethod
    def of_pairs(cls, name, prs, mode, **kw):
        return cls(name, [r.comp for r, _ in prs], [c for _, c in prs], mode=mode, stored=[r.stored for r, _ in prs],
                   frame_words=any(r.stored for r, _ in prs), **kw)

    def out_arena(self, run):
        return pattern(2 * MARGIN + self.span, run)

    def in_arena(self, run):
        a = np.full(2 * MARGIN + self.in_span + 1, 0x00 if run == 0 else 0xFF, dtype=np.uint8)
        for off, p in zip(self.in_offs, self.pays):
            a[MARGIN + off:MARGIN + off + p.size] = p
            if run:
                a[MARGIN + off + p.size] = 0x1F
        return a

    def words(self):
        return np.array([p.size | (0x80000000 if s else 0) for p, s in zip(self.pays, self.stored)], dtype=np.uint32)


def _batched_status(comp, cap, js, out_off):
    """A block of an independent batch whose first failing check is a reference below its own start
    (the oracle's DICT_OOB when the block is decoded at position 0 without a dictionary):
    ERR_CROSS_BLOCK where the reference lands in `out`, the reference's DICT_OOB below out[0]."""
    st, _, _ = O.decompress_block(comp, cap, js_compat=js)
    if st == DICT_OOB:
        pos, off = first_far_reference(comp)
        return CROSS if off <= out_off + pos else DICT_OOB
    return None


def expected_image(init, blocks, slots, mode, dictionary=None, stored=None):
    """The arena the reference leaves, from the oracle only -> (image, care, status, out_len).
    init: the arena before the call; blocks: the payloads; slots: (offsets, capacities) relative
    to out[0] = init[MARGIN]. A failing block's own slot is don't-care (the GPU does not promise the
    reference's partial output there) and its out_len 0; everything else is compared."""
    offs, caps = slots
    n = len(blocks)
    stored = [False] * n if stored is None else stored
    js = mode in JS_MODES
    image = init.copy()
    care = np.ones(init.size, dtype=bool)
    view = image[MARGIN:]
    base = init[MARGIN:]
    status, lens = [], []
    if mode in LINKED_MODES:
        if mode == "linked_exact":
            st, ln, arr = in_order(blocks, offs, caps, base, dictionary, stored)
        else:
            st, ln, arr = _in_order_spec(blocks, offs, caps, base, dictionary, stored)
        view[:] = arr
        for b in range(n):
            if st[b] != 0:                            # the first failing block; the later ones stay init
                care[MARGIN + offs[b]:MARGIN + offs[b] + caps[b]] = False
                break
        return image, care, st, ln
    for b in range(n):
        off, cap, comp = offs[b], caps[b], blocks[b]
        sl = slice(MARGIN + off, MARGIN + off + cap)
        if stored[b]:
            if comp.size > cap:                       # the kernel returns before any store: the slot stays init
                status.append(RANGE)
                lens.append(0)
            else:
                image[MARGIN + off:MARGIN + off + comp.size] = comp
                status.append(OK)
                lens.append(int(comp.size))
            continue
        st, w, res = O.decompress_block(comp, cap, out=base[:off + cap].copy(), out_off=off, dictionary=dictionary,
                                        js_compat=js)
        if n > 1:
            cross = _batched_status(comp, cap, js, off)
            st = cross if cross is not None else st
            if js and st not in (0, CROSS) and reads_below(comp):
                # reference modes, batched: a rewrite that reads below the block is ERR_CROSS_BLOCK, reported
                # when its chunk is replayed -- before or after the block's other error
                st = (int(st), CROSS)
        status.append(st if isinstance(st, tuple) else int(st))
        if st != 0:
            lens.append(0)
            care[sl] = False
            continue
        lens.append(int(w))
        if n > 1:
            image[sl] = res[off:off + cap]
            assert np.array_equal(res[:off], base[:off]), "an independent block changed bytes below its slot"
        else:
            view[:off + cap] = res                    # a lone block: history below the slot included
    return image, care, status, lens


def _in_order_spec(pay, out_off, out_cap, init, dictionary, stored):
    """linked_exact_common.in_order with the spec decoder (LZ4MI_LINKED)."""
    out = np.array(init, dtype=np.uint8, copy=True)
    st, ln, failed = [], [], False
    for b in range(len(pay)):
        off, cap = int(out_off[b]), int(out_cap[b])
        if failed:
            st.append(CROSS)
            ln.append(0)
        elif stored[b]:
            if pay[b].size > cap:
                st.append(RANGE)
                ln.append(0)
                failed = True
            else:
                out[off:off + pay[b].size] = pay[b]
                st.append(OK)
                ln.append(int(pay[b].size))
        else:
            trial = out.copy()
            s, w, _ = O.decompress_block(pay[b], cap, out=trial[:off + cap], out_off=off, dictionary=dictionary)
            st.append(int(s))
            ln.append(int(w) if s == 0 else 0)
            if s == 0:
                out = trial
            else:
                failed = True
    return st, ln, out


def sequential_image(init, batch):
    """What one reference decoder call per block, in index order on the one array, leaves (partial
    output of failing blocks included): the host decoder's claim. -> (image, status, out_len)."""
    image = init.copy()
    view = image[MARGIN:]
    st, ln = [], []
    for comp, off, cap in zip(batch.pays, batch.offs, batch.caps):
        s, w, _ = O.decompress_block(comp, cap, out=view[:off + cap], out_off=off, dictionary=batch.dictionary,
                                     js_compat=batch.mode in JS_MODES)
        st.append(int(s))
        ln.append(int(w) if s == 0 else 0)
    return image, st, ln


def host_decode(lz4mi, batch, run):
    """The batch through the host decoder (lz4mi_host_decompress_block), one call per block on the
    caller's arena -> (out arena, in arena, status, out_len)."""
    out, inp = batch.out_arena(run), batch.in_arena(run)
    view = out[MARGIN:]
    st, ln = [], []
    for comp, ioff, off, cap in zip(batch.pays, batch.in_offs, batch.offs, batch.caps):
        try:
            # (the input array ends with the block: like lz4mi_decompress_blocks, bytes past it read as 0)
            w = lz4mi.host_decompress_raw(inp[:MARGIN + ioff + comp.size], MARGIN + ioff, comp.size, view[:off + cap], off,
                                          dictionary=batch.dictionary, spec=batch.mode not in JS_MODES)
            st.append(0)
            ln.append(w)
        except lz4mi.Lz4miError as e:
            st.append(e.status)
            ln.append(0)
    return out, inp, st, ln


def dev_decode(lz4mi, batch, run):
    """One lz4mi.decompress_blocks_dev call on torch tensors built from the arenas; out_ptr and
    in_ptr are the tensors' data_ptr() + MARGIN -> (out arena, in arena, status[n + 64], out_len[n + 64])."""
    import torch
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a).astype(dt)).cuda()
    d_out, d_in = t(batch.out_arena(run), np.uint8), t(batch.in_arena(run), np.uint8)
    d_ioff, d_ooff = t(batch.in_offs, np.int64), t(batch.offs, np.int64)
    d_ilen, d_cap = t(batch.words().view(np.int32), np.int32), t(batch.caps, np.int32)
    d_len = torch.full((batch.n + SENTINELS,), FILL, dtype=torch.int32, device="cuda")
    d_st = torch.full((batch.n + SENTINELS,), FILL, dtype=torch.int32, device="cuda")
    d_dict = None if batch.dictionary is None else t(batch.dictionary, np.uint8)
    mode = batch.mode
    lz4mi.decompress_blocks_dev(d_in.data_ptr() + MARGIN, d_ioff.data_ptr(), d_ilen.data_ptr(),
                                d_out.data_ptr() + MARGIN, d_ooff.data_ptr(), d_cap.data_ptr(), d_len.data_ptr(),
                                d_st.data_ptr(), batch.n, torch.cuda.current_stream().cuda_stream,
                                js_compat=mode == "js_compat", js_exact=mode == "js_exact",
                                dict_ptr=None if d_dict is None else d_dict.data_ptr(),
                                dict_len=0 if d_dict is None else d_dict.numel(), frame_words=batch.frame_words,
                                linked="exact" if mode == "linked_exact" else mode == "linked")
    torch.cuda.synchronize()
    return d_out.cpu().numpy(), d_in.cpu().numpy(), d_st.cpu().numpy(), d_len.cpu().numpy().view(np.uint32)


def check_batch(batch, decode, all_care=False):
    """Runs 0 and 1 of a batch through `decode(batch, run)`; the whole out arena against the oracle's
    image, the in arena unchanged, statuses and lengths against the oracle and equal in both runs,
    the sentinels untouched. -> the expected statuses."""
    seen = []
    for run in (0, 1):
        init = batch.out_arena(run)
        if all_care:
            image, st, ln = sequential_image(init, batch)
            care = np.ones(init.size, dtype=bool)
        else:
            image, care, st, ln = expected_image(init, batch.pays, (batch.offs, batch.caps), batch.mode,
                                                 batch.dictionary, batch.stored)
        got, got_in, gst, gln = decode(batch, run)
        what = f"{batch.name} [{batch.mode}] run {run}"
        gs, gl = [int(x) for x in gst[:batch.n]], [int(x) for x in gln[:batch.n]]
        assert all(_is(g, w) for g, w in zip(gs, st)), (what, "status", _first_diff(gs, st))
        assert gl == [int(x) for x in ln], (what, "out_len", _first_diff(gl, ln))
        assert_sentinels(gst, batch.n, what + " status[]")
        assert_sentinels(gln, batch.n, what + " out_len[]")
        assert_footprint(got, image, care, Regions(batch.offs, batch.caps, ln), what)
        assert np.array_equal(got_in, batch.in_arena(run)), (what, "the input arena changed")
        seen.append((gs, gl, got, image, care))
    a, b = seen
    assert a[0] == b[0] and a[1] == b[1], (batch.name, "statuses or lengths depend on the surrounding bytes")
    same = (a[3] == b[3]) & a[4]                      # bytes the expected image does not take from the pre-fill
    assert np.array_equal(a[2][same], b[2][same]), (batch.name, "decoded bytes depend on the surrounding bytes")
    return a[0]


def _is(got, want):
    return got in want if isinstance(want, tuple) else int(got) == int(want)


def _first_diff(got, want):
    for k, (g, w) in enumerate(zip(got, want)):
        if not _is(g, w):
            return f"block {k}: got {int(g)}, expected {w}"
    return "lengths differ"


# ------------------------------------------------------------------------------------- the routes
def dont_care_fraction(batch):
    _, care, _, _ = expected_image(batch.out_arena(0), batch.pays, (batch.offs, batch.caps), batch.mode,
                                   batch.dictionary, batch.stored)
    return float((~care).sum()) / max(1, sum(batch.caps))


def _fails(row, cap, mode):
    """Whether (row, cap) fails in an independent batch."""
    if row.stored:
        return row.comp.size > cap
    js = mode in JS_MODES
    return O.decompress_block(row.comp, cap, js_compat=js)[0] != 0


def grouped(prs, size, mode, name, fill=True):
    """The pairs in batches of at most `size` blocks. Failing blocks sit at positions 1, 4, 7, ...:
    never adjacent, at most a third of a batch. A batch with a failing block ends on a roomy block
    whose slot is long enough for the don't-care bytes to be at most a quarter of the slot bytes;
    with `fill` every batch is filled up to `size` with roomy blocks."""
    t = table()
    roomy = (t["lit_short"], t["lit_short"].n + 16)
    bad = [p for p in prs if _fails(p[0], p[1], mode)]
    good = [p for p in prs if not _fails(p[0], p[1], mode)]
    out = []
    while bad or good:
        nb = min(len(bad), size // 3)
        ng = size - nb - (1 if nb else 0)
        if not fill:
            ng = min(ng, max(len(good), 2 * nb))
        cur, b, g = [], [bad.pop(0) for _ in range(nb)], [good.pop(0) if good else roomy for _ in range(ng)]
        while b or g:
            cur.append(b.pop(0) if b and (len(cur) % 3 == 1 or not g) else g.pop(0))
        if nb:
            dc = sum(c for r, c in cur if _fails(r, c, mode))
            cur.append((roomy[0], roomy[1] + max(0, 4 * dc - sum(c for _, c in cur) - roomy[1])))
        out.append(Batch.of_pairs(f"{name}{len(out)}", cur, mode))
    return out


@functools.lru_cache(maxsize=None)
def batches(size, mode, fill=True):
    stored = mode != "js_compat"
    return tuple(grouped(pairs(stored=stored), size, mode, f"batch{size}_", fill))


@functools.lru_cache(maxsize=None)
def lone_batches(mode):
    """Every pair of the table (the lone-only rows included) alone in a call, at out_off 0, 3 and
    300 in turn: the bytes below the slot are history, with a 400-byte dictionary below out[0]
    for every other block."""
    d = table()["dict_spill"].dictionary
    out = []
    prs = [p for p in pairs(stored=mode != "js_compat", lone=True)]
    k = 0
    for r, cap in prs:
        both = r.name in ("hist", "f1_src_below")
        firsts = (0, 3, 300) if both else ((r.first,) if r.first is not None else ((0, 3, 300)[k % 3],))
        for first in firsts:
            for dictionary in ((None, d) if both else (r.dictionary if r.dictionary is not None else
                                                                   (d if k % 2 else None),)):
                out.append(Batch(f"lone_{r.name}_cap{cap}_at{first}" + ("_dict" if dictionary is not None else ""),
                                 [r.comp], [cap], mode=mode, dictionary=dictionary, stored=[r.stored],
                                 frame_words=r.stored, first=first))
        k += 1
    return tuple(out)


@functools.lru_cache(maxsize=None)
def linked_cases():
    """Five dependent 64 KiB blocks (the frame encoder's, block_independence=False) in slots with
    guards between them -- except in front of block 3, whose reference-mode rewrite reaches into
    block 2's tail --, block 0 in a slot 100 bytes too long, block 1 stored. `ok`: every capacity
    fits; `fail`: block 2 one byte short, so blocks 3 and 4 are not written."""
    from lz4mi import shard
    bs = 65536
    data = O.generate("copy", 5, 5 * bs)
    frame = O.compress_frame(data, None, bs, False, False, True)
    _, blocks = shard.frame_blocks(frame)
    pay = [frame[p:p + n].copy() for p, n, _ in blocks]
    assert len(pay) == 5 and not any(s for _, _, s in blocks)
    pay[1] = data[bs:2 * bs].copy()
    stored = [False, True, False, False, False]
    out = {}
    for name, caps in (("ok", [bs + 100, bs, bs, bs, bs]), ("fail", [bs + 100, bs, bs - 1, bs, bs])):
        out[name] = {"pay": pay, "caps": caps, "stored": stored, "offs": layout(caps, first=3, contiguous=(3,))}
    return out


def linked_batch(which, mode):
    c = linked_cases()[which]
    return Batch(f"linked_{which}", c["pay"], c["caps"], offs=c["offs"], mode=mode, stored=c["stored"], frame_words=True)


# ------------------------------------------------------------------------------------- the encoder
ENC_SIZES = (0, 1, 12, 13, 15, 16, 17, 2031, 2032, 2033, 2047, 2048, 2049, 65536)


@functools.lru_cache(maxsize=None)
def encoder_inputs():
    """Random inputs around the encoder's ring limit and direct literal copy, and compressible
    text / tiles216 blocks of 5 000 and 100 003 bytes: 20 blocks."""
    rng = np.random.default_rng(700)
    srcs = [rng.integers(0, 256, n, dtype=np.uint8) for n in ENC_SIZES]
    srcs += [O.generate(kind, 71 + n % 7, n) for kind in ("text", "tiles216") for n in (5000, 100003)]
    srcs += [O.generate("text", 75, 2040), O.generate("tiles216", 76, 777)]
    assert len(srcs) == 20
    return tuple(srcs)


class EncBatch:
    """One compress call: inputs at odd offsets of an in arena, output slots exactly
    compress_bound(n) long with a 1 KiB guard between them, at odd offsets."""

    def __init__(self, name, srcs):
        self.name, self.srcs, self.n = name, [np.ascontiguousarray(s, dtype=np.uint8) for s in srcs], len(srcs)
        self.bounds = [O.compress_bound(s.size) for s in self.srcs]
        self.offs = layout(self.bounds)
        self.span = self.offs[-1] + self.bounds[-1]
        self.in_offs = layout([s.size for s in self.srcs], guard=33, page=-1)
        self.in_span = self.in_offs[-1] + self.srcs[-1].size

    def out_arena(self, run):
        return pattern(2 * MARGIN + self.span, run)

    def in_arena(self, run):
        a = np.full(2 * MARGIN + self.in_span + 1, 0x00 if run == 0 else 0xFF, dtype=np.uint8)
        for off, s in zip(self.in_offs, self.srcs):
            a[MARGIN + off:MARGIN + off + s.size] = s
        return a

    def expected(self, run):
        """-> (image, lengths): init with [off, off + len) replaced by the oracle encoder's bytes."""
        image = self.out_arena(run)
        lens = []
        for off, s in zip(self.offs, self.srcs):
            c = _compressed(s.tobytes())
            image[MARGIN + off:MARGIN + off + c.size] = c
            lens.append(int(c.size))
        return image, lens


@functools.lru_cache(maxsize=None)
def _compressed(b):
    return O.compress_block_bytes(np.frombuffer(b, dtype=np.uint8))


def encoder_batch(nblocks):
    """20 blocks, or those padded with tiny blocks (0 to 18 bytes) to `nblocks`."""
    srcs = list(encoder_inputs())
    rng = np.random.default_rng(701)
    while len(srcs) < nblocks:
        srcs.append(rng.integers(0, 256, len(srcs) % 19, dtype=np.uint8))
    return EncBatch(f"enc{nblocks}", srcs)
