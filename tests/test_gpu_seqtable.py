"""The decoder's sequence table (csrc/lz4mi_decompress.hip, step 4): built sequence-major, lane l
of row i takes sequence 64 i + l of the 1 KiB chunk. Hand-assembled raw blocks put the row
boundaries, the slow length-field paths and every error check at chosen sequence numbers of the
first chunk; bytes, status and out_len are checked against the CPU oracle in spec and js_exact
mode, through the small-batch path (1 and 3 blocks) and the batch kernel (SMALL_BLOCKS + 8 copies).

Sequence layout per the LZ4 block format (the reference's decoder, src/block/blockDecompress.js:30,
reads the same fields and makes the checks in this order: output too small, malformed input,
offset 0, dictionary offset out of bounds).
"""
import functools

import numpy as np
import pytest

import oracle as O

CHUNK = 1024          # compressed bytes the decoder parses per step
OK, TOO_SMALL, MALFORMED, OFFSET0, DICT_OOB, CROSS = 0, -1, -2, -3, -4, -9


def _varint(n):
    out = []
    while n >= 255:
        out.append(255)
        n -= 255
    out.append(n)
    return out


def encode(seqs, final_lits, truncate=None):
    """seqs: [(literal bytes, offset, match length)] (any offset, 0 included), then the
    literal-only tail; truncate: keep only that many bytes."""
    out = []
    for lits, off, ml in seqs:
        ll = len(lits)
        out.append((min(ll, 15) << 4) | min(ml - 4, 15))
        if ll >= 15:
            out += _varint(ll - 15)
        out += list(lits)
        out += [off & 255, off >> 8]
        if ml - 4 >= 15:
            out += _varint(ml - 4 - 15)
    if final_lits is not None:
        ll = len(final_lits)
        out.append(min(ll, 15) << 4)
        if ll >= 15:
            out += _varint(ll - 15)
        out += list(final_lits)
    a = np.array(out, dtype=np.uint8)
    return a if truncate is None else a[:truncate].copy()


def first_far_reference(comp):
    """(output position of the match, offset) of the first sequence whose offset reaches before
    the block's own output; for blocks the oracle rejects with DICT_OOB when decoded alone."""
    data = [int(x) for x in comp]

    class Padded:               # (bytes past the block's end read as 0)
        def __len__(self):
            return len(data)

        def __getitem__(self, i):
            return data[i] if i < len(data) else 0
    c = Padded()
    ip, pos = 0, 0
    while ip < len(c):
        tok = c[ip]
        ip += 1
        ll = tok >> 4
        if ll == 15:
            while True:
                b = c[ip]
                ip += 1
                ll += b
                if b != 255:
                    break
        ip += ll
        pos += ll
        if ip >= len(c):
            break
        off = c[ip] | (c[ip + 1] << 8)
        ip += 2
        ml = tok & 15
        if ml == 15:
            while True:
                b = c[ip]
                ip += 1
                ml += b
                if b != 255:
                    break
        if off > pos:
            return pos, off
        pos += ml + 4
    raise AssertionError("no far reference")


class Maker:
    """base: the block's position in its frame (tests/chain_blocks_common.py): an explicit offset may
    reach below the block, and a drawn one is drawn a second time, from a generator of its own, over
    the history from the frame's start -- the first draw keeps the stream of lengths and literals,
    so the block's shape, that of base 0."""

    def __init__(self, seed, base=0):
        self.rng = np.random.default_rng(seed)
        self.pos = 0
        self.base = base
        self.far = np.random.default_rng([seed, base])

    def lits(self, n):
        return bytes(self.rng.integers(0, 256, n, dtype=np.uint8))

    def seq(self, ll, ml, off=None):
        """One sequence of ll literals and a match of ml bytes at a valid offset (or `off`)."""
        self.pos += ll
        if off is None:
            assert self.pos or self.base, "a match at the first byte of the first block"
            if self.pos:
                off = int(self.rng.integers(1, min(self.pos, 65535) + 1))
            if self.base:
                off = int(self.far.integers(1, min(self.base + self.pos, 65535) + 1))
        self.pos += ml
        return (self.lits(ll), off, ml)

    def short(self, n, ml=None):
        """n four-byte sequences: token, one literal, offset."""
        return [self.seq(1, int(self.rng.integers(4, 19)) if ml is None else ml) for _ in range(n)]


def case_dense(base=0):
    """Three-byte sequences (no literals, match length 4-18): 5-6 tokens per 16-byte segment and
    the most tokens a chunk can hold, over six rows."""
    m = Maker(1, base)
    seqs = [m.seq(1, 8)] + [m.seq(0, int(m.rng.integers(4, 19))) for _ in range(700)]
    return seqs, m.lits(9)


def cases_rows(base=0):
    """First chunks of exactly n sequences: n - 1 four-byte ones and a literal run that carries the
    parse past the chunk's end (inside the window: the block is short enough for the exact
    next-token table); n four-byte ones and a run too long for the window (the cut sequence); and
    blocks whose final literal-only sequence is number 0, 63 or 64."""
    out = {}
    for n in (1, 63, 64, 65, 127, 128, 129):
        m = Maker(100 + n, base)
        seqs = m.short(n - 1)
        seqs.append(m.seq(CHUNK + 8 - 4 * n, 7))
        out[f"rows_{n}_run"] = (seqs + m.short(5), m.lits(6))
        m = Maker(200 + n, base)
        seqs = m.short(n)
        seqs.append(m.seq(1400, 9))
        out[f"rows_{n}_cut"] = (seqs + m.short(70), m.lits(6))
    for n in (0, 63, 64):
        m = Maker(300 + n, base)
        out[f"final_at_{n}"] = (m.short(n), m.lits(11))
    return out


def cases_slow(base=0):
    """Length fields of several bytes among >= 65 other sequences, in row 0 and in row 1: a literal
    length of 2 and of 3 extension bytes, a match length of 2+ bytes (the fast next-token table
    assumes one: the chunk is parsed again)."""
    out = {}
    for row, at in ((0, 10), (1, 80)):
        for name, ll, ml in (("ll2", 300, 6), ("ll3", 600, 6), ("ml2", 2, 4 + 15 + 255 + 40), ("ml3", 1, 4 + 15 + 600)):
            m = Maker(400 + 10 * row + ll % 7 + ml % 5, base)
            seqs = m.short(at) + [m.seq(ll, ml)] + m.short(90) + [m.seq(1500, 5)] + m.short(70)
            out[f"{name}_row{row}"] = (seqs, m.lits(5))
            m = Maker(450 + 10 * row + ll % 7 + ml % 5, base)       # a short block: the exact table from the start
            out[f"{name}_row{row}_short"] = (m.short(at) + [m.seq(ll, ml)] + m.short(70), m.lits(5))
    return out


def cases_redo(base=0):
    """The fast next-token table sent back for the exact one: a match length field of 2 bytes and
    one of 3 bytes among the true tokens of one chunk, far enough from the block's end for the
    fast table. redo_2k: in the first chunk of a block of about 2 KiB (one segment). redo_seg1:
    past 5120 compressed bytes in a block of two segments, so that segment 1's parse -- the guess
    and, forced, the re-parse from segment 0's exit -- meets them too."""
    long2, long3 = 4 + 15 + 255 + 40, 4 + 15 + 600
    m = Maker(600, base)
    a = m.short(10) + [m.seq(2, long2)] + m.short(20) + [m.seq(1, long3)] + m.short(470)
    fa = m.lits(5)
    m = Maker(601, base)
    b = m.short(1300) + [m.seq(2, long2)] + m.short(20) + [m.seq(1, long3)] + m.short(1000)
    return {"redo_2k": (a, fa), "redo_seg1": (b, m.lits(5))}


@functools.lru_cache(maxsize=None)
def redo_cases():
    done = {}
    for name, (s, f) in cases_redo().items():
        comp = encode(s, f)
        st, cap, _ = O.decompress_block(comp, 1 << 16)
        assert st == 0 and cap <= (1 << 16), name
        done[name] = (comp, cap, {js: O.decompress_block(comp, cap, js_compat=js) for js in (False, True)})
    return done


def build_cases(base=0):
    """name -> (compressed block, capacity, dictionary or None)."""
    cases = {}
    s, f = case_dense(base)
    cases["dense3"] = (encode(s, f), None, None)
    for group in (cases_rows(base), cases_slow(base)):
        for name, (s, f) in group.items():
            cases[name] = (encode(s, f), None, None)

    def hundred(seed, edits):
        m = Maker(seed, base)
        seqs = m.short(100)
        for k, fn in edits.items():
            lits, off, ml = seqs[k]
            seqs[k] = (lits, fn(off), ml)
        return encode(seqs, m.lits(7)), m.pos + 7

    for k in (0, 63, 64, 70):
        cases[f"offset0_at_{k}"] = (hundred(500 + k, {k: lambda o: 0})[0], 2000, None)
    cases["offset0_then_far"] = (hundred(510, {20: lambda o: 0, 70: lambda o: 60000})[0], 2000, None)
    cases["far_then_offset0"] = (hundred(511, {20: lambda o: 60000, 70: lambda o: 0})[0], 2000, None)
    cases["far_at_64"] = (hundred(512, {64: lambda o: 40000})[0], 2000, None)
    c, n = hundred(513, {})
    cases["cap_exact"] = (c, n, None)
    cases["cap_one_short"] = (c, n - 1, None)
    m = Maker(514, base)
    seqs = m.short(66) + [m.seq(12, 6)]
    full = encode(seqs, None)
    cases["malformed_and_offset0"] = (full[:full.size - 2 - 5].copy(), 2000, None)   # 5 of its 12 literals missing
    m = Maker(515, base)
    seqs = m.short(10)
    seqs += [m.seq(1, 8, off=m.pos + 1 + 300)] + m.short(53)                            # 300 bytes before the block
    d = m.lits(400)
    cases["dict_inside"] = (encode(seqs, m.lits(3)), 2000, d)
    cases["dict_outside"] = (encode(seqs, m.lits(3)), 2000, d[:200])
    return cases


def fuzz_blocks(base=0):
    """200 seeded random token streams (<= 8 KiB each): short and long literal runs and matches,
    some with an offset of 0, a far offset, a truncated end or a capacity a few bytes off."""
    rng = np.random.default_rng(20240607)
    out = []
    for t in range(200):
        m = Maker(1000 + t, base)
        seqs, size = [], 0
        limit = int(rng.integers(40, 7000))
        while size < limit:
            r = rng.random()
            ll = int(rng.integers(0, 4)) if r < 0.7 else int(rng.integers(4, 40)) if r < 0.95 else int(rng.integers(200, 900))
            r = rng.random()
            ml = int(rng.integers(4, 19)) if r < 0.8 else int(rng.integers(19, 300)) if r < 0.97 else int(rng.integers(300, 3000))
            if not seqs and ll == 0:
                ll = 1
            seqs.append(m.seq(ll, ml))
            size += 3 + ll + (1 if ll >= 15 else 0) + (1 if ml >= 19 else 0)
        fin = m.lits(int(rng.integers(0, 20)))
        cap = m.pos + len(fin)
        kind = int(rng.integers(0, 8))
        trunc = None
        if kind == 1:
            k = int(rng.integers(0, len(seqs)))
            seqs[k] = (seqs[k][0], 0, seqs[k][2])
        elif kind == 2:
            k = int(rng.integers(0, len(seqs)))
            seqs[k] = (seqs[k][0], int(rng.integers(30000, 65536)), seqs[k][2])
        elif kind == 3:
            cap += int(rng.integers(-3, 3))
        elif kind == 4:
            trunc = int(rng.integers(1, encode(seqs, fin).size))
        out.append((encode(seqs, fin, trunc), cap, None))
    return out


@functools.lru_cache(maxsize=None)
def all_cases():
    cases = build_cases()
    for i, c in enumerate(fuzz_blocks()):
        cases[f"fuzz{i}"] = c
    done = {}
    for name, (comp, cap, d) in cases.items():
        if cap is None:
            st, n, _ = O.decompress_block(comp, 1 << 16)
            assert st == 0 and n <= (1 << 16), name
            cap = n
        ref = {js: O.decompress_block(comp, cap, dictionary=d, js_compat=js) for js in (False, True)}
        done[name] = (comp, cap, d, ref)
    return done


def test_cases_are_what_they_claim():
    """CPU: the oracle's verdict on the hand-assembled blocks."""
    cs = all_cases()
    want = {"offset0_at_0": OFFSET0, "offset0_at_63": OFFSET0, "offset0_at_64": OFFSET0, "offset0_at_70": OFFSET0,
            "offset0_then_far": OFFSET0, "far_then_offset0": DICT_OOB, "far_at_64": DICT_OOB, "cap_exact": OK,
            "cap_one_short": TOO_SMALL, "malformed_and_offset0": MALFORMED, "dict_inside": OK, "dict_outside": DICT_OOB}
    for name, st in want.items():
        assert cs[name][3][False][0] == st and cs[name][3][True][0] == st, name
    for name, (comp, cap, d, ref) in cs.items():
        if not name.startswith("fuzz") and name not in want:
            assert ref[False][0] == 0 and ref[True][0] == 0 and cap <= (1 << 16), name
    assert cs["dense3"][0].size > 2 * CHUNK and cs["rows_129_cut"][0].size > CHUNK
    seen = {cs[f"fuzz{i}"][3][False][0] for i in range(200)}
    assert {OK, TOO_SMALL, MALFORMED, OFFSET0, DICT_OOB} <= seen
    assert max(cs[f"fuzz{i}"][0].size for i in range(200)) <= 8192


def test_redo_cases_are_what_they_claim():
    """CPU: the long match length fields lie where the fast table is in use (more than
    kFastRem = 1024 + 64 + 300 bytes before the block's end), in the first chunk of a one-segment
    block and in segment 1 (from 5120) of a two-segment one (csrc/lz4mi_decompress.h, seg_geom)."""
    cs = redo_cases()
    comp = cs["redo_2k"][0]
    two, three = 4 * 10, 4 * 10 + 3 + 2 + 2 + 4 * 20      # tokens of the two long matches
    assert 2 * CHUNK - 100 <= comp.size <= 8192 and three < CHUNK
    assert comp[two] & 15 == 15 and list(comp[two + 5:two + 7]) == [255, 40]
    assert comp[three] & 15 == 15 and list(comp[three + 4:three + 7]) == [255, 255, 90]
    comp = cs["redo_seg1"][0]
    two = 4 * 1300
    three = two + 3 + 2 + 2 + 4 * 20
    assert 8192 < comp.size <= 16384 and two >= 5120 and comp.size - three > 2 * CHUNK
    assert comp[two] & 15 == 15 and list(comp[two + 5:two + 7]) == [255, 40]
    assert comp[three] & 15 == 15 and list(comp[three + 4:three + 7]) == [255, 255, 90]
    for name, (comp, cap, ref) in cs.items():
        assert ref[False][0] == 0 and ref[True][0] == 0, name


def _check(lz4mi, name, comp, cap, ref, js, st, out, n, batched_at=None):
    """One decoded block against the oracle; batched_at: the block's output offset in a batch of
    independent blocks, where a reference before the block's start is CROSS_BLOCK."""
    est, ew, eo = ref[js]
    if batched_at is not None and est == DICT_OOB:
        pos, off = first_far_reference(comp)
        if off <= batched_at + pos:
            est = CROSS
    if batched_at is not None and js and st == CROSS and est != CROSS:
        # reference mode, batched: a tail rewrite of an earlier chunk reaches before the
        # block, which the kernel reports when it replays that chunk -- before a later chunk's error
        assert n == 0, (name, js, batched_at)
        return
    assert st == est, (name, js, batched_at, int(st), est)
    if est == 0:
        assert n == ew and np.array_equal(out, eo[:ew]), (name, js, batched_at)
    else:
        assert n == 0, (name, js, batched_at)


@pytest.mark.gpu
@pytest.mark.parametrize("js", [False, True], ids=["spec", "js_exact"])
def test_small_batch_path(js):
    lz4mi = pytest.importorskip("lz4mi")
    lz4mi.init(0)
    for name, (comp, cap, d, ref) in all_cases().items():
        st, outs, lens = lz4mi.decompress_blocks([comp], [cap], dictionary=d, js_exact=js)
        _check(lz4mi, name, comp, cap, ref, js, st[0], outs[0], lens[0])
        if d is not None or name.startswith("fuzz"):
            continue
        st, outs, lens = lz4mi.decompress_blocks([comp] * 3, [cap] * 3, js_exact=js)
        for j in range(3):
            _check(lz4mi, name, comp, cap, ref, js, st[j], outs[j], lens[j], batched_at=j * cap)


@pytest.mark.gpu
@pytest.mark.parametrize("js", [False, True], ids=["spec", "js_exact"])
@pytest.mark.parametrize("path", ["batch", "small_reparse"])
def test_fast_table_redo(path, js, monkeypatch):
    """A true token's match length field of 2 and of 3 bytes where the fast next-token table is in
    use: the chunk is parsed again with the exact table (decompress_block's loop around
    parse_chunk and seq_table). Both instantiations that take that path: the batch kernel
    (SMALL_BLOCKS + 8 copies) and the small path's export kernel, one block, with the test hook
    LZ4MI_SMALL_REPARSE=2 (every guess past segment 0 counts as wrong, so redo_seg1's segment 1 is
    parsed again from segment 0's exit)."""
    lz4mi = pytest.importorskip("lz4mi")
    lz4mi.init(0)
    if path == "small_reparse":
        monkeypatch.setenv("LZ4MI_SMALL_REPARSE", "2")
    copies = lz4mi.SMALL_BLOCKS + 8 if path == "batch" else 1
    for name, (comp, cap, ref) in redo_cases().items():
        st, outs, lens = lz4mi.decompress_blocks([comp] * copies, [cap] * copies, js_exact=js)
        for j in range(copies):
            _check(lz4mi, name, comp, cap, ref, js, st[j], outs[j], lens[j],
                   batched_at=j * cap if copies > 1 else None)


@pytest.mark.gpu
@pytest.mark.parametrize("js", [False, True], ids=["spec", "js_exact"])
def test_batch_kernel(js):
    lz4mi = pytest.importorskip("lz4mi")
    lz4mi.init(0)
    copies = lz4mi.SMALL_BLOCKS + 8
    cs = all_cases()
    for name, (comp, cap, d, ref) in cs.items():
        if d is not None or name.startswith("fuzz"):
            continue
        st, outs, lens = lz4mi.decompress_blocks([comp] * copies, [cap] * copies, js_exact=js)
        for j in range(copies):
            _check(lz4mi, name, comp, cap, ref, js, st[j], outs[j], lens[j], batched_at=j * cap)
    fz = [cs[f"fuzz{i}"] for i in range(200)]     # the fuzz streams: one batch of all of them
    assert len(fz) >= copies
    st, outs, lens = lz4mi.decompress_blocks([c[0] for c in fz], [c[1] for c in fz], js_exact=js)
    at = 0
    for j, (comp, cap, d, ref) in enumerate(fz):
        _check(lz4mi, f"fuzz{j}", comp, cap, ref, js, st[j], outs[j], lens[j], batched_at=at)
        at += cap
