"""Raw blocks far above 4 MiB through the decoder, the size pass and the encoder (tests/big_blocks_common.py).

include/lz4mi.h promises raw calls blocks up to LZ4MI_MAX_BLOCK = 2^31 - 1 bytes. The decoder cases put a 1 to 2 MiB
body of tiles216 / text / copy behind a periodic prefix so that it lies across the block-relative positions 2^27,
2^29 - 64 KiB, 2^29 + 2^27 and 2^30, wholly inside [2^29, 2^29 + 2^27), and against the top edge (the body ends on
the last byte the ABI allows), and decode them through lz4mi_decompress_blocks on device pointers, in spec mode and
LZ4MI_JS_EXACT, on three routes: a lone block (nblocks == 1, at out_off 0 and at an odd out_off), a small batch
(the blocks are past the export limits, so the small-path launch decodes each with one wave) and the batch kernel
(lz4mi.SMALL_BLOCKS + 1 blocks, all but two of them 13-byte fillers). Everywhere status 0, out_len n, the whole slot
equal to the image the construction names (built on the device: a tiled prefix plus the uploaded tail), and the bytes
around every slot -- 4 KiB below, 64 KiB behind, inside the same allocation -- and the sentinel entries of status[]
and out_len[] untouched. In a reference-mode batch no block may answer ERR_CROSS_BLOCK: every block starts with 64
or more literals, so no tail rewrite reaches below it.

Left out: LZ4MI_JS_COMPAT (one lane per block, far too slow at these sizes; its arithmetic is int64 throughout) and
LZ4MI_LINKED / LZ4MI_LINKED_EXACT (capped at 4 MiB by contract; tests/test_gpu_linked.py::test_refusals pins ERR_ARG
for a host-pointer call with a 4 MiB + 1 capacity).

The encoder side: blocks of 4 MiB + 1, 8 MiB + 12345 and 40 MiB in one batch, a chain of (8 MiB + 4)-byte blocks
with a carried table, and a lone 9 MiB block with a caller table, equal to the oracle's bytes and tables."""
import time

import numpy as np
import pytest

import big_blocks_common as B
import footprint_common as F
import oracle as O

lz4mi = pytest.importorskip("lz4mi")
torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

SENT, FILL = F.SENTINELS, F.FILL
BELOW, BEHIND = 4096, 65536
SLOT_FILL = 0xA5
CROSS = lz4mi.ERR_CROSS_BLOCK
MODES = ("spec", "js_exact")
ROUTES = ("lone", "small", "batch")
NBATCH = lz4mi.SMALL_BLOCKS + 1
PIECE = 16 << 20


@pytest.fixture(scope="module", autouse=True)
def _device():
    lz4mi.init(0)
    yield
    _drop()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _t(a, dt):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a).astype(dt))).cuda()


def _pattern(n, at):
    return ((131 * (np.arange(n, dtype=np.int64) + at) + 7) & 255).astype(np.uint8)


class Arena:
    """One device allocation holding every output slot of a case: BELOW bytes of pattern below each slot, BEHIND bytes
    behind it, slots at odd positions (1, 5, 15 mod 16 in turn), then the slots of the batch route's fillers. The
    expected image of each block in both modes lies in a second allocation per block."""

    def __init__(self, blocks):
        self.blocks = blocks
        self.pos, at = [], 0
        for k, b in enumerate(blocks):
            p = at + BELOW
            p += (F.RESIDUES[k % 3] - p) % 16
            self.pos.append(p)
            at = p + b.n + BEHIND
        self.fill_pos = [at + BELOW + 48 * j + 1 for j in range(NBATCH)]       # 13-byte slots, 35 bytes apart
        self.size = self.fill_pos[-1] + B.FILLER_N + BELOW
        self.t = torch.empty(self.size, dtype=torch.uint8, device="cuda")
        # the gaps: everything outside the big slots (the fillers' region included, reset before each call)
        self.gaps, lo = [], 0
        for p, b in zip(self.pos, blocks):
            self.gaps.append((lo, p - lo))
            lo = p + b.n
        self.gaps.append((lo, self.size - lo))
        self.gap_img = [_t(_pattern(n, a), np.uint8) for a, n in self.gaps]
        self.want = {}
        for k, b in enumerate(blocks):
            for mode in MODES:
                js = mode == "js_exact"
                if js and np.array_equal(b.tail(True), b.tail(False)):
                    self.want[k, mode] = self.want[k, "spec"]
                    continue
                w = torch.empty(b.n, dtype=torch.uint8, device="cuda")
                lits = _t(B.literals(b.per), np.uint8)
                reps = b.target // b.per
                w[:reps * b.per].view(reps, b.per).copy_(lits.unsqueeze(0).expand(reps, b.per))
                w[reps * b.per:b.target].copy_(lits[:b.target - reps * b.per])
                w[b.target:].copy_(_t(b.tail(js), np.uint8))
                self.want[k, mode] = w
        torch.cuda.synchronize()

    def reset(self, ks):
        for (a, n), img in zip(self.gaps, self.gap_img):
            self.t[a:a + n].copy_(img)
        for k in ks:
            self.t[self.pos[k]:self.pos[k] + self.blocks[k].n].fill_(SLOT_FILL)

    def check_gaps(self, what, fillers=()):
        """Everything outside the big slots is the pattern, but for the fillers' slots, which hold the fillers."""
        src = _t(B.filler()[0], np.uint8)
        for j in fillers:
            p = self.fill_pos[j]
            assert torch.equal(self.t[p:p + B.FILLER_N], src), (what, "filler", j)
            a, _ = self.gaps[-1]
            self.t[p:p + B.FILLER_N].copy_(self.gap_img[-1][p - a:p - a + B.FILLER_N])
        for g, ((a, n), img) in enumerate(zip(self.gaps, self.gap_img)):
            if not torch.equal(self.t[a:a + n], img):
                bad = torch.nonzero(self.t[a:a + n] != img).flatten()
                p = a + int(bad[0])
                near = [f"slot {k} ends {p - (q + b.n)} below" if p >= q + b.n else f"slot {k} starts {q - p} above"
                        for k, (q, b) in enumerate(zip(self.pos, self.blocks))]
                raise AssertionError(f"{what}: {int(bad.numel())} byte(s) outside the slots were written, first at arena "
                                     f"position {p} (value {int(self.t[p])}): {near}")

    def check_slot(self, k, mode, what):
        b, p = self.blocks[k], self.pos[k]
        got, want = self.t[p:p + b.n], self.want[k, mode]
        if torch.equal(got, want):
            return
        for a in range(0, b.n, PIECE):
            g, w = got[a:a + PIECE], want[a:a + PIECE]
            if not torch.equal(g, w):
                bad = torch.nonzero(g != w).flatten()
                y = a + int(bad[0])
                lo, hi = max(0, y - 8), min(b.n, y + 24)
                raise AssertionError(f"{what}: block {b.name} differs from the expected image, first at output position "
                                     f"{y} ({y:#x}; {int(bad.numel())} wrong byte(s) in its 16 MiB piece): {b.where(y)}; "
                                     f"got[{lo}:{hi}] = {got[lo:hi].cpu().tolist()}, "
                                     f"expected {want[lo:hi].cpu().tolist()}")


_live = {}


def _drop():
    _live.clear()
    torch.cuda.empty_cache()


def _arena(name):
    """The arena of a case; one at a time is kept on the device."""
    if name not in _live:
        _drop()
        _live[name] = Arena(B.case(name))
    return _live[name]


def _call(A, rows, mode, base=0):
    """One decode call: rows = [(compressed block, arena position, capacity)]; the out pointer is the arena's start
    plus `base`, the offsets relative to it -> (statuses, lengths)."""
    n = len(rows)
    comps = [np.ascontiguousarray(c) for c, _, _ in rows]
    ilen = np.array([c.size for c in comps], dtype=np.int64)
    ioff = np.zeros(n, dtype=np.int64)
    ioff[1:] = np.cumsum(ilen[:-1] + 33)                       # odd input positions
    arena = np.full(int(ioff[-1] + ilen[-1]) + 64, 0xC3, dtype=np.uint8)
    for c, o in zip(comps, ioff):
        arena[o:o + c.size] = c
    d_in, d_ioff, d_ilen = _t(arena, np.uint8), _t(ioff, np.int64), _t(ilen, np.int32)
    d_ooff = _t([p - base for _, p, _ in rows], np.int64)
    d_cap = _t(np.array([cap for _, _, cap in rows], dtype=np.uint32).view(np.int32), np.int32)
    d_len = torch.full((n + SENT,), FILL, dtype=torch.int32, device="cuda")
    d_st = torch.full((n + SENT,), FILL, dtype=torch.int32, device="cuda")
    lz4mi.decompress_blocks_dev(d_in.data_ptr(), d_ioff.data_ptr(), d_ilen.data_ptr(), A.t.data_ptr() + base,
                                d_ooff.data_ptr(), d_cap.data_ptr(), d_len.data_ptr(), d_st.data_ptr(), n, _stream(),
                                js_exact=mode == "js_exact")
    torch.cuda.synchronize()
    st, ln = d_st.cpu().numpy(), d_len.cpu().numpy().view(np.uint32)
    F.assert_sentinels(st, n, "status[]")
    F.assert_sentinels(ln.view(np.int32), n, "out_len[]")
    assert torch.equal(d_in, torch.from_numpy(arena).cuda()), "the input arena changed"
    return st[:n].tolist(), [int(x) for x in ln[:n]]


def _decode(A, ks, mode, route, what, base_at=None):
    """The blocks ks of the arena's case in one call on `route`; base_at: the slot the out pointer points at (out_off
    0 for it), else the arena's start (odd out_off)."""
    A.reset(ks)
    rows = [(A.blocks[k].comp, A.pos[k], A.blocks[k].n) for k in ks]
    where, fillers = list(range(len(ks))), []
    if route == "batch":
        at = {5: 0, NBATCH - 40: 1} if len(ks) == 2 else {NBATCH // 2: 0}
        full, where = [], [None] * len(ks)
        for j in range(NBATCH):
            if j in at:
                where[at[j]] = j
                full.append(rows[at[j]])
            else:
                fillers.append(j)
                full.append((B.filler()[1], A.fill_pos[j], B.FILLER_N))
        rows = full
        assert len(rows) == NBATCH > lz4mi.SMALL_BLOCKS
    else:
        assert len(rows) <= lz4mi.SMALL_BLOCKS and (route == "lone") == (len(rows) == 1)
    t0 = time.perf_counter()
    st, ln = _call(A, rows, mode, A.pos[base_at] if base_at is not None else 0)
    dt = time.perf_counter() - t0
    print(f"[big_blocks] {what}: {len(rows)} block(s), call {dt:.3f} s")
    assert CROSS not in st, (what, "ERR_CROSS_BLOCK", [j for j, s in enumerate(st) if s == CROSS])
    assert st == [0] * len(rows), (what, [(j, s) for j, s in enumerate(st) if s])
    for i, k in enumerate(ks):
        assert ln[where[i]] == A.blocks[k].n, (what, A.blocks[k].name, ln[where[i]])
    assert all(ln[j] == B.FILLER_N for j in fillers), what
    A.check_gaps(what, fillers)
    for k in ks:
        A.check_slot(k, mode, what)


def _batch_pair(name):
    """The two blocks of the case that ride in the batch-kernel call (another pair at each threshold)."""
    names = list(B.CASES)
    n = len(B.case(name))
    return [(0, 1), (1, 2), (0, 2)][names.index(name) % 3] if n > 2 else tuple(range(n))


def _routes(name, route, mode):
    A = _arena(name)
    n = len(A.blocks)
    what = f"{name}/{route}/{mode}"
    if route == "lone":
        # block 0 at out_off 0 and at an odd out_off, the others at one of the two in turn
        _decode(A, [0], mode, route, what + "/block0@0", base_at=0)
        _decode(A, [0], mode, route, what + "/block0@odd")
        for k in range(1, n):
            _decode(A, [k], mode, route, what + f"/block{k}@{'0' if k % 2 else 'odd'}", base_at=k if k % 2 else None)
    elif route == "small":
        _decode(A, list(range(n)), mode, route, what)
    else:
        _decode(A, list(_batch_pair(name)), mode, route, what)


@pytest.mark.parametrize("name,route,mode", [(n, r, m) for n in B.CASES for r in ROUTES for m in MODES])
def test_decode_across(name, route, mode):
    """The body across (or, `inside`, between) the positions where the decoder's 32-bit position fields change
    meaning. `inside` with tiles216 is the split-alias case: with kSplitBase = 0x20000000 the split mappings of
    sources in [2^29 - 65536, 2^29 + 2^27) were followed as whole-match memos (csrc/lz4mi_decompress.hip,
    remap_src)."""
    _routes(name, route, mode)


@pytest.mark.parametrize("route,mode", [(r, m) for r in ROUTES for m in MODES])
def test_top_edge(route, mode):
    """n == out_cap == 0x7FFFFFFF: the body ends on the last byte the ABI allows; two blocks of 2 GiB. An overrun
    of the slot would land in the 64 KiB behind it."""
    _routes("top", route, mode)


def test_top_edge_one_byte_too_long():
    """The first top-edge block with one more literal in the body's last run (2^31 bytes) in a slot of 0x7FFFFFFF:
    ERR_OUTPUT_TOO_SMALL, out_len 0, nothing written outside the slot -- lone and in the batch kernel."""
    A = _arena("top")
    blk = B.too_long()
    for route, mode in (("lone", "spec"), ("batch", "js_exact")):
        A.reset([0])
        rows, fillers = [(blk.comp, A.pos[0], B.MAX_BLOCK)], []
        if route == "batch":
            fillers = list(range(1, NBATCH))
            rows += [(B.filler()[1], A.fill_pos[j], B.FILLER_N) for j in fillers]
        st, ln = _call(A, rows, mode)
        assert (st[0], ln[0]) == (lz4mi.ERR_OUTPUT_TOO_SMALL, 0), (route, st[0], ln[0])
        assert st[1:] == [0] * len(fillers) and all(x == B.FILLER_N for x in ln[1:]), route
        A.check_gaps(f"too long/{route}", fillers)


def test_decoded_sizes_every_block():
    """lz4mi_decoded_sizes: (0, n) for every block of every case in one batch; one byte past the limit is
    ERR_OUTPUT_TOO_SMALL with 0x7FFFFFFF."""
    _drop()
    blocks = [b for name in list(B.CASES) + ["top"] for b in B.case(name)]
    st, sz = lz4mi.decoded_sizes([b.comp for b in blocks] + [B.too_long().comp])
    want = [(0, b.n) for b in blocks] + [(lz4mi.ERR_OUTPUT_TOO_SMALL, 0x7FFFFFFF)]
    assert [(int(s), int(z)) for s, z in zip(st, sz)] == want


# ------------------------------------------------------------------------------------------- the encoder
MIB = 1 << 20


@pytest.fixture(scope="module")
def composite():
    """40 MiB: tiles216, text, a 3 MiB zero run, then random runs, constant runs, short periods and copies from 1 to
    65535 bytes back and from beyond the window (test_gpu_fuzz._segmented_block): positions far past every epoch
    relabel of the encoder's table."""
    from test_gpu_fuzz import _segmented_block
    rng = np.random.default_rng(20261021)
    parts = [O.generate("tiles216", 21, 10 * MIB), O.generate("text", 22, 10 * MIB), np.zeros(3 * MIB, dtype=np.uint8),
             _segmented_block(rng, 17 * MIB)]
    data = np.concatenate(parts)
    assert data.size == 40 * MIB
    data.setflags(write=False)
    return data


def _first_diff(a, b):
    n = min(a.size, b.size)
    bad = np.nonzero(a[:n] != b[:n])[0]
    return int(bad[0]) if bad.size else n


@pytest.mark.parametrize("dev", [False, True], ids=["host_ptrs", "device_ptrs"])
def test_encode_blocks_above_4_mib(composite, dev):
    """lz4mi_compress_blocks on blocks of 4 MiB + 1, 8 MiB + 12345 and 40 MiB: the oracle's bytes, and the GPU decode
    returns the source."""
    srcs = [O.generate("text", 23, 4 * MIB + 1), O.generate("tiles216", 24, 8 * MIB + 12345), composite]
    want = [O.compress_block_bytes(s) for s in srcs]
    if dev:
        b = F.EncBatch("big", srcs)
        d_in, d_ioff = _t(b.in_arena(0), np.uint8), _t(b.in_offs, np.int64)
        d_ilen = _t([s.size for s in srcs], np.int32)
        d_out, d_ooff = _t(b.out_arena(0), np.uint8), _t(b.offs, np.int64)
        d_len = torch.full((b.n + SENT,), FILL, dtype=torch.int32, device="cuda")
        lz4mi.compress_blocks_dev(d_in.data_ptr() + F.MARGIN, d_ioff.data_ptr(), d_ilen.data_ptr(),
                                  d_out.data_ptr() + F.MARGIN, d_ooff.data_ptr(), d_len.data_ptr(), b.n, _stream())
        torch.cuda.synchronize()
        ln, out = d_len.cpu().numpy(), d_out.cpu().numpy()
        F.assert_sentinels(ln, b.n, "out_len[]")
        got = [out[F.MARGIN + o:F.MARGIN + o + int(n)] for o, n in zip(b.offs, ln[:b.n])]
    else:
        got = lz4mi.compress_blocks(srcs)
    for k, (g, w) in enumerate(zip(got, want)):
        assert g.size == w.size and np.array_equal(g, w), (k, g.size, w.size, _first_diff(g, w))
    if not dev:
        st, outs, lens = lz4mi.decompress_blocks(got, [s.size for s in srcs])
        for k, (s, o) in enumerate(zip(srcs, outs)):
            assert st[k] == 0 and lens[k] == s.size and np.array_equal(o, s), (k, st[k], _first_diff(o, s))


def test_encode_chain_of_8_mib_blocks(composite):
    """lz4mi_compress_chain, block_size 8 MiB + 4, 20 MiB from a non-zero start: every block and the final table
    equal the oracle's compressBlock per block with the table carried."""
    start, length, bs = 14 * MIB + 5001, 20 * MIB, 8 * MIB + 4
    data = np.ascontiguousarray(composite[:start + length + 777])
    t_ref = np.zeros(16384, dtype=np.int32)
    t_gpu = t_ref.copy()
    got = lz4mi.compress_chain(data, start, length, bs, t_gpu)
    pos, b = start, 0
    while pos < start + length:
        n = min(bs, start + length - pos)
        w, out, _ = O.compress_block(data, pos, n, t_ref)
        assert got[b].size == w and np.array_equal(got[b], out[:w]), (b, got[b].size, w, _first_diff(got[b], out[:w]))
        pos += n
        b += 1
    assert b == len(got) == 3
    assert np.array_equal(t_gpu, t_ref)


def test_encode_lone_9_mib_block_with_a_table(composite):
    """lz4mi_compress_block_table on a lone 9 MiB block with a caller table and room for the bound (the GPU route):
    bytes and table equal the oracle's."""
    start, n = 9 * MIB + 77, 9 * MIB
    data = np.ascontiguousarray(composite[:start + n + 100])
    rng = np.random.default_rng(5)
    t_ref = rng.integers(0, start, 16384).astype(np.int32)        # a table a caller carried: positions below the block
    t_gpu = t_ref.copy()
    out = np.full(lz4mi.compress_bound(n) + 7, FILL, dtype=np.uint8)
    w = lz4mi.compress_raw(data, out, start, n, t_gpu, 7)
    ref = np.full(out.size, FILL, dtype=np.uint8)
    rw, ref, _ = O.compress_block(data, start, n, t_ref, ref, 7)
    assert w == rw, (w, rw)
    assert np.array_equal(out, ref), _first_diff(out, ref)
    assert np.array_equal(t_gpu, t_ref)
