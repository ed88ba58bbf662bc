"""WHERE the kernels write (tests/footprint_common.py): every route is called through device
pointers on a caller-owned arena whose every byte is known beforehand, and the whole arena
afterwards -- margins, guards, slot tails, the bytes below out[0], the out_len[] / status[]
sentinels, the input arena -- is compared with the image the CPU oracle says the reference
leaves. Each case runs on two complementary pre-fills; tests/test_footprint_cpu.py checks the
model and the conditions on these batches without a GPU."""
import numpy as np
import pytest

import oracle as O
import footprint_common as F
import sizes_common

lz4mi = pytest.importorskip("lz4mi")
torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

MARGIN, FILL, SENT = F.MARGIN, F.FILL, F.SENTINELS


@pytest.fixture(scope="module", autouse=True)
def _device():
    lz4mi.init(0)


def _dev(batch, run):
    return F.dev_decode(lz4mi, batch, run)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _t(a, dt):
    return torch.from_numpy(np.ascontiguousarray(a).astype(dt)).cuda()


# ---- 1. the small path ------------------------------------------------------------------------
@pytest.mark.parametrize("reparse", [0, 2])
@pytest.mark.parametrize("mode", ["spec", "js_exact"])
@pytest.mark.parametrize("size", [3, 7])
def test_small_path(size, mode, reparse, monkeypatch):
    """Every block and capacity of the table in calls of 3 and of 7 blocks (the pointer pipeline of
    csrc/lz4mi_expand.hip; ratio >= 32 blocks by one wave of the same launch), with the segment
    re-parse forced or not."""
    if reparse:
        monkeypatch.setenv("LZ4MI_SMALL_REPARSE", str(reparse))
    for b in F.batches(size, mode, False):
        F.check_batch(b, _dev)


def test_small_path_four_mib_run():
    """One match of 4 MiB - 3 at offset 1 behind 20 literals, no final literals, in a slot one byte
    short at an odd offset: status 0, out_len = N > cap, clipped at the capacity."""
    m = F.Maker(661)
    m.pos = 0
    comp = F.encode([m.seq(20, (4 << 20) - 3, off=1)], None)
    n = 20 + (4 << 20) - 3
    t = F.table()["lit_short"]
    b = F.Batch("four_mib", [t.comp, comp, t.comp], [t.n + 1, n - 1, t.n])
    assert F.check_batch(b, _dev) == [0, 0, 0]


# ---- 2. the batch kernel ----------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["spec", "js_exact"])
def test_batch_kernel(mode):
    """SMALL_BLOCKS + 8 blocks per call: one wave per block (csrc/lz4mi_decompress.hip)."""
    for b in F.batches(lz4mi.SMALL_BLOCKS + 8, mode):
        assert b.n == lz4mi.SMALL_BLOCKS + 8
        F.check_batch(b, _dev)


# ---- 3. lone blocks ---------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["spec", "js_exact", "js_compat"])
def test_lone_block(mode):
    """nblocks == 1 at out_off 0, 3 and 300: the bytes below the slot are history, then the
    dictionary. The reference modes' rewrite below the slot (f1_first) is the only change outside
    it; js_compat is the serial kernel (csrc/lz4mi_decompress_serial.hip)."""
    for b in F.lone_batches(mode):
        F.check_batch(b, _dev)


def test_js_compat_batches_of_four():
    for b in F.batches(4, "js_compat", False):
        F.check_batch(b, _dev)


# ---- 4. linked and linked exact ---------------------------------------------------------------
@pytest.mark.parametrize("window", [0, 2])
@pytest.mark.parametrize("which", ["ok", "fail"])
@pytest.mark.parametrize("mode", ["linked", "linked_exact"])
def test_linked(mode, which, window, monkeypatch):
    """Five dependent blocks with guards between the slots, a slot with an unused tail, a stored
    block; `fail`: block 2 one byte short, the blocks after it are not written. Windows of two
    blocks put the failure and a gap on a window edge. Reference mode: block 3's rewrite of the
    bytes below its slot (block 2's tail) is exactly the oracle's."""
    if window:
        monkeypatch.setenv("LZ4MI_LINKED_WINDOW", str(window))
    st = F.check_batch(F.linked_batch(which, mode), _dev)
    assert st == ([0] * 5 if which == "ok" else [0, 0, F.TOO_SMALL, F.CROSS, F.CROSS])


# ---- 5. decoded sizes -------------------------------------------------------------------------
def test_decoded_sizes_writes_two_arrays_only():
    """lz4mi_decoded_sizes on the batch kernel's blocks: out_len[0 .. n) and status[0 .. n) are
    the walker's, their sentinels and the whole input arena are untouched, and an output arena
    that the call is not given stays as it was."""
    for b in F.batches(lz4mi.SMALL_BLOCKS + 8, "spec"):
        want = [(0, p.size) if s else sizes_common.walk(p) for p, s in zip(b.pays, b.stored)]
        seen = []
        for run in (0, 1):
            d_in, d_out = _t(b.in_arena(run), np.uint8), _t(b.out_arena(run), np.uint8)
            d_ioff, d_ilen = _t(b.in_offs, np.int64), _t(b.words().view(np.int32), np.int32)
            d_len = torch.full((b.n + SENT,), FILL, dtype=torch.int32, device="cuda")
            d_st = torch.full((b.n + SENT,), FILL, dtype=torch.int32, device="cuda")
            lz4mi.decoded_sizes_dev(d_in.data_ptr() + MARGIN, d_ioff.data_ptr(), d_ilen.data_ptr(), d_len.data_ptr(),
                                    d_st.data_ptr(), b.n, _stream(), frame_words=True)
            torch.cuda.synchronize()
            st, ln = d_st.cpu().numpy(), d_len.cpu().numpy()
            assert [(int(s), int(x)) for s, x in zip(st[:b.n], ln[:b.n])] == want, (b.name, run)
            F.assert_sentinels(st, b.n, "status[]")
            F.assert_sentinels(ln, b.n, "out_len[]")
            assert np.array_equal(d_in.cpu().numpy(), b.in_arena(run)), (b.name, run, "the input arena changed")
            assert np.array_equal(d_out.cpu().numpy(), b.out_arena(run)), (b.name, run, "the output arena changed")
            seen.append((st.tolist(), ln.tolist()))
        assert seen[0] == seen[1]


# ---- 6. the encoder ---------------------------------------------------------------------------
def _dev_encode(b, run):
    d_in, d_out = _t(b.in_arena(run), np.uint8), _t(b.out_arena(run), np.uint8)
    d_ioff, d_ilen = _t(b.in_offs, np.int64), _t([s.size for s in b.srcs], np.int32)
    d_ooff = _t(b.offs, np.int64)
    d_len = torch.full((b.n + SENT,), FILL, dtype=torch.int32, device="cuda")
    lz4mi.compress_blocks_dev(d_in.data_ptr() + MARGIN, d_ioff.data_ptr(), d_ilen.data_ptr(), d_out.data_ptr() + MARGIN,
                              d_ooff.data_ptr(), d_len.data_ptr(), b.n, _stream())
    torch.cuda.synchronize()
    return d_out.cpu().numpy(), d_in.cpu().numpy(), d_len.cpu().numpy()


@pytest.mark.parametrize("nblocks", [20, 770])
def test_encoder(nblocks):
    """lz4mi_compress_blocks into slots of exactly compress_bound(n) bytes at odd offsets with 1 KiB
    guards: the oracle encoder's bytes in [off, off + len) and nothing else, the slot's own tail
    [off + len, off + bound) included. 20 blocks take the kernel with the hash table in LDS, 770 the
    one with the tables in global memory (kLdsTableMaxBlocks = 768)."""
    b = F.encoder_batch(nblocks)
    for run in (0, 1):
        image, lens = b.expected(run)
        got, got_in, glen = _dev_encode(b, run)
        assert [int(x) for x in glen[:b.n]] == lens, (run, F._first_diff(glen[:b.n], lens))
        F.assert_sentinels(glen, b.n, "out_len[]")
        F.assert_footprint(got, image, np.ones(image.size, dtype=bool), F.Regions(b.offs, b.bounds, lens),
                           f"encoder {nblocks} run {run}")
        assert np.array_equal(got_in, b.in_arena(run)), (run, "the input arena changed")


# ---- 7. related entry points ------------------------------------------------------------------
@pytest.mark.parametrize("block_checksum", [False, True])
def test_frame_pack(block_checksum):
    """lz4mi_frame_pack: the records equal the reference frame's, the frame buffer beyond the last
    record and its margins are untouched."""
    from lz4mi import shard
    data = np.concatenate([O.generate("tiles216", 8, 200000), O.generate("random", 9, 70001)])
    bsize = 65536
    ref = O.compress_frame(data, None, bsize, True, False, True, block_checksum=block_checksum)
    _, blocks = shard.frame_blocks(ref)
    records = ref[blocks[0][0] - 4:ref.size - 4]
    nb = len(blocks)
    sizes = [min(bsize, data.size - k * bsize) for k in range(nb)]
    comps = [O.compress_block_bytes(data[k * bsize:k * bsize + n]) for k, n in enumerate(sizes)]
    slot = lz4mi.compress_bound(bsize)
    comp = np.zeros(nb * slot, dtype=np.uint8)
    for k, c in enumerate(comps):
        comp[k * slot:k * slot + c.size] = c
    rec = [(n if c.size >= n else c.size) + (8 if block_checksum else 4) for c, n in zip(comps, sizes)]
    rec_off = np.cumsum([0] + rec[:-1])
    assert sum(rec) == records.size
    for run in (0, 1):
        init = F.pattern(2 * MARGIN + records.size + 333, run)
        d_frame = _t(init, np.uint8)
        d_raw, d_comp = _t(data, np.uint8), _t(comp, np.uint8)
        d_roff, d_rlen = _t(np.arange(nb) * bsize, np.int64), _t(sizes, np.int32)
        d_coff, d_clen = _t(np.arange(nb) * slot, np.int64), _t([c.size for c in comps], np.int32)
        d_rec = _t(rec_off, np.int64)
        lz4mi.frame_pack_dev(d_raw.data_ptr(), d_roff.data_ptr(), d_rlen.data_ptr(), d_comp.data_ptr(), d_coff.data_ptr(),
                             d_clen.data_ptr(), d_frame.data_ptr() + MARGIN + 1, d_rec.data_ptr(), nb, _stream(),
                             block_checksum=block_checksum)
        torch.cuda.synchronize()
        image = init.copy()
        image[MARGIN + 1:MARGIN + 1 + records.size] = records
        F.assert_footprint(d_frame.cpu().numpy(), image, np.ones(image.size, dtype=bool),
                           F.Regions([1 + int(o) for o in rec_off], rec), f"frame_pack run {run}")
        assert np.array_equal(d_raw.cpu().numpy(), data) and np.array_equal(d_comp.cpu().numpy(), comp)


# payload lengths at the edges of the whole-wave copy (wave_copy, csrc/lz4mi_common.h): below one 16-byte piece,
# around one and two pieces, around one full trip of its loop (4 x 64 lanes x 16 bytes = 4096), and two trips
COPY_EDGES = (0, 1, 15, 16, 17, 31, 32, 33, 4095, 4096, 4097, 8197)


def _le32(x):
    return np.array([x & 0xFFFFFFFF], dtype="<u4").view(np.uint8)


def test_wave_copy_edges():
    """(a) lz4mi_frame_pack: per length L > 0 one stored record (comp_len 0, raw_len L) and one compressed record
    (comp_len L of arbitrary bytes, raw_len L + 1), at odd rec_off with a few bytes between two records, the
    sources at all sixteen address residues, with and without block checksums: size word, payload and the
    spec XXH32 assembled in numpy, nothing else written.
    (b) lz4mi_frame_decompress: stored blocks of every length, content size their sum, at an odd frame and an
    odd output address: the output is their concatenation, nothing outside out[0 .. content size) is written
    (the 4 KiB behind out_cap, the margins). The call sizes its lists from content size / block_max, two blocks
    for these sizes, and declines a frame with more (the parent commit's library too): so the lengths go
    through it as six frames of two stored blocks each."""
    rng = np.random.default_rng(720)
    # ---- (a)
    recs = [(L, stored) for L in COPY_EDGES if L for stored in (True, False)]
    src_off, at = [], 0
    for k, (L, _) in enumerate(recs):
        at += (k % 16 - at) % 16
        src_off.append(at)
        at += L + 16
    assert {o % 16 for o in src_off} == set(range(16))
    raw, comp = rng.integers(0, 256, at, dtype=np.uint8), rng.integers(0, 256, at, dtype=np.uint8)
    for block_checksum in (False, True):
        rec_off, sizes, at = [], [], 1
        for k, (L, _) in enumerate(recs):
            rec_off.append(at)
            sizes.append(4 + L + (4 if block_checksum else 0))
            at = (at + sizes[-1] + 5 + 2 * (k % 3)) | 1    # (every rec_off odd)
        assert all(o % 2 for o in rec_off)
        span = at
        d_raw, d_comp = _t(raw, np.uint8), _t(comp, np.uint8)
        d_off = _t(src_off, np.int64)
        d_rlen = _t([L if st else L + 1 for L, st in recs], np.int32)
        d_clen = _t([0 if st else L for L, st in recs], np.int32)
        d_rec = _t(rec_off, np.int64)
        for run in (0, 1):
            init = F.pattern(2 * MARGIN + span, run)
            image = init.copy()
            for (L, st), so, ro in zip(recs, src_off, rec_off):
                pay = (raw if st else comp)[so:so + L]
                parts = [_le32(L | (0x80000000 if st else 0)), pay] + ([_le32(O.xxh32_std(pay))] if block_checksum else [])
                r = np.concatenate(parts)
                image[MARGIN + ro:MARGIN + ro + r.size] = r
            d_frame = _t(init, np.uint8)
            lz4mi.frame_pack_dev(d_raw.data_ptr(), d_off.data_ptr(), d_rlen.data_ptr(), d_comp.data_ptr(), d_off.data_ptr(),
                                 d_clen.data_ptr(), d_frame.data_ptr() + MARGIN, d_rec.data_ptr(), len(recs), _stream(),
                                 block_checksum=block_checksum)
            torch.cuda.synchronize()
            F.assert_footprint(d_frame.cpu().numpy(), image, np.ones(image.size, dtype=bool), F.Regions(rec_off, sizes),
                               f"frame_pack copy edges, checksums {block_checksum}, run {run}")
            assert np.array_equal(d_raw.cpu().numpy(), raw) and np.array_equal(d_comp.cpu().numpy(), comp)
    # ---- (b)
    from lz4mi import frame as FR
    seen = []
    for k in range(0, len(COPY_EDGES), 2):
        pays = [rng.integers(0, 256, L, dtype=np.uint8) for L in COPY_EDGES[k:k + 2]]
        seen += [p.size for p in pays]
        size = sum(p.size for p in pays)
        head = np.frombuffer(FR.header(65536, True, False, size), dtype=np.uint8)
        f = np.concatenate([head] + [x for p in pays for x in (_le32(p.size | 0x80000000), p)] + [_le32(0)])
        d_f = torch.zeros(f.size + 3, dtype=torch.uint8, device="cuda")
        d_f[3:] = torch.from_numpy(f).cuda()
        for run in (0, 1):
            init = F.pattern(2 * MARGIN + 1 + size, run)
            d_out = _t(init, np.uint8)
            info = lz4mi.frame_decompress_dev(d_f.data_ptr() + 3, f.size, d_out.data_ptr() + MARGIN + 1, size, _stream())
            torch.cuda.synchronize()
            assert (info["status"], info["content_size"], info["written"], info["stored_blocks"]) == (0, size, size, 2)
            image = init.copy()
            image[MARGIN + 1:MARGIN + 1 + size] = np.concatenate(pays)
            F.assert_footprint(d_out.cpu().numpy(), image, np.ones(image.size, dtype=bool), F.Regions([1], [size]),
                               f"frame_decompress stored {[p.size for p in pays]} run {run}")
    assert tuple(seen) == COPY_EDGES


@pytest.mark.parametrize("bsize", [4099, 8190])
def test_generate_blocks(bsize):
    """lz4mi_generate_blocks writes out[0 .. nblocks * bsize) and nothing else."""
    nb = 5
    for run, kind in ((0, "tiles216"), (1, "random")):
        init = F.pattern(2 * MARGIN + nb * bsize + 100, run)
        d = _t(init, np.uint8)
        lz4mi.generate_blocks_dev(d.data_ptr() + MARGIN + 3, kind, 11, bsize, nb, _stream())
        torch.cuda.synchronize()
        image = init.copy()
        for k in range(nb):
            image[MARGIN + 3 + k * bsize:MARGIN + 3 + (k + 1) * bsize] = O.generate(kind, 11 + k, bsize)
        F.assert_footprint(d.cpu().numpy(), image, np.ones(image.size, dtype=bool),
                           F.Regions([3 + k * bsize for k in range(nb)], [bsize] * nb), f"generate {kind}")


def test_xxh32_blocks_sentinels():
    b = F.encoder_batch(20)
    d_in = _t(b.in_arena(1), np.uint8)
    d_off, d_len = _t(b.in_offs, np.int64), _t([s.size for s in b.srcs], np.int32)
    d_h = torch.full((b.n + SENT,), FILL, dtype=torch.int32, device="cuda")
    lz4mi.xxh32_blocks_dev(d_in.data_ptr() + MARGIN, d_off.data_ptr(), d_len.data_ptr(), d_h.data_ptr(), b.n, 0, _stream())
    torch.cuda.synchronize()
    h = d_h.cpu().numpy()
    assert [int(x) & 0xFFFFFFFF for x in h[:b.n]] == [O.xxh32(s) for s in b.srcs]
    F.assert_sentinels(h, b.n, "hashes[]")
    assert np.array_equal(d_in.cpu().numpy(), b.in_arena(1))


@pytest.mark.parametrize("mode", ["spec", "js_exact", "js_compat"])
def test_host_pointer_copy_back(mode):
    """lz4mi.decompress_raw on the caller's host array at an odd offset: after the call the whole
    array equals the oracle's image (the copy-back's footprint), for blocks that fit, roomy slots,
    clipped matches and the rewrite below the slot."""
    t = F.table()
    cases = [(t["lit_300"], t["lit_300"].n, 301), (t["match_end"], t["match_end"].n - 16, 301),
             (t["per_3_fin"], t["per_3_fin"].n + 5000, 4095), (t["per_long_251"], t["per_long_251"].n - 1, 77),
             (t["f1_first"], t["f1_first"].n + 16, 300), (t["hist"], t["hist"].n, 300)]
    for r, cap, first in cases:
        b = F.Batch(f"host_{r.name}", [r.comp], [cap], mode=mode, first=first)
        for run in (0, 1):
            init = b.out_arena(run)
            image, care, st, ln = F.expected_image(init, b.pays, (b.offs, b.caps), mode)
            assert st == [0] and care.all()
            got = init.copy()
            n = lz4mi.decompress_raw(b.in_arena(run), MARGIN + b.in_offs[0], r.comp.size, got[MARGIN:MARGIN + first + cap],
                                     first, js_compat=mode == "js_compat", js_exact=mode == "js_exact")
            assert n == ln[0], (r.name, mode, run)
            F.assert_footprint(got, image, care, F.Regions(b.offs, b.caps, ln), f"{b.name} [{mode}] run {run}")


def test_host_pointer_compress_raw():
    """lz4mi.compress_raw into the caller's host array at an odd offset, room for exactly
    compress_bound(n): the oracle encoder's bytes and nothing else."""
    for s in (F.encoder_inputs()[9], F.encoder_inputs()[14]):
        for run in (0, 1):
            init = F.pattern(2 * MARGIN + O.compress_bound(s.size), run)
            got = init.copy()
            table = np.zeros(16384, dtype=np.int32)
            n = lz4mi.compress_raw(s, got[:MARGIN + O.compress_bound(s.size)], 0, s.size, table, MARGIN)
            c = O.compress_block_bytes(s)
            image = init.copy()
            image[MARGIN:MARGIN + c.size] = c
            assert n == c.size
            F.assert_footprint(got, image, np.ones(image.size, dtype=bool),
                               F.Regions([0], [O.compress_bound(s.size)], [n]), f"compress_raw {s.size} run {run}")
