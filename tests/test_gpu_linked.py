"""Linked batches (LZ4MI_LINKED): the blocks of a dependent-block frame decoded in one call.
Each block may reference the 64 KiB of output before it; the small path's pointers are resolved
across the blocks of a window (csrc/lz4mi_expand.hip, "linked mode"). The checker is the oracle
(oracle/lz4_oracle.c): its frame decode, and its block decoder run in index order on one output
array, which is what the flag's contract promises (include/lz4mi.h): bytes, lengths, statuses,
and ERR_CROSS_BLOCK for every block after the first failing one."""
import numpy as np
import pytest

import oracle as O

lz4mi = pytest.importorskip("lz4mi")
from lz4mi import shard  # noqa: E402

pytestmark = pytest.mark.gpu

BS = 65536


@pytest.fixture(scope="module", autouse=True)
def _device():
    lz4mi.init(0)


def _blocks_of(frame):
    """(payloads, stored flags) of a frame's blocks in order."""
    _, blocks = shard.frame_blocks(frame)
    return [frame[p:p + n].copy() for p, n, _ in blocks], [s for _, _, s in blocks]


def _sizes(total, bs):
    return [min(bs, total - p) for p in range(0, total, bs)]


def _dependent(data, bs=BS):
    """Payloads and decoded sizes of data's dependent-block frame; no stored block."""
    pay, stored = _blocks_of(O.compress_frame(data, None, bs, False, False, True))
    assert not any(stored)
    return pay, _sizes(data.size, bs)


def _in_order(pay, caps, dictionary=None):
    """The oracle's decoder on the blocks in index order on one output array (slots back to back,
    each block's capacity its slot): statuses with the after-failure rule, lengths, the array."""
    out = np.zeros(max(1, sum(caps)), dtype=np.uint8)
    st, ln, pos, failed = [], [], 0, False
    for c, cap in zip(pay, caps):
        if failed:
            st.append(lz4mi.ERR_CROSS_BLOCK)
            ln.append(0)
        else:
            s, w, _ = O.decompress_block(c, cap, out=out[:pos + cap], out_off=pos, dictionary=dictionary)
            st.append(s)
            ln.append(w if s == 0 else 0)
            failed = s != 0
        pos += cap
    return st, ln, out


@pytest.fixture(scope="module")
def case1():
    data = np.concatenate([O.generate("tiles216", 11, 250000), O.generate("text", 12, 250000),
                           O.generate("repetitive", 13, 100000)])
    pay, sizes = _dependent(data)
    return data, pay, sizes


def _check_equal(pay, sizes, data, **kw):
    st, outs, lens = lz4mi.decompress_blocks(pay, sizes, linked=True, **kw)
    assert (st == 0).all(), st
    assert [int(x) for x in lens] == list(sizes)
    assert np.array_equal(np.concatenate(outs), data)


def test_parity_smallest_shape(case1):
    data, pay, sizes = case1
    st, _, _ = lz4mi.decompress_blocks(pay, sizes)
    assert (st == lz4mi.ERR_CROSS_BLOCK).any()       # the blocks do depend on each other
    _check_equal(pay, sizes, data)


@pytest.mark.parametrize("name", ["period60000", "repetitive", "text"])
def test_shortcut_traps(name):
    """Blocks the unlinked small path would decode with one wave (ratio >= 32: a few matches at
    offset 60 000 into the predecessor; an overlapping match whose period lies in the previous
    block) and chains deeper than the jump rounds that cross blocks in the chase (text)."""
    pytest.importorskip("torch")
    if name == "period60000":
        data = np.resize(np.random.default_rng(5).integers(0, 256, 60000, dtype=np.uint8), 1200000)
    elif name == "repetitive":
        data = O.generate("repetitive", 1, 300000)
        assert np.array_equal(data[:600], np.arange(600) % 251)
    else:
        data = O.generate("text", 21, 1 << 20)
    frame = O.compress_frame(data, None, BS, False, False, True)
    est, eo = O.decompress_frame(frame, verify_checksum=False)
    assert est == 0 and np.array_equal(eo, data)
    pay, stored = _blocks_of(frame)
    sizes = _sizes(data.size, BS)
    if name == "period60000":   # (the reference's encoder finds the period in every other block; the last is stored)
        assert sum(p.size * 32 <= n for p, n in zip(pay, sizes)) >= 8
    if name == "repetitive":
        assert all(p.size * 32 <= n for p, n in zip(pay, sizes))
    if not any(stored):
        _check_equal(pay, sizes, data)
    words = [p.size | (0x80000000 if s else 0) for p, s in zip(pay, stored)]
    st, ln, out = _dev(pay, words, np.zeros(data.size, dtype=np.uint8), [b * BS for b in range(len(pay))], sizes,
                       frame_words=True)
    assert not st.any() and ln.tolist() == sizes and np.array_equal(out, data)


def test_four_mib_blocks():
    data = O.generate("tiles216", 31, 3 * (4 << 20))
    pay, sizes = _dependent(data, 4 << 20)
    assert len(pay) == 3
    _check_equal(pay, sizes, data)


def test_independent_blocks_linked():
    srcs = [O.generate("tiles216", 41 + k, 4 << 20) for k in range(3)]
    comps = [O.compress_block_bytes(s) for s in srcs]
    sizes = [s.size for s in srcs]
    st0, outs0, lens0 = lz4mi.decompress_blocks(comps, sizes)
    st1, outs1, lens1 = lz4mi.decompress_blocks(comps, sizes, linked=True)
    assert (st0 == 0).all() and (st1 == 0).all() and np.array_equal(lens0, lens1)
    for a, b, s in zip(outs0, outs1, srcs):
        assert np.array_equal(a, b) and np.array_equal(b, s)


@pytest.mark.parametrize("window", [1, 3, None])
def test_windows(case1, window, monkeypatch):
    """The batch cut into windows of 1, 3 and all blocks (test hook LZ4MI_LINKED_WINDOW, read per
    call): earlier windows' output is history for the later ones; the same bytes each time."""
    data, pay, sizes = case1
    if window:
        monkeypatch.setenv("LZ4MI_LINKED_WINDOW", str(window))
    _check_equal(pay, sizes, data)


def _first_offset_pos(c):
    """Position of the first sequence's match offset in a compressed block."""
    ll = int(c[0]) >> 4
    p = 1
    if ll == 15:
        while True:
            v = int(c[p])
            p += 1
            ll += v
            if v != 255:
                break
    return p + ll


@pytest.mark.parametrize("how", ["truncated", "offset0", "before_out0"])
@pytest.mark.parametrize("window", [None, 2])
def test_failure_rule(case1, how, window, monkeypatch):
    data, pay, sizes = case1
    k = 0 if how == "before_out0" else 4
    bad = [p.copy() for p in pay]
    if how == "truncated":
        bad[k] = bad[k][:bad[k].size - 9].copy()
    else:
        q = _first_offset_pos(bad[k])
        bad[k][q] = bad[k][q + 1] = 0 if how == "offset0" else 0xFF
    # the status of an nblocks == 1 call at the block's position, on the bytes before it
    alone = np.zeros(data.size, dtype=np.uint8)
    alone[:k * BS] = data[:k * BS]
    with pytest.raises(lz4mi.Lz4miError) as ei:
        lz4mi.decompress_raw(bad[k], 0, bad[k].size, alone[:k * BS + sizes[k]], k * BS)
    want = ei.value.status
    est, _, _ = _in_order(bad, sizes)
    assert est[k] == want and want in (lz4mi.ERR_MALFORMED, lz4mi.ERR_OFFSET0, lz4mi.ERR_DICT_OOB,
                                       lz4mi.ERR_OUTPUT_TOO_SMALL)
    if window:
        monkeypatch.setenv("LZ4MI_LINKED_WINDOW", str(window))
    st, outs, lens = lz4mi.decompress_blocks(bad, sizes, linked=True)
    assert [int(x) for x in st] == est, (st, est)
    for b in range(k):
        assert lens[b] == sizes[b] and np.array_equal(outs[b], data[b * BS:b * BS + sizes[b]]), b
    assert not lens[k:].any()


def test_scratch_allocation_failure_decodes_block_by_block(case1, monkeypatch):
    """When the window scratch cannot be allocated (a real hipMalloc failure: the test hook
    LZ4MI_TEST_SCRATCH_EXTRA_MB asks for a petabyte more) the call decodes one block per launch in
    order: the same bytes, statuses and after-failure rule."""
    data, pay, sizes = case1
    monkeypatch.setenv("LZ4MI_TEST_SCRATCH_EXTRA_MB", str(1 << 30))
    _check_equal(pay, sizes, data)
    bad = [p.copy() for p in pay]
    bad[4] = bad[4][:bad[4].size - 9].copy()
    est, eln, _ = _in_order(bad, sizes)
    st, outs, lens = lz4mi.decompress_blocks(bad, sizes, linked=True)
    assert [int(x) for x in st] == est and [int(x) for x in lens] == eln
    for b in range(4):
        assert np.array_equal(outs[b], data[b * BS:b * BS + sizes[b]]), b
    monkeypatch.delenv("LZ4MI_TEST_SCRATCH_EXTRA_MB")
    _check_equal(pay, sizes, data)


# ---- device pointers -------------------------------------------------------------------------
def _dev(pay, words, out_init, out_off, out_cap, dictionary=None, frame_words=False, linked=True):
    """One device-pointer call on torch tensors -> (status, out_len, out) as numpy."""
    import torch
    src, in_off, _ = lz4mi._pack([lz4mi._u8(p) for p in pay])
    t = lambda a, dt: torch.from_numpy(np.asarray(a).astype(dt)).cuda()
    d_in, d_ioff, d_w = t(src, np.uint8), t(in_off, np.int64), t(np.asarray(words, dtype=np.uint32).view(np.int32), np.int32)
    d_out, d_ooff, d_cap = t(out_init, np.uint8), t(out_off, np.int64), t(out_cap, np.int32)
    d_len = torch.full((len(pay),), 77, dtype=torch.int32, device="cuda")
    d_st = torch.full((len(pay),), 77, dtype=torch.int32, device="cuda")
    d_dict = None if dictionary is None else t(dictionary, np.uint8)
    lz4mi.decompress_blocks_dev(d_in.data_ptr(), d_ioff.data_ptr(), d_w.data_ptr(), d_out.data_ptr(), d_ooff.data_ptr(),
                                d_cap.data_ptr(), d_len.data_ptr(), d_st.data_ptr(), len(pay),
                                torch.cuda.current_stream().cuda_stream,
                                dict_ptr=None if d_dict is None else d_dict.data_ptr(),
                                dict_len=0 if d_dict is None else d_dict.numel(), frame_words=frame_words, linked=linked)
    torch.cuda.synchronize()
    return d_st.cpu().numpy(), d_len.cpu().numpy(), d_out.cpu().numpy()


def test_device_history_before_first_slot(case1):
    pytest.importorskip("torch")
    data, pay, sizes = case1
    k = 2                                              # blocks k.. decoded behind the caller's first k blocks
    init = np.zeros(data.size, dtype=np.uint8)
    init[:k * BS] = data[:k * BS]
    off = [b * BS for b in range(k, len(pay))]
    st, ln, out = _dev(pay[k:], [p.size for p in pay[k:]], init, off, sizes[k:])
    assert not st.any() and ln.tolist() == sizes[k:] and np.array_equal(out, data)
    # without the history the first block's references read other bytes: the test does depend on it
    st, ln, out = _dev(pay[k:], [p.size for p in pay[k:]], np.zeros(data.size, dtype=np.uint8), off, sizes[k:])
    assert not np.array_equal(out[k * BS:], data[k * BS:])


def test_device_gap_with_stored_block():
    pytest.importorskip("torch")
    rnd = O.generate("random", 51, BS)
    data = np.concatenate([O.generate("text", 52, BS), rnd, rnd[1000:30000], O.generate("text", 53, 2 * BS - 29000)])
    frame = O.compress_frame(data, None, BS, False, False, True)
    pay, stored = _blocks_of(frame)
    sizes = _sizes(data.size, BS)
    assert stored == [False, True, False, False]
    # the block after the stored one copies from it
    st, _, _ = lz4mi.decompress_blocks([pay[2]], [sizes[2]])
    assert st[0] != 0
    # (i) the stored block copied beforehand: it lies in a gap between the slots of the batch
    comp = [0, 2, 3]
    init = np.zeros(data.size, dtype=np.uint8)
    init[BS:2 * BS] = rnd
    st, ln, out = _dev([pay[b] for b in comp], [pay[b].size for b in comp], init, [b * BS for b in comp],
                       [sizes[b] for b in comp])
    assert not st.any() and ln.tolist() == [sizes[b] for b in comp] and np.array_equal(out, data)
    # (ii) the stored block in the batch, as a frame size word, copied by the call
    words = [p.size | (0x80000000 if s else 0) for p, s in zip(pay, stored)]
    st, ln, out = _dev(pay, words, np.zeros(data.size, dtype=np.uint8), [b * BS for b in range(4)], sizes,
                       frame_words=True)
    assert not st.any() and ln.tolist() == sizes and np.array_equal(out, data)


def test_device_golden_dependent_frames_with_dictionary(manifest):
    pytest.importorskip("torch")
    from conftest import cases_of, golden_bytes
    (g,) = cases_of(manifest, "frames")
    seen = 0
    for f in g["frames"]:
        if f["indep"] or not ("dict" in f or "dict_text" in f):
            continue
        if "dict" in f:
            dic = O.generate(f["dict"]["gen"], f["dict"]["seed"], f["dict"]["n"])
            data = O.generate("text", 5, 300000)[:f["n"]]
            frame = golden_bytes(f["frame_file"]).copy()
        else:
            dic = np.frombuffer(f["dict_text"].encode(), dtype=np.uint8)
            data = np.frombuffer(f["input_text"].encode(), dtype=np.uint8)
            frame = np.frombuffer(bytes.fromhex(f["frame_hex"]), dtype=np.uint8)
        est, eo = O.decompress_frame(frame, dic, verify_checksum=False)
        assert est == 0 and np.array_equal(eo, data)
        pay, stored = _blocks_of(frame)
        sizes = _sizes(data.size, f["block"])
        off = np.cumsum([0] + sizes[:-1]).tolist()
        words = [p.size | (0x80000000 if s else 0) for p, s in zip(pay, stored)]   # (the 56-byte message is stored)
        st, ln, out = _dev(pay, words, np.zeros(data.size, dtype=np.uint8), off, sizes, dictionary=dic, frame_words=True)
        assert not st.any() and ln.tolist() == sizes and np.array_equal(out, data), f["input"]
        if not any(stored):   # host pointers too
            _check_equal(pay, sizes, data, dictionary=dic)
        seen += 1
    assert seen >= 2


def test_refusals(case1):
    pytest.importorskip("torch")
    data, pay, sizes = case1
    n = len(pay)
    off = [b * BS for b in range(n)]
    words = [p.size for p in pay]
    zeros = np.zeros(data.size + (8 << 20), dtype=np.uint8)
    cross = lz4mi.ERR_CROSS_BLOCK
    # slot 3 overlaps slot 2
    bad_off = list(off)
    bad_off[3] = off[3] - 1
    st, ln, out = _dev(pay, words, zeros, bad_off, sizes)
    assert st.tolist() == [0, 0, 0, lz4mi.ERR_ARG] + [cross] * (n - 4) and not ln[3:].any()
    assert np.array_equal(out[:3 * BS], data[:3 * BS]) and not out[3 * BS:].any()
    # a slot above the export limit (4 MiB), as the last block
    caps = list(sizes)
    caps[-1] = (4 << 20) + 1
    st, ln, out = _dev(pay, words, zeros, off, caps)
    assert st.tolist() == [0] * (n - 1) + [lz4mi.ERR_ARG]
    assert np.array_equal(out[:(n - 1) * BS], data[:(n - 1) * BS]) and not out[(n - 1) * BS:].any()
    # host pointers: the call is refused
    with pytest.raises(lz4mi.Lz4miError) as ei:
        lz4mi.decompress_blocks(pay, caps, linked=True)
    assert ei.value.status == lz4mi.ERR_ARG
    # the reference modes are not linked in this version
    L = lz4mi.lib()
    for flag in (lz4mi.JS_EXACT, lz4mi.JS_COMPAT):
        r = L.lz4mi_decompress_blocks(None, None, None, None, None, None, None, 0, None, None, 0,
                                      lz4mi.LINKED | flag | lz4mi.DEVICE_PTRS, None)
        assert r == lz4mi.ERR_ARG
    assert L.lz4mi_decompress_blocks(None, None, None, None, None, None, None, 0, None, None, 0,
                                     lz4mi.LINKED | lz4mi.DEVICE_PTRS, None) == lz4mi.OK


# ---- frames ----------------------------------------------------------------------------------
def test_frames_linked_routes():
    torch = pytest.importorskip("torch")
    from lz4mi import frame as F
    data = np.concatenate([O.generate("tiles216", 31, 900000), O.generate("random", 32, 300000),
                           O.generate("text", 33, 500000), O.generate("repetitive", 34, 77777)])
    cases = [(65536, True, True, False), (262144, False, True, False), (1048576, True, False, True),
             (4194304, True, True, False), (65536, False, False, True)]
    for bs, indep, cs, bcs in cases:
        for sized in (True, False):
            f = O.compress_frame(data, None, bs, indep, cs, sized, block_checksum=bcs)
            est, eo = O.decompress_frame(f, verify_checksum=False)
            assert est == 0 and np.array_equal(eo, data)
            dev = torch.from_numpy(f.copy()).cuda()
            rep = {}
            got = F.decompress_frame_device(dev, verify_checksum=cs, report=rep, linked=True)
            assert rep["route"] == ("layout" if sized else "linked"), (bs, indep, sized, rep)
            assert np.array_equal(got.cpu().numpy(), eo), (bs, indep, cs, bcs, sized)
            # reference mode ignores the flag: route and bytes as without it
            r0, r1 = {}, {}
            try:
                a = F.decompress_frame_device(dev, js_exact=True, verify_checksum=cs, report=r0).cpu().numpy()
            except lz4mi.Lz4miError as e:
                a = e.status
            try:
                b = F.decompress_frame_device(dev, js_exact=True, verify_checksum=cs, report=r1, linked=True).cpu().numpy()
            except lz4mi.Lz4miError as e:
                b = e.status
            assert r0 == r1 and np.array_equal(a, b), (bs, indep, sized)
    # a corrupted content checksum, on both linked routes
    for sized in (True, False):
        f = O.compress_frame(data, None, 65536, False, True, sized)
        f[-1] ^= 0x55
        with pytest.raises(lz4mi.Lz4miError) as ei:
            F.decompress_frame_device(torch.from_numpy(f.copy()).cuda(), linked=True)
        assert ei.value.status == lz4mi.ERR_CHECKSUM
    # lz4mi_frame_decompress: LINKED | JS_EXACT is refused
    info = np.zeros(8, dtype=np.int64)
    r = lz4mi.lib().lz4mi_frame_decompress(dev.data_ptr(), dev.numel(), dev.data_ptr(), 0, info.ctypes.data,
                                           lz4mi.DEVICE_PTRS | lz4mi.LINKED | lz4mi.JS_EXACT, None)
    assert r == lz4mi.ERR_ARG


# ---- fuzz ------------------------------------------------------------------------------------
def test_seeded_fuzz(monkeypatch):
    """200 batches of 2-12 dependent blocks of 1..70 000 bytes over the generators (one table carried
    along a buffer that mixes them), every eighth with one corrupted byte, every third cut into
    windows of 1-4 blocks: statuses, lengths and bytes == the oracle's decoder in index order."""
    rng = np.random.default_rng(20240)
    kinds = ("tiles216", "text", "repetitive", "copy", "runs", "random")
    for t in range(200):
        nb = int(rng.integers(2, 13))
        sizes = [int(rng.integers(1, 70001)) if rng.random() < 0.7 else int(rng.integers(1, 3000)) for _ in range(nb)]
        total = sum(sizes)
        parts, have = [], 0
        while have < total:
            n = int(rng.integers(1000, 90000))
            parts.append(O.generate(kinds[int(rng.integers(0, len(kinds)))], int(rng.integers(1, 50)), n))
            have += n
        data = np.concatenate(parts)[:total]
        table = np.zeros(16384, dtype=np.int32)
        pay, pos = [], 0
        for n in sizes:
            w, out, table = O.compress_block(data, pos, n, table)
            pay.append(out[:w].copy())
            pos += n
        if t % 8 == 7:
            b = int(rng.integers(0, nb))
            pay[b][int(rng.integers(0, pay[b].size))] = int(rng.integers(0, 256))
        est, eln, eout = _in_order(pay, sizes)
        if t % 8 != 7:
            assert not any(est) and np.array_equal(eout, data)
        if t % 3 == 2:
            monkeypatch.setenv("LZ4MI_LINKED_WINDOW", str(int(rng.integers(1, 5))))
        else:
            monkeypatch.delenv("LZ4MI_LINKED_WINDOW", raising=False)
        st, outs, lens = lz4mi.decompress_blocks(pay, sizes, linked=True)
        assert [int(x) for x in st] == est, (t, st, est)
        assert [int(x) for x in lens] == eln, (t, lens, eln)
        pos = 0
        for b, n in enumerate(sizes):
            if est[b] == 0:
                assert np.array_equal(outs[b], eout[pos:pos + min(eln[b], n)]), (t, b)
            pos += n
