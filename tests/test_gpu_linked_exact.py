"""Linked batches in the reference decoder's bytes (LZ4MI_LINKED_EXACT, include/lz4mi.h; kernels:
csrc/lz4mi_expand.hip "linked reference mode"; argument: DESIGN §4.8). The expected value is always
the oracle's reference-mode decoder (js_compat) run on the blocks in index order on one array
(linked_exact_common.in_order) or the fixture recorded from the reference itself
(tests/golden/linked_exact.json; tests/test_linked_exact_cpu.py pins the one to the other)."""
import ctypes

import numpy as np
import pytest

import oracle as O
from linked_exact_common import dependent_blocks, fixture_cases, in_order, parse

lz4mi = pytest.importorskip("lz4mi")
from lz4mi import shard  # noqa: E402

pytestmark = pytest.mark.gpu

BS = 65536
CROSS = lz4mi.ERR_CROSS_BLOCK


@pytest.fixture(scope="module", autouse=True)
def _device():
    lz4mi.init(0)


def _sizes(total, bs):
    return [min(bs, total - p) for p in range(0, total, bs)]


def _offsets(sizes):
    return np.cumsum([0] + list(sizes[:-1])).tolist()


def _blocks_of(frame):
    _, blocks = shard.frame_blocks(frame)
    return [frame[p:p + n].copy() for p, n, _ in blocks], [s for _, _, s in blocks]


def _host(pay, out_off, out_cap, init, dictionary=None, flags=None):
    """One host-pointer call on a copy of `init` -> (status, out_len, array); raises on a call error."""
    src, in_off, in_len = lz4mi._pack([lz4mi._u8(p) for p in pay])
    n = len(pay)
    out = np.array(init, dtype=np.uint8, copy=True)
    ooff, ocap = np.asarray(out_off, dtype=np.uint64), np.asarray(out_cap, dtype=np.uint32)
    ln, st = np.full(n, 77, dtype=np.uint32), np.full(n, 77, dtype=np.int32)
    d = lz4mi._u8(dictionary)
    lz4mi._check(lz4mi.lib().lz4mi_decompress_blocks(
        lz4mi._p(src), lz4mi._p(in_off), lz4mi._p(in_len), lz4mi._p(out), lz4mi._p(ooff), lz4mi._p(ocap), lz4mi._p(d),
        0 if d is None else d.size, lz4mi._p(ln), lz4mi._p(st), n, lz4mi.LINKED_EXACT if flags is None else flags, None))
    return st.tolist(), ln.tolist(), out


def _dev(pay, words, init, out_off, out_cap, dictionary=None, frame_words=False, linked="exact", js_exact=False):
    """One device-pointer call on torch tensors -> (status, out_len, array)."""
    import torch
    src, in_off, _ = lz4mi._pack([lz4mi._u8(p) for p in pay])
    t = lambda a, dt: torch.from_numpy(np.asarray(a).astype(dt)).cuda()
    d_in, d_ioff = t(src, np.uint8), t(in_off, np.int64)
    d_w = t(np.asarray(words, dtype=np.uint32).view(np.int32), np.int32)
    d_out, d_ooff, d_cap = t(init, np.uint8), t(out_off, np.int64), t(out_cap, np.int32)
    d_len = torch.full((len(pay),), 77, dtype=torch.int32, device="cuda")
    d_st = torch.full((len(pay),), 77, dtype=torch.int32, device="cuda")
    d_dict = None if dictionary is None else t(dictionary, np.uint8)
    lz4mi.decompress_blocks_dev(d_in.data_ptr(), d_ioff.data_ptr(), d_w.data_ptr(), d_out.data_ptr(), d_ooff.data_ptr(),
                                d_cap.data_ptr(), d_len.data_ptr(), d_st.data_ptr(), len(pay),
                                torch.cuda.current_stream().cuda_stream,
                                dict_ptr=None if d_dict is None else d_dict.data_ptr(),
                                dict_len=0 if d_dict is None else d_dict.numel(), frame_words=frame_words,
                                linked=linked, js_exact=js_exact)
    torch.cuda.synchronize()
    return d_st.cpu().numpy().tolist(), d_len.cpu().numpy().tolist(), d_out.cpu().numpy()


def _resumed(call, alone, n, init):
    """The caller's side of a refusal: linked calls from the first undecoded block on; a block that
    gets ERR_CROSS_BLOCK as the first status of a call is decoded alone in reference mode and the
    next call starts behind it. -> (statuses, lengths, array, refused blocks)."""
    arr, first, st, ln, refused = init, 0, [], [], []
    while first < n:
        s, l, arr = call(first, arr)
        bad = [k for k, v in enumerate(s) if v != 0]
        if not bad or s[bad[0]] != CROSS:
            return st + s, ln + l, arr, refused
        k = bad[0]
        assert all(v == CROSS for v in s[k:]) and not any(l[k:])
        st += s[:k]
        ln += l[:k]
        refused.append(first + k)
        s1, l1, arr = alone(first + k, arr)
        st.append(s1)
        ln.append(l1)
        if s1 != 0:
            return st + [CROSS] * (n - len(st)), ln + [0] * (n - len(ln)), arr, refused
        first += k + 1
    return st, ln, arr, refused


def _host_resumed(pay, off, cap, init, dictionary=None):
    def alone(b, arr):
        arr = arr.copy()
        try:
            return 0, lz4mi.decompress_raw(pay[b], 0, pay[b].size, arr[:off[b] + cap[b]], off[b], dictionary=dictionary,
                                           js_exact=True), arr
        except lz4mi.Lz4miError as e:
            return e.status, 0, arr
    return _resumed(lambda f, arr: _host(pay[f:], off[f:], cap[f:], arr, dictionary), alone, len(pay), init)


def _dev_resumed(pay, words, off, cap, init, dictionary=None):
    def alone(b, arr):
        s, l, arr = _dev([pay[b]], [words[b]], arr, [off[b]], [cap[b]], dictionary, True, linked=False, js_exact=True)
        return s[0], l[0], arr
    return _resumed(lambda f, arr: _dev(pay[f:], words[f:], arr, off[f:], cap[f:], dictionary, True), alone, len(pay), init)


# ---- 1. the smallest real shape --------------------------------------------------------------
@pytest.fixture(scope="module")
def case1():
    data = O.generate("text", 33, 300000)
    sizes = _sizes(data.size, BS)
    pay, stored = _blocks_of(O.compress_frame(data, None, BS, False, False, True))
    assert not any(stored) and len(pay) == 5
    off = _offsets(sizes)
    zeros = np.zeros(data.size, dtype=np.uint8)
    st, ln, want = in_order(pay, off, sizes, zeros)
    assert not any(st) and ln == sizes
    return {"data": data, "pay": pay, "sizes": sizes, "off": off, "zeros": zeros, "want": want}


def test_smallest_real_shape(case1):
    pytest.importorskip("torch")
    c = case1
    assert int((c["want"] != c["data"]).sum()) > 1000          # the reference's result is not the input
    hits = 0
    for b in range(1, 5):
        before = in_order(c["pay"], c["off"], c["sizes"], c["zeros"], count=b)[2]
        hits += int(not np.array_equal(before[c["off"][b] - 4:c["off"][b]], c["want"][c["off"][b] - 4:c["off"][b]]))
    assert hits >= 1                                           # a block changes its predecessor's last 4 bytes
    for sizes in (c["sizes"], None):                            # host pointers, given and measured sizes
        st, outs, lens = lz4mi.decompress_blocks(c["pay"], sizes, linked="exact")
        assert not st.any() and [int(x) for x in lens] == c["sizes"]
        assert np.array_equal(np.concatenate(outs), c["want"])
    st, ln, out = _dev(c["pay"], [p.size for p in c["pay"]], c["zeros"], c["off"], c["sizes"])
    assert not any(st) and ln == c["sizes"] and np.array_equal(out, c["want"])
    # LZ4MI_LINKED beside the flag changes nothing
    st, ln, out = _host(c["pay"], c["off"], c["sizes"], c["zeros"], flags=lz4mi.LINKED | lz4mi.LINKED_EXACT)
    assert not any(st) and np.array_equal(out, c["want"])
    # a spec-mode linked decode is not what the reference returns
    st, outs, _ = lz4mi.decompress_blocks(c["pay"], c["sizes"], linked=True)
    assert not st.any() and np.array_equal(np.concatenate(outs), c["data"])


# ---- 2. golden frames ------------------------------------------------------------------------
def test_golden_frames(manifest):
    torch = pytest.importorskip("torch")
    from conftest import cases_of, golden_bytes
    from lz4mi import frame as F
    (g,) = cases_of(manifest, "frames")
    inputs = {"text": ("text", 5, 300000), "copy": ("copy", 6, 150000)}
    seen = set()
    for f in g["frames"]:
        if (f["input"] not in inputs or f["block"] != BS or f["indep"] or f["checksum"] or "dict" in f or "dict_text" in f
                or not f.get("add_size", True) or not f["dec_ok"]):
            continue
        data = O.generate(*inputs[f["input"]])[:f["n"]]
        frame = golden_bytes(f["frame_file"]).copy() if f["frame_file"] else O.compress_frame(data, None, BS, False, False, True)
        assert "%08x" % O.xxh32(frame) == f["frame_xxh"]
        dev = torch.from_numpy(frame).cuda()
        rep = {}
        got = F.decompress_frame_device(dev, linked="exact", report=rep).cpu().numpy()
        assert rep["route"] == "layout" and got.size == f["dec_len"]
        assert "%08x" % O.xxh32(got) == f["dec_xxh"], f["input"]
        assert not f["dec_equals_input"] and not np.array_equal(got, data)
        out = torch.zeros(f["n"], dtype=torch.uint8, device="cuda")
        info = lz4mi.frame_decompress_dev(dev.data_ptr(), dev.numel(), out.data_ptr(), out.numel(),
                                          torch.cuda.current_stream().cuda_stream, linked="exact")
        torch.cuda.synchronize()
        assert info["status"] == 0 and info["written"] == f["n"]
        assert "%08x" % O.xxh32(out.cpu().numpy()) == f["dec_xxh"]
        r0 = {}
        ref = F.decompress_frame_device(dev, js_exact=True, report=r0).cpu().numpy()
        assert np.array_equal(got, ref)
        both = F.decompress_frame_device(dev, js_exact=True, linked="exact", report=rep).cpu().numpy()
        assert rep["route"] == "layout" and np.array_equal(both, got)
        seen.add(f["input"])
    assert seen == {"text", "copy"}


# ---- 3. windows ------------------------------------------------------------------------------
@pytest.mark.parametrize("window", [1, 3, None])
def test_windows(case1, window, monkeypatch):
    """With 1 every block is its window's first: the rewrite below it lands on final bytes."""
    c = case1
    if window:
        monkeypatch.setenv("LZ4MI_LINKED_WINDOW", str(window))
    st, ln, out = _host(c["pay"], c["off"], c["sizes"], c["zeros"])
    assert not any(st) and ln == c["sizes"] and np.array_equal(out, c["want"])


# ---- 4. the fixture --------------------------------------------------------------------------
MAY_REFUSE = {"stored_pred": {2}, "gap": {1}, "short_tail": {1}, "first_at_0_dict": {0}}
CASES = fixture_cases()


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_fixture_cases(case):
    pytest.importorskip("torch")
    c = case
    want_st = [0] * len(c["blocks"])
    words = [b.size | (0x80000000 if s else 0) for b, s in zip(c["blocks"], c["stored"])]
    st, ln, out, refused = _dev_resumed(c["blocks"], words, c["out_off"], c["out_cap"], c["init"], c["dict"])
    assert st == want_st and ln == c["results"], (st, ln)
    assert set(refused) <= MAY_REFUSE.get(c["name"], set()), refused
    assert np.array_equal(out, c["after"])
    if not any(c["stored"]):
        st, ln, out, refused = _host_resumed(c["blocks"], c["out_off"], c["out_cap"], c["init"], c["dict"])
        assert st == want_st and ln == c["results"], (st, ln)
        assert set(refused) <= MAY_REFUSE.get(c["name"], set()), refused
        assert np.array_equal(out, c["after"])


# ---- 5. the failure rule ---------------------------------------------------------------------
def _first_offset_pos(c):
    lp, ll, _, _ = parse(c)[0]
    return lp + ll


@pytest.mark.parametrize("how", ["truncated", "offset0"])
@pytest.mark.parametrize("window", [None, 2])
def test_failure_rule(case1, how, window, monkeypatch):
    pytest.importorskip("torch")
    c = case1
    bad = [p.copy() for p in c["pay"]]
    if how == "truncated":
        bad[2] = bad[2][:bad[2].size - 9].copy()
    else:
        q = _first_offset_pos(bad[2])
        bad[2][q] = bad[2][q + 1] = 0
    est, eln, want = in_order(bad, c["off"], c["sizes"], c["zeros"])
    assert est[:2] == [0, 0] and est[2] in (lz4mi.ERR_MALFORMED, lz4mi.ERR_OFFSET0, lz4mi.ERR_OUTPUT_TOO_SMALL)
    assert est[3:] == [CROSS, CROSS]
    # blocks 0-1 as decoded alone in order; nothing from block 2 on, the predecessor's tail included
    assert np.array_equal(want, in_order(bad, c["off"], c["sizes"], c["zeros"], count=2)[2])
    assert not want[c["off"][2]:].any()
    if window:
        monkeypatch.setenv("LZ4MI_LINKED_WINDOW", str(window))
    st, ln, out = _host(bad, c["off"], c["sizes"], c["zeros"])
    assert st == est and ln == eln and np.array_equal(out, want)
    st, ln, out = _dev(bad, [p.size for p in bad], c["zeros"], c["off"], c["sizes"])
    assert st == est and ln == eln and np.array_equal(out, want)


# ---- 6. independent blocks -------------------------------------------------------------------
def test_independent_blocks():
    srcs = [O.generate("copy", 61 + k, 300000) for k in range(3)]
    comps = [O.compress_block_bytes(s) for s in srcs]
    sizes = [s.size for s in srcs]
    st0, outs0, lens0 = lz4mi.decompress_blocks(comps, sizes, js_exact=True)
    st1, outs1, lens1 = lz4mi.decompress_blocks(comps, sizes, linked="exact")
    assert not st0.any() and not st1.any() and np.array_equal(lens0, lens1)
    assert any(not np.array_equal(a, s) for a, s in zip(outs0, srcs))   # (the rewrite does change copy)
    for a, b in zip(outs0, outs1):
        assert np.array_equal(a, b)


# ---- 7. 4 MiB blocks -------------------------------------------------------------------------
def test_four_mib_blocks():
    data = O.generate("text", 71, 2 * (4 << 20))
    pay, stored = _blocks_of(O.compress_frame(data, None, 4 << 20, False, False, True))
    assert len(pay) == 2 and not any(stored)
    sizes = [4 << 20] * 2
    st, ln, want = in_order(pay, [0, 4 << 20], sizes, np.zeros(data.size, dtype=np.uint8))
    assert not any(st) and not np.array_equal(want, data)
    st, outs, lens = lz4mi.decompress_blocks(pay, sizes, linked="exact")
    assert not st.any() and [int(x) for x in lens] == sizes and np.array_equal(np.concatenate(outs), want)


# ---- 8. scratch allocation failure -----------------------------------------------------------
def test_scratch_allocation_failure(case1, monkeypatch):
    """The window scratch cannot be allocated (the hook asks for a petabyte more): one block per
    launch in reference mode, the same bytes."""
    c = case1
    monkeypatch.setenv("LZ4MI_TEST_SCRATCH_EXTRA_MB", str(1 << 30))
    st, ln, out = _host(c["pay"], c["off"], c["sizes"], c["zeros"])
    assert not any(st) and ln == c["sizes"] and np.array_equal(out, c["want"])
    stats = (ctypes.c_ulonglong * 4)()
    lz4mi.lib().lz4mi_debug_linked_stats(stats)
    assert stats[0] == 0                                       # no window ran
    monkeypatch.delenv("LZ4MI_TEST_SCRATCH_EXTRA_MB")
    st, ln, out = _host(c["pay"], c["off"], c["sizes"], c["zeros"])
    assert not any(st) and np.array_equal(out, c["want"])
    lz4mi.lib().lz4mi_debug_linked_stats(stats)
    assert stats[0] == 1


# ---- 9. refusals -----------------------------------------------------------------------------
def test_refusals(case1):
    torch = pytest.importorskip("torch")
    c = case1
    L = lz4mi.lib()
    for flag in (lz4mi.JS_EXACT, lz4mi.JS_COMPAT):
        for lk in (0, lz4mi.LINKED):
            r = L.lz4mi_decompress_blocks(None, None, None, None, None, None, None, 0, None, None, 0,
                                          lz4mi.LINKED_EXACT | lk | flag | lz4mi.DEVICE_PTRS, None)
            assert r == lz4mi.ERR_ARG
    assert L.lz4mi_decompress_blocks(None, None, None, None, None, None, None, 0, None, None, 0,
                                     lz4mi.LINKED_EXACT | lz4mi.DEVICE_PTRS, None) == lz4mi.OK
    caps = list(c["sizes"])
    caps[-1] = (4 << 20) + 1
    with pytest.raises(lz4mi.Lz4miError) as ei:
        lz4mi.decompress_blocks(c["pay"], caps, linked="exact")
    assert ei.value.status == lz4mi.ERR_ARG
    big = np.zeros(c["data"].size + (8 << 20), dtype=np.uint8)
    st, ln, out = _dev(c["pay"], [p.size for p in c["pay"]], big, c["off"], caps)
    four = in_order(c["pay"], c["off"], c["sizes"], c["zeros"], count=4)[2]   # (block 4 rewrites nothing either)
    assert st == [0] * 4 + [lz4mi.ERR_ARG] and np.array_equal(out[:c["data"].size], four)
    assert not out[c["off"][4]:].any()
    # a mixed frame: text, one random (stored) block, text -- through lz4mi_frame_decompress
    data = np.concatenate([O.generate("text", 91, 3 * BS), O.generate("random", 92, BS), O.generate("text", 93, 3 * BS + 777)])
    frame = O.compress_frame(data, None, BS, False, False, True)
    stored = _blocks_of(frame)[1]
    assert sum(stored) == 1 and stored[3]
    est, want = O.decompress_frame(frame, verify_checksum=False, js_compat=True)
    assert est == 0 and not np.array_equal(want, data)
    dev = torch.from_numpy(frame).cuda()
    out = torch.zeros(data.size, dtype=torch.uint8, device="cuda")
    info = np.zeros(8, dtype=np.int64)
    for flag in (lz4mi.JS_EXACT, lz4mi.JS_EXACT | lz4mi.LINKED):
        r = L.lz4mi_frame_decompress(dev.data_ptr(), dev.numel(), out.data_ptr(), out.numel(), info.ctypes.data,
                                     lz4mi.DEVICE_PTRS | lz4mi.LINKED_EXACT | flag, None)
        assert r == lz4mi.ERR_ARG
    inf = lz4mi.frame_decompress_dev(dev.data_ptr(), dev.numel(), out.data_ptr(), out.numel(),
                                     torch.cuda.current_stream().cuda_stream, linked="exact")
    torch.cuda.synchronize()
    assert inf["status"] == 0 and inf["written"] == data.size and inf["stored_blocks"] == 1
    assert np.array_equal(out.cpu().numpy(), want)
    L.lz4mi_debug_linked_resumes.restype = ctypes.c_ulonglong
    assert L.lz4mi_debug_linked_resumes() <= 1                 # at most one resume per stored block


# ---- 10. fuzz --------------------------------------------------------------------------------
def _refusal_allowed(pay, off, eln, b, ws):
    """The contract's case 3: block b is not the first of its window (which starts at block ws) and
    its region below its start touches a byte that is not decoded output of an earlier block of
    that window (the unused tail of a short predecessor; behind tiny blocks, the window before)."""
    if b == ws:
        return False
    _, ll, o, ml = parse(pay[b])[0]
    if o < 8 or ml >= 8 or ll + ml >= 8:
        return False
    for a in range(max(0, off[b] - (8 - ml - ll)), off[b]):
        p = max(k for k in range(b) if off[k] <= a)
        if p < ws or a - off[p] >= eln[p]:
            return True
    return False


def test_seeded_fuzz(monkeypatch):
    """100 batches of 2-12 dependent blocks of 1..70 000 bytes over the six generators with one
    carried table; every eighth with one corrupted byte, every third cut into windows of 1-4.
    Statuses, lengths and the whole array == the oracle in index order; a refusal is accepted only
    where the contract allows one, and then resumed. Every batch is compared."""
    rng = np.random.default_rng(20248)
    kinds = ("tiles216", "text", "repetitive", "copy", "runs", "random")
    compared = 0
    for t in range(100):
        nb = int(rng.integers(2, 13))
        sizes = [int(rng.integers(1, 70001)) if rng.random() < 0.7 else int(rng.integers(1, 3000)) for _ in range(nb)]
        total = sum(sizes)
        parts, have = [], 0
        while have < total:
            n = int(rng.integers(1000, 90000))
            parts.append(O.generate(kinds[int(rng.integers(0, len(kinds)))], int(rng.integers(1, 50)), n))
            have += n
        data = np.concatenate(parts)[:total]
        pay = dependent_blocks(data, sizes)
        if t % 8 == 7:
            b = int(rng.integers(0, nb))
            pay[b][int(rng.integers(0, pay[b].size))] = int(rng.integers(0, 256))
        off = _offsets(sizes)
        zeros = np.zeros(total, dtype=np.uint8)
        est, eln, want = in_order(pay, off, sizes, zeros)
        window = int(rng.integers(1, 5)) if t % 3 == 2 else 0
        if window:
            monkeypatch.setenv("LZ4MI_LINKED_WINDOW", str(window))
        else:
            monkeypatch.delenv("LZ4MI_LINKED_WINDOW", raising=False)
        starts = []

        def call(f, arr):
            starts.append(f)
            return _host(pay[f:], off[f:], sizes[f:], arr)

        def alone(b, arr):
            arr = arr.copy()
            try:
                return 0, lz4mi.decompress_raw(pay[b], 0, pay[b].size, arr[:off[b] + sizes[b]], off[b], js_exact=True), arr
            except lz4mi.Lz4miError as e:
                return e.status, 0, arr
        st, ln, out, refused = _resumed(call, alone, nb, zeros)
        for b in refused:
            f = max(s for s in starts if s <= b)                # the call, then the window, that held block b
            ws = f + (b - f) // window * window if window else f
            assert est[b] == 0 and _refusal_allowed(pay, off, eln, b, ws), (t, b)
        assert st == est, (t, st, est)
        assert ln == eln, (t, ln, eln)
        assert np.array_equal(out, want), t
        compared += 1
    assert compared == 100
