"""The built rewrite shapes of tests/rewrite_shapes_common.py through every decoder route: status, out_len and
the WHOLE array against the CPU oracle. The routes are selected by the documented dispatch rules
(csrc/lz4mi_capi.cpp decode_launch, csrc/lz4mi_decompress.hip x_enter):

  lone, small path        one block within the export limits: the segment-parallel parse and the pointer pass
                          (lz4mi_xf1ptr_kernel); a rewrite that writes below the slot, or reads below the array
                          with a dictionary, sends the block back to the batch kernel through redo[];
  lone, one wave          the same calls with a capacity of 4 MiB + 1, past the export limit: one wave of the
                          same launch decodes the block as the batch kernel does (step 7: f1_table, f1_fixup,
                          cut_match), not isolated: it reads the history and the dictionary;
  small batch, isolated   3 shapes and every shape in one call: the pointer pass with isolate set;
  batch kernel, isolated  more than SMALL_BLOCKS + 8 blocks: lz4mi_decompress_kernel, one wave per block;
  serial kernel           LZ4MI_JS_COMPAT, one lane in order;
  re-parse modes          the segment family with LZ4MI_SMALL_REPARSE = 0, 1, 2;
  linked exact            a literal-only block that holds the history, then the shape (LZ4MI_LINKED_EXACT:
                          lz4mi_xf1ptr_linked_kernel).

Device arrays lie inside sentinel margins, which must come back untouched."""
import functools

import numpy as np
import pytest

import rewrite_shapes_common as X
from test_gpu_seqtable import encode

MARGIN = 4096
SENT = 0xC3               # the margins around every device array
FILL = 0x5A               # the slots before a call
EXTRA = 8                 # sentinel entries behind status[] and out_len[]
BIG = (4 << 20) + 1       # past the small path's export limit (kSmallOutMax)


def _flags(lz4mi, mode, linked=False):
    if linked:
        return lz4mi.LINKED_EXACT
    return {"spec": 0, "reference": lz4mi.JS_EXACT, "serial": lz4mi.JS_COMPAT}[mode]


def _pack(blocks):
    lens = np.array([b.size for b in blocks], dtype=np.uint32)
    offs = np.zeros(len(blocks), dtype=np.uint64)
    offs[1:] = np.cumsum(lens[:-1].astype(np.uint64))
    return np.concatenate(blocks), offs, lens


def host_call(lz4mi, blocks, offs, caps, arr, dictionary, flags):
    """One lz4mi_decompress_blocks call with host pointers on `arr` (changed in place) -> (statuses, lengths)."""
    src, in_off, in_len = _pack(blocks)
    n = len(blocks)
    o_off, o_cap = np.array(offs, dtype=np.uint64), np.array(caps, dtype=np.uint32)
    out_len, status = np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.int32)
    d = dictionary
    rc = lz4mi.lib().lz4mi_decompress_blocks(src.ctypes.data, in_off.ctypes.data, in_len.ctypes.data, arr.ctypes.data,
                                             o_off.ctypes.data, o_cap.ctypes.data, None if d is None else d.ctypes.data,
                                             0 if d is None else d.size, out_len.ctypes.data, status.ctypes.data, n, flags, None)
    assert rc == 0, rc
    return [int(x) for x in status], [int(x) for x in out_len]


def dev_call(lz4mi, blocks, offs, caps, arr, dictionary, flags):
    """The same call with device pointers: every array inside margins of SENT, which are checked; `arr` is
    replaced by what the device holds afterwards -> (statuses, lengths)."""
    import torch
    src, in_off, in_len = _pack(blocks)
    n = len(blocks)

    def padded(a):
        p = np.full(a.size + 2 * MARGIN, SENT, dtype=np.uint8)
        p[MARGIN:MARGIN + a.size] = a
        return torch.from_numpy(p).cuda()

    t = lambda a, dt: torch.from_numpy(np.asarray(a).astype(dt)).cuda()
    d_out, d_in = padded(arr), padded(src)
    d_dict = None if dictionary is None else padded(dictionary)
    d_ioff, d_ilen = t(in_off, np.int64), t(in_len.view(np.int32), np.int32)
    d_ooff, d_cap = t(offs, np.int64), t(np.array(caps, dtype=np.uint32).view(np.int32), np.int32)
    d_len = torch.full((n + EXTRA,), 77, dtype=torch.int32, device="cuda")
    d_st = torch.full((n + EXTRA,), 77, dtype=torch.int32, device="cuda")
    rc = lz4mi.lib().lz4mi_decompress_blocks(d_in.data_ptr() + MARGIN, d_ioff.data_ptr(), d_ilen.data_ptr(),
                                             d_out.data_ptr() + MARGIN, d_ooff.data_ptr(), d_cap.data_ptr(),
                                             None if d_dict is None else d_dict.data_ptr() + MARGIN,
                                             0 if dictionary is None else dictionary.size, d_len.data_ptr(), d_st.data_ptr(),
                                             n, flags | lz4mi.DEVICE_PTRS, torch.cuda.current_stream().cuda_stream)
    assert rc == 0, rc
    torch.cuda.synchronize()
    got = d_out.cpu().numpy()
    assert (got[:MARGIN] == SENT).all() and (got[MARGIN + arr.size:] == SENT).all(), "the margins around the output changed"
    assert np.array_equal(d_in.cpu().numpy()[MARGIN:MARGIN + src.size], src), "the input changed"
    st, ln = d_st.cpu().numpy(), d_len.cpu().numpy().view(np.uint32)
    assert (st[n:] == 77).all() and (ln[n:] == 77).all(), "entries behind status[] / out_len[] were written"
    arr[:] = got[MARGIN:MARGIN + arr.size]
    return [int(x) for x in st[:n]], [int(x) for x in ln[:n]]


CALLS = {"host": host_call, "device": dev_call}


def check_lone(lz4mi, call, s, mode, cap=None):
    """The shape alone on its array (the history, then the slot) against the oracle alone."""
    exact = mode != "spec"
    cap = s.cap if cap is None else cap
    # (the 4 MiB arrays of the raised capacity are not kept: the cache's function itself)
    est, ew, want = (X.expected if cap == s.cap else X.expected.__wrapped__)(s.name, exact, cap, FILL)
    arr = X.array_for(s, cap, FILL)
    h = X.out_off(s)
    (st,), (n,) = call(lz4mi, [s.comp], [h], [cap], arr, s.dictionary, _flags(lz4mi, mode))
    what = (s.name, mode, call.__name__, cap)
    assert st == est, (what, "status", st, est)
    if est == 0:
        bad = np.nonzero(arr != want)[0]
        assert n == ew and bad.size == 0, (what, n, ew, f"{bad.size} bytes differ, first at {int(bad[0]) if bad.size else None}"
                                           f" (slot at {h})")
    else:                                   # a failing block: nothing outside its slot changes
        assert n == 0 and np.array_equal(arr[:h], X.array_for(s, cap, FILL)[:h]), what
    if h:                                   # with history only [out_off - 4, out_off) may differ from it
        assert np.array_equal(arr[:h - 4], s.history[:h - 4]), what


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["spec", "reference"])
@pytest.mark.parametrize("ptrs", ["host", "device"])
def test_lone_small_path(ptrs, mode):
    lz4mi = pytest.importorskip("lz4mi")
    lz4mi.init(0)
    X.claims()
    for s in X.shapes():
        check_lone(lz4mi, CALLS[ptrs], s, mode)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["spec", "reference"])
@pytest.mark.parametrize("ptrs", ["host", "device"])
def test_lone_one_wave_not_isolated(ptrs, mode):
    lz4mi = pytest.importorskip("lz4mi")
    lz4mi.init(0)
    for s in X.shapes():
        if not s.says.get("clip"):          # (raising the capacity undoes the clip)
            check_lone(lz4mi, CALLS[ptrs], s, mode, BIG)


@pytest.mark.gpu
@pytest.mark.parametrize("ptrs", ["host", "device"])
def test_serial_kernel(ptrs):
    lz4mi = pytest.importorskip("lz4mi")
    lz4mi.init(0)
    for s in X.shapes():
        check_lone(lz4mi, CALLS[ptrs], s, "serial")


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["spec", "reference"])
@pytest.mark.parametrize("reparse", ["0", "1", "2"])
def test_reparse_modes(reparse, mode, monkeypatch):
    """The segment family with every guess kept, and with the re-parses forced (the hook is read per call)."""
    lz4mi = pytest.importorskip("lz4mi")
    lz4mi.init(0)
    monkeypatch.setenv("LZ4MI_SMALL_REPARSE", reparse)
    fam = X.by_family("segment")
    assert len(fam) == 6
    for s in fam:
        check_lone(lz4mi, host_call, s, mode)
        check_lone(lz4mi, dev_call, s, mode)


# ------------------------------------------------------------------------------------------- isolated batches
@functools.lru_cache(maxsize=None)
def independent():
    """The shapes without history or dictionary."""
    X.claims()
    return tuple(s for s in X.shapes() if s.history is None and s.dictionary is None)


def check_batch(lz4mi, call, picks, mode):
    """`picks` in one call, each slot behind a gap of 13 + its index bytes: a shape whose `isolated` is 0 matches
    the oracle byte for byte, one whose `isolated` is ERR_CROSS_BLOCK reports exactly that with out_len 0;
    nothing between the slots changes."""
    exact = mode == "reference"
    offs, at = [], 0
    for j, s in enumerate(picks):
        at += 13 + j % 7
        offs.append(at)
        at += s.cap
    arr = np.full(at + 16, FILL, dtype=np.uint8)
    want, care = arr.copy(), np.ones(arr.size, dtype=bool)
    est, elen = [], []
    for s, off in zip(picks, offs):
        iso = X.isolated(s, exact)
        assert iso in (0, X.CROSS), s.name
        est.append(iso)
        if iso == 0:
            st, w, one = X.expected(s.name, exact, None, FILL)
            assert st == 0, s.name
            want[off:off + s.cap] = one
            elen.append(w)
        else:
            care[off:off + s.cap] = False
            elen.append(0)
    st, ln = call(lz4mi, [s.comp for s in picks], offs, [s.cap for s in picks], arr, None, _flags(lz4mi, mode))
    for j, s in enumerate(picks):
        assert st[j] == est[j] and ln[j] == elen[j], (s.name, j, mode, call.__name__, st[j], est[j], ln[j], elen[j])
    bad = np.nonzero((arr != want) & care)[0]
    if bad.size:
        p = int(bad[0])
        j = max(k for k in range(len(offs)) if offs[k] - 13 - k % 7 <= p)
        raise AssertionError((picks[j].name, j, mode, call.__name__, f"{bad.size} bytes differ, first at {p} (slot at {offs[j]})"))
    return est


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["spec", "reference"])
def test_small_batch_isolated(mode):
    lz4mi = pytest.importorskip("lz4mi")
    lz4mi.init(0)
    ind = independent()
    assert 3 < len(ind) <= lz4mi.SMALL_BLOCKS
    three = [next(s for s in ind if s.name == n) for n in ("chain_ml4_depth3", "cond_below_a", "cut_run_1100_ml4")]
    assert check_batch(lz4mi, dev_call, three, mode) == [0, X.CROSS if mode == "reference" else 0, 0]
    est = check_batch(lz4mi, host_call, list(ind), mode)
    assert 2 * est.count(0) > len(est)
    check_batch(lz4mi, dev_call, list(ind), mode)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["spec", "reference"])
def test_batch_kernel_isolated(mode):
    lz4mi = pytest.importorskip("lz4mi")
    lz4mi.init(0)
    ind = list(independent())
    picks = ind * (-(-(lz4mi.SMALL_BLOCKS + 9) // len(ind)))
    assert len(picks) > lz4mi.SMALL_BLOCKS + 8
    check_batch(lz4mi, host_call, picks, mode)
    check_batch(lz4mi, dev_call, picks, mode)


# ----------------------------------------------------------------------------------------------- linked exact
@pytest.mark.gpu
@pytest.mark.parametrize("ptrs", ["host", "device"])
def test_linked_exact(ptrs):
    """A literal-only block that holds the history, then the shape: the oracle's two decodes in order on one
    array; both statuses 0."""
    lz4mi = pytest.importorskip("lz4mi")
    lz4mi.init(0)
    fam = X.by_family("history")
    assert len(fam) == 14
    for s in fam:
        h = X.out_off(s)
        est, ew, want = X.expected(s.name, True, None, FILL)
        assert est == 0
        arr = np.full(h + s.cap, FILL, dtype=np.uint8)
        st, ln = CALLS[ptrs](lz4mi, [encode([], bytes(s.history)), s.comp], [0, h], [h, s.cap], arr, None, _flags(lz4mi, "", True))
        bad = np.nonzero(arr != want)[0]
        assert st == [0, 0] and ln == [h, ew] and bad.size == 0, (s.name, ptrs, st, ln, bad[:4])
