"""Frame decoding of damaged frames on the GPU against the reference decoder's recorded outcomes
(tests/golden/damaged_frames.json; test_damaged_frames_cpu.py pins the oracle to them, so the
expected bytes here are the oracle's).

Every specified case of every base frame goes through decompress_frame_host and the device entry
point (defaults, linked=True, js_exact=True), with verify_checksum both ways; the device runs read
the frame from the start of a larger buffer whose tail is 0x00 in one run and 0xFF in the other
(nothing past the frame's length may matter). The frame kernels are compared with the byte-wise
walk of the reference (damaged_common.walk): lz4mi_frame_index's info words and lists, poisoned
beforehand, at full and at short capacities, and lz4mi_frame_decompress's info words with a
canary behind its output.

Spec mode (js_exact=False). The recorded statuses are the reference's; the expected bytes are the
oracle's spec decode. They differ from the reference's bytes in the frames whose text blocks
decode (double-copy-tail rewrites, SURVEY F1: content A's first block, content B's first two), and
only for those cases, with a content checksum verified, the verdict follows the spec bytes (the
reference fails its own undamaged text frames there): `_expected` takes the status from the
oracle's spec decode exactly when both decodes run to the checksum stage and their bytes differ.
For every other case the recorded status is asserted in both modes."""
import collections
import functools

import numpy as np
import pytest

import damaged_common as D
import oracle as O

lz4mi = pytest.importorskip("lz4mi")
torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

ROUTES = collections.Counter()       # report["route"] of the damaged (not "whole") cases this module decoded
PAD = 4096


@pytest.fixture(scope="module", autouse=True)
def _init():
    lz4mi.init(0)


@functools.lru_cache(maxsize=2)
def _expected(name, verify):
    """Per specified case: (index, kind, frame, (status, bytes) in reference mode, (status, bytes) in spec mode)."""
    res = []
    for k, c, f in D.cases(name):
        want = c["v" if verify else "n"]
        exp = D.expected_status(want)
        if exp == "alloc":
            exp = lz4mi.ERR_RANGE        # the 2^48 content size: refused before any allocation
            js = sp = (exp, None)
        else:
            st_c, out_c = O.decompress_frame(f, verify_checksum=verify, js_compat=True)
            st_s, out_s = O.decompress_frame(f, verify_checksum=verify, js_compat=False)
            assert st_c == exp                                   # (test_damaged_frames_cpu.py)
            js = (exp, out_c if exp == 0 else None)
            stage = (0, lz4mi.ERR_CHECKSUM)
            if st_c in stage and st_s in stage and not np.array_equal(
                    *(O.decompress_frame(f, verify_checksum=False, js_compat=m)[1] for m in (True, False))):
                sp = (st_s, out_s if st_s == 0 else None)        # the F1 cases (module docstring)
            else:
                assert st_s == exp, (name, k, c["k"], st_s, exp)
                sp = (exp, out_c if exp == 0 else None)
        res.append((k, c["k"], f, js, sp))
    return res


def _decode(entry, f, verify, fill, rep):
    from lz4mi import frame as F
    if entry == "host":
        return F.decompress_frame_host(f, verify_checksum=verify)
    if entry == "host_js":
        return F.decompress_frame_host(f, js_exact=True, verify_checksum=verify)
    buf = torch.full((f.size + PAD,), fill, dtype=torch.uint8, device="cuda")
    buf[:f.size] = torch.from_numpy(f.copy()).cuda()
    kw = {"device": {}, "linked": {"linked": True}, "js_exact": {"js_exact": True}}[entry]
    return F.decompress_frame_device(buf[:f.size], verify_checksum=verify, report=rep, **kw).cpu().numpy()


ENTRIES = [("host", 0), ("host_js", 0)] + [(e, fill) for e in ("device", "linked", "js_exact") for fill in (0x00, 0xFF)]


@pytest.mark.parametrize("name,verify,entry,fill", [(n, v, e, fl) for n in D.base_names() for v in (True, False)
                                                    for e, fl in ENTRIES])
def test_every_entry_point_gives_the_reference_outcome(name, verify, entry, fill):
    bad = []
    for k, kind, f, js, sp in _expected(name, verify):
        want_st, want = js if entry in ("host_js", "js_exact") else sp
        rep = {}
        try:
            got = _decode(entry, f, verify, fill, rep)
            st = 0
        except lz4mi.Lz4miError as e:       # (anything else, a torch out-of-memory error included, fails the test)
            if e.status == lz4mi.ERR_HIP:
                raise
            got, st = None, e.status
        if kind != "whole" and "route" in rep:
            ROUTES[rep["route"]] += 1
        if st != want_st or (st == 0 and not np.array_equal(got, want)):
            diff = None
            if st == 0 and want_st == 0 and got.size == want.size:
                at = np.nonzero(got != want)[0]
                diff = (int(at[0]), int(at[-1]), int(at.size))      # first, last, number of differing bytes
            bad.append((k, kind, st, want_st, None if got is None else got.size, None if want is None else want.size,
                        diff, rep.get("route")))
    assert not bad, "%d cases: %r" % (len(bad), bad[:8])


DEFAULT_ROUTE = {"is": "layout", "iu": "measured", "ds": "layout", "du": "host", "isc": "layout", "isb": "layout"}
LINKED_ROUTE = dict(DEFAULT_ROUTE, iu="linked", du="linked")
JS_ROUTE = dict(DEFAULT_ROUTE, iu="host", du="host")


@pytest.mark.parametrize("name", D.base_names())
def test_routes_of_the_undamaged_frames(name):
    from lz4mi import frame as F
    f = D.base_frame(name)
    data = D.base_content(name)
    var = name.split("_")[1]
    d = torch.from_numpy(f.copy()).cuda()
    for kw, table in (({}, DEFAULT_ROUTE), ({"linked": True}, LINKED_ROUTE), ({"js_exact": True}, JS_ROUTE)):
        rep = {}
        got = F.decompress_frame_device(d, verify_checksum=not kw.get("js_exact"), report=rep, **kw)
        assert rep == {"route": "host" if name == "E_iu" else table[var]}, (name, kw)
        if not kw.get("js_exact"):
            assert np.array_equal(got.cpu().numpy(), data)


def test_every_route_decodes_damaged_frames_too():
    """layout, measured, linked and host, each at least once on a damaged frame (counted in ROUTES by
    the entry-point tests as well; the cases here make the test stand on its own)."""
    from lz4mi import frame as F
    for name, kw, kind, route in (("A_is", {}, "garbage", "layout"), ("A_isc", {}, "csum", "layout"),
                                  ("A_iu", {}, "garbage", "measured"), ("B_du", {"linked": True}, "garbage", "linked"),
                                  ("B_iu", {"linked": True}, "hdr_hc", "linked"), ("A_is", {}, "cut_block", "host"),
                                  ("B_du", {}, "hdr_bd", "host")):
        _, c, f = next(x for x in D.cases(name) if x[1]["k"] == kind)
        rep = {}
        try:
            F.decompress_frame_device(torch.from_numpy(f.copy()).cuda(), verify_checksum=False, report=rep, **kw)
        except lz4mi.Lz4miError as e:
            assert e.status != lz4mi.ERR_HIP
        assert rep == {"route": route}, (name, kind)
        ROUTES[rep["route"]] += 1
    assert all(ROUTES[r] > 0 for r in ("layout", "measured", "linked", "host")), dict(ROUTES)


def _signed(v):
    return v - (1 << 64) if v >= 1 << 63 else v


def _index(d, n, cap, room):
    """frame_index_dev on d[:n] with lists of `room` poisoned entries: (info, pay_off, size_word)."""
    pay = torch.full((room,), -7, dtype=torch.int64, device="cuda")
    word = torch.full((room,), -77, dtype=torch.int32, device="cuda")
    info = torch.full((8,), -777, dtype=torch.int64, device="cuda")
    lz4mi.frame_index_dev(d.data_ptr(), n, pay.data_ptr(), word.data_ptr(), cap, info.data_ptr(),
                          torch.cuda.current_stream().cuda_stream)
    return info.cpu().tolist(), pay.cpu().tolist(), (word.cpu().numpy().astype(np.int64) & 0xFFFFFFFF).tolist()


@pytest.mark.parametrize("name", D.base_names())
def test_frame_index_equals_the_reference_walk(name):
    """All eight info words and the listed entries, the unspecified cases included (the walk decodes
    nothing); entries past info[3] stay poisoned; at a capacity below the block count the overflow
    flag is set, `capacity` blocks are listed and nothing is written behind them."""
    bad = []
    for k, c, f in D.cases(name, specified=False):
        info, blocks = D.walk(f)
        info[2] = _signed(info[2])
        nb = len(blocks)
        room = nb + 4
        for fill in (0x00, 0xFF):
            d = torch.full((f.size + PAD,), fill, dtype=torch.uint8, device="cuda")
            d[:f.size] = torch.from_numpy(f.copy()).cuda()
            gi, gp, gw = _index(d, f.size, room, room)
            if gi != info or list(zip(gp[:nb], gw[:nb])) != blocks or gp[nb:] != [-7] * 4 or \
                    gw[nb:] != [(-77) & 0xFFFFFFFF] * 4:
                bad.append((k, c["k"], fill, gi, info, gp, gw))
        for cap in sorted({nb, max(nb - 1, 0), min(nb, 1), 0}):
            gi, gp, gw = _index(d, f.size, cap, room)
            if cap == nb:          # everything fits: the walk's own words
                want = info
            else:                  # (info[5], the position the walk stopped at, is not part of the contract)
                want = info[:3] + [cap, 0, gi[5], info[6], 1]
            if gi != want or list(zip(gp[:cap], gw[:cap])) != blocks[:cap] or gp[cap:] != [-7] * (room - cap) or \
                    gw[cap:] != [(-77) & 0xFFFFFFFF] * (room - cap):
                bad.append((k, c["k"], "cap", cap, gi, want))
    assert not bad, "%d cases: %r" % (len(bad), bad[:4])


@pytest.mark.parametrize("name", D.base_names())
def test_frame_decompress_info_and_canary(name):
    """lz4mi_frame_decompress (reference mode) on every specified case: a frame it takes gives the
    walk's info words, the recorded status, the oracle's bytes and zeros behind them up to the
    content size at most; a frame without a content size, with one above out_cap (the 2^48 case)
    or whose walk runs off the frame is declined with ERR_ARG; the 4 KiB behind out_cap stay as
    they were in every case."""
    data = D.base_content(name)
    out_cap = data.size + 65536 + 1
    bad = []
    took = 0
    s = torch.cuda.current_stream().cuda_stream
    for k, c, f in D.cases(name):
        info, blocks = D.walk(f)
        d = torch.from_numpy(f.copy()).cuda()
        out = torch.full((out_cap + PAD,), 0xA5, dtype=torch.uint8, device="cuda")
        try:
            got = lz4mi.frame_decompress_dev(d.data_ptr(), f.size, out.data_ptr(), out_cap, s, js_exact=True)
        except lz4mi.Lz4miError as e:
            if e.status == lz4mi.ERR_HIP:
                raise
            got = e.status
        h = out.cpu().numpy()
        if not (h[out_cap:] == 0xA5).all():
            bad.append((k, c["k"], "canary"))
        must_decline = info[0] == 0 and (info[2] == 0 or info[2] > out_cap or info[7])
        if got == lz4mi.ERR_ARG:
            if info[0]:
                bad.append((k, c["k"], "declined", info))
            continue
        if not isinstance(got, dict) or must_decline:
            bad.append((k, c["k"], "taken", got, info))
            continue
        took += 1
        gi = [got[x] for x in ("status", "flg", "content_size", "written", "stored_blocks", "checksum_pos", "block_max",
                               "overflow")]
        want_st = D.expected_status(c["n"])
        if info[0]:
            want = info
        else:
            stored = sum(1 for _, w in blocks if w & 0x80000000)
            want = [want_st, info[1], info[2], gi[3], stored, info[5], info[6], 0]
        if gi != want or not 0 <= gi[3] <= max(info[2], 0):
            bad.append((k, c["k"], "info", gi, want))
        elif want_st == 0 and not info[0]:
            st, ref = O.decompress_frame(f, verify_checksum=False, js_compat=True)
            w = gi[3]
            if st != 0 or ref.size != info[2] or not np.array_equal(h[:w], ref[:w]) or ref[w:].any():
                bad.append((k, c["k"], "bytes", w, ref.size))
    assert not bad, "%d cases: %r" % (len(bad), bad[:6])
    assert took >= (20 if D.base(name)["size"] else 7), took   # (unsized: the magic and version cases)


def test_content_size_above_what_the_frame_can_hold():
    """A content size of 2^48, and any above content_size_bound (255 bytes out per frame byte, plus
    slack): ERR_RANGE from both entry points before anything is allocated for it (a torch
    out-of-memory error would escape as such); lz4mi_frame_decompress keeps ERR_ARG (size > out_cap);
    at the bound itself the frame is decoded, zeros behind the content."""
    from lz4mi import frame as F
    name = "A_is"
    big = [f for _, c, f in D.cases(name) if c["k"] == "hdr_size_2p48"]
    assert len(big) == 1 and int.from_bytes(big[0][6:14].tobytes(), "little") == 1 << 48
    f = D.base_frame(name)
    bound = F.content_size_bound(f.size)
    assert bound == 255 * f.size + 4194304
    over = f.copy()
    over[6:14] = np.frombuffer(int(bound + 1).to_bytes(8, "little"), dtype=np.uint8)
    for g in (big[0], over):
        d = torch.from_numpy(g.copy()).cuda()
        before = torch.cuda.memory_reserved()
        for kw in ({}, {"linked": True}, {"js_exact": True}):
            rep = {}
            with pytest.raises(lz4mi.Lz4miError) as ei:
                F.decompress_frame_device(d, report=rep, **kw)
            assert ei.value.status == lz4mi.ERR_RANGE and rep == {"route": "host"}
        assert torch.cuda.memory_reserved() == before
        with pytest.raises(lz4mi.Lz4miError) as ei:
            F.decompress_frame_host(g)
        assert ei.value.status == lz4mi.ERR_RANGE
        out = torch.empty(1 << 20, dtype=torch.uint8, device="cuda")
        with pytest.raises(lz4mi.Lz4miError) as ei:
            lz4mi.frame_decompress_dev(d.data_ptr(), g.size, out.data_ptr(), out.numel(),
                                       torch.cuda.current_stream().cuda_stream)
        assert ei.value.status == lz4mi.ERR_ARG
    at = f.copy()
    at[6:14] = np.frombuffer(int(bound).to_bytes(8, "little"), dtype=np.uint8)
    data = D.base_content(name)
    for got in (F.decompress_frame_host(at), F.decompress_frame_device(torch.from_numpy(at.copy()).cuda()).cpu().numpy()):
        assert got.size == bound and np.array_equal(got[:data.size], data) and not got[data.size:].any()
