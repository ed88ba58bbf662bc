"""Decoded sizes on the GPU (lz4mi_decoded_sizes, csrc/lz4mi_size.hip) against the host walker
lz4mi_host_decoded_size and the pure-Python walker, decode at measured sizes, and the measured
route of decompress_frame_device for frames the layout walk declines."""
import numpy as np
import pytest

import oracle as O
import sizes_common as C

lz4mi = pytest.importorskip("lz4mi")
torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _init():
    lz4mi.init(0)


def _host(blocks):
    got = [lz4mi.host_decoded_size(b) for b in blocks]
    return np.array([g[0] for g in got], dtype=np.int32), np.array([g[1] for g in got], dtype=np.uint32)


def _dev(blocks, frame_words=False, words=None):
    """decoded_sizes_dev on device tensors: (statuses, sizes)."""
    n = len(blocks)
    lens = np.array([b.size for b in blocks], dtype=np.int64)
    off = np.zeros(n, dtype=np.int64)
    off[1:] = np.cumsum(lens[:-1])
    src = np.concatenate(list(blocks)) if lens.sum() else np.zeros(1, dtype=np.uint8)
    d_src = torch.from_numpy(src.copy()).cuda()
    d_off = torch.from_numpy(off).cuda()
    w = lens.astype(np.uint32) if words is None else np.asarray(words, dtype=np.uint32)
    d_len = torch.from_numpy(w.view(np.int32).copy()).cuda()
    # poisoned: every entry has to be written by the kernel
    d_size = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    d_st = torch.full((n,), -77, dtype=torch.int32, device="cuda")
    s = torch.cuda.current_stream()
    lz4mi.decoded_sizes_dev(d_src.data_ptr(), d_off.data_ptr(), d_len.data_ptr(), d_size.data_ptr(), d_st.data_ptr(), n,
                            s.cuda_stream, frame_words=frame_words)
    torch.cuda.synchronize()
    return d_st.cpu().numpy(), d_size.cpu().numpy().view(np.uint32)


@pytest.fixture(scope="module")
def batch_blocks():
    """(sources, compressed): the six generators at the sweep's sizes and five 4 MiB blocks."""
    srcs = [O.generate(kind, 5, n) for kind in C.GENERATOR_KINDS for n in C.SOURCE_SIZES]
    n = 4 << 20
    srcs += [O.generate("tiles216", 9, n), O.generate("text", 9, n),
             O.generate("random", 9, n),                                   # one 4 MiB literal run
             np.zeros(n, dtype=np.uint8),                                  # one offset-1 match, a ~16 KiB varint
             np.tile(np.array([1, 2, 3], dtype=np.uint8), n // 3 + 1)[:n]]  # period 3
    comps = [O.compress_block_bytes(s) for s in srcs]
    return srcs, comps


def test_batches_equal_the_host_walker(batch_blocks):
    srcs, comps = batch_blocks
    want = np.array([s.size for s in srcs], dtype=np.uint32)
    hst, hsz = _host(comps)
    assert (hst == 0).all() and np.array_equal(hsz, want)
    n = len(comps)
    rep = [k % n for k in range(300)]
    for idx in ([n - 5], [n - 4, 3], [n - 3, n - 2, n - 1, 0, 7], list(range(n)), rep):
        sub = [comps[k] for k in idx]
        st, sz = lz4mi.decoded_sizes(sub)
        assert (st == 0).all() and np.array_equal(sz, want[idx]), idx[:5]
        st, sz = _dev(sub)
        assert (st == 0).all() and np.array_equal(sz, want[idx]), idx[:5]


def test_decode_at_measured_sizes(batch_blocks):
    srcs, comps = batch_blocks
    st, outs, lens = lz4mi.decompress_blocks(comps, out_sizes=None)
    assert (st == 0).all()
    for k, (s, o) in enumerate(zip(srcs, outs)):
        assert lens[k] == s.size and np.array_equal(s, o), k
    st, outs, _ = lz4mi.decompress_blocks(c for c in comps[:3])            # any iterable
    assert (st == 0).all() and all(np.array_equal(a, b) for a, b in zip(outs, srcs[:3]))
    # a block the size pass fails keeps that status; the others decode
    bad = np.frombuffer(b"\x90abc", dtype=np.uint8)
    st, outs, _ = lz4mi.decompress_blocks([comps[3], bad, comps[5]], out_sizes=None)
    assert list(st) == [0, lz4mi.ERR_MALFORMED, 0]
    assert np.array_equal(outs[0], srcs[3]) and np.array_equal(outs[2], srcs[5]) and outs[1].size == 0


def test_chunk_edges():
    blocks = C.chunk_edge_blocks()
    assert len(blocks) >= 200
    hst, hsz = _host(blocks)
    walked = [C.walk(b) for b in blocks]
    assert [(int(a), int(b)) for a, b in zip(hst, hsz)] == walked
    assert (hst == 0).all()
    st, sz = _dev(blocks)
    bad = np.nonzero((st != hst) | (sz != hsz))[0]
    assert bad.size == 0, (bad[:8], st[bad[:8]], sz[bad[:8]], hsz[bad[:8]])


def test_prefixes_equal_the_host_walker():
    pre = C.prefixes()
    assert len(pre) == 11561
    hst, hsz = _host(pre)
    st, sz = _dev(pre)
    bad = np.nonzero((st != hst) | (sz != hsz))[0]
    assert bad.size == 0, (bad[:8], st[bad[:8]], hst[bad[:8]], sz[bad[:8]], hsz[bad[:8]])
    assert set(hst.tolist()) == {0, -2, -3}


def test_mutations_equal_the_host_walker():
    muts = [m for part in C.mutations() for m in part]
    assert len(muts) == 4000
    hst, hsz = _host(muts)
    st, sz = _dev(muts)
    bad = np.nonzero((st != hst) | (sz != hsz))[0]
    assert bad.size == 0, (bad[:8], st[bad[:8]], hst[bad[:8]], sz[bad[:8]], hsz[bad[:8]])


def test_hand_built_and_overflow():
    blocks = [np.zeros(0, dtype=np.uint8), C.arr(b"\x00"), C.arr(C.seq(5, 8, 3) + C.seq(7)),
              C.arr(C.seq(5, 8, 3) + C.seq(0, 20, 1)), C.arr(C.seq(3, 4, 1) + b"\x90abc"),
              C.arr(C.seq(3, 4, 1) + C.seq(2, 9, 0) + C.seq(4)), C.arr(C.seq(3, 4, 1) + b"\x10a\x05"),
              C.arr(C.seq(3, 4, 1) + b"\x10a\x00"), C.arr(C.seq(3, 4, 1) + b"\x1fa\x01\x00\xff\xff"),
              C.arr(C.seq(3, 4, 1) + b"\xf0\xff\xff"),
              C.arr(b"\x1fa\x01\x00" + b"\xff" * (17 << 19))]   # above 2^31 - 1: Output Buffer Too Small
    for k in (1, 2, 5, 300):
        blocks.append(C.arr(C.seq(2, 6, 2) + C.seq(C.ext_len(k), 5, 1) + C.seq(3)))
        blocks.append(C.arr(C.seq(2, 6, 2) + C.seq(1, C.ext_len(k) + 4, 1) + C.seq(3)))
        blocks.append(C.arr(C.seq(C.ext_len(k), C.ext_len(k) + 4, 7)))
    hst, hsz = _host(blocks)
    assert (int(hst[10]), int(hsz[10])) == (lz4mi.ERR_OUTPUT_TOO_SMALL, 0x7FFFFFFF)
    assert [(int(a), int(b)) for a, b in zip(hst, hsz)] == [C.walk(b) for b in blocks]
    for st, sz in (_dev(blocks), lz4mi.decoded_sizes(blocks)):
        assert np.array_equal(st, hst) and np.array_equal(sz, hsz), (st, hst, sz, hsz)


def test_frame_words():
    """Size words: bit 31 = a stored block (size = the word's low 31 bits, status 0, its bytes unread)."""
    a, b = C.base_blocks()
    stored = O.generate("random", 3, 5000)
    bad = C.arr(C.seq(3, 4, 1) + b"\x90abc")
    blocks = [a, stored, b, stored[:0], bad, stored[:1]]
    words = [a.size, 5000 | 0x80000000, b.size, 0x80000000, bad.size, 1 | 0x80000000]
    st, sz = _dev(blocks, frame_words=True, words=words)
    assert list(st) == [0, 0, 0, 0, lz4mi.ERR_MALFORMED, 0]
    assert list(sz) == [8192, 5000, 8192, 0, 7, 1]


@pytest.fixture(scope="module")
def mixed_data():
    return np.concatenate([O.generate("tiles216", 31, 900000), O.generate("random", 32, 300000),
                           O.generate("text", 33, 500000), O.generate("repetitive", 34, 77777)])


def _status_of(fn):
    try:
        fn()
    except lz4mi.Lz4miError as e:
        return e.status
    return 0


def _check_measured_frame(f, data, has_checksum):
    from lz4mi import frame as F
    from lz4mi import shard
    rep = {}
    got = F.decompress_frame_device(torch.from_numpy(f.copy()).cuda(), report=rep)
    assert rep == {"route": "measured"}
    assert np.array_equal(got.cpu().numpy(), data)
    if has_checksum:
        c = f.copy()
        c[-1] ^= 0x55
        with pytest.raises(lz4mi.Lz4miError) as ei:
            F.decompress_frame_device(torch.from_numpy(c).cuda())
        assert ei.value.status == lz4mi.ERR_CHECKSUM
    # one block truncated (its size word says so): the host path's error, through the host route
    info, blocks = shard.frame_blocks(f)
    comp = [b for b in blocks if not b[2]]
    p, n, stored = comp[len(comp) // 2]
    for cut in range(1, 9):
        t = np.concatenate([f[:p - 4], np.frombuffer(int(n - cut).to_bytes(4, "little"), dtype=np.uint8),
                            f[p:p + n - cut], f[p + n:]])
        want = _status_of(lambda: F.decompress_frame_host(t))
        if want not in (0, lz4mi.ERR_CHECKSUM):
            break
    assert want not in (0, lz4mi.ERR_CHECKSUM)
    assert want == O.decompress_frame(t)[0]      # the reference's error for it, not only the host route's
    rep = {}
    assert _status_of(lambda: F.decompress_frame_device(torch.from_numpy(t.copy()).cuda(), report=rep)) == want
    assert rep == {"route": "host"}


@pytest.mark.parametrize("bs,cs,bcs", [(65536, True, False), (65536, False, True), (4194304, True, True),
                                       (4194304, False, False)])
def test_unsized_frames_take_the_measured_route(mixed_data, bs, cs, bcs):
    f = O.compress_frame(mixed_data, None, bs, True, cs, False, block_checksum=bcs)
    _check_measured_frame(f, mixed_data, cs)


def test_sized_frame_with_a_short_middle_block(mixed_data):
    from lz4mi import frame as F
    data = mixed_data[:400000]
    cuts = [0, 65536, 65536 + 30000, 2 * 65536 + 30000, 3 * 65536 + 30000, 3 * 65536 + 30001, data.size]
    f = bytearray(F.header(65536, independent=True, content_checksum=True, content_size=data.size))
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        for a in range(lo, hi, 65536):
            raw = data[a:min(a + 65536, hi)]
            comp = O.compress_block_bytes(raw)
            if comp.size < raw.size:
                f += int(comp.size).to_bytes(4, "little") + comp.tobytes()
            else:
                f += int(raw.size | 0x80000000).to_bytes(4, "little") + raw.tobytes()
    f += (0).to_bytes(4, "little") + int(lz4mi.xxh32(data)).to_bytes(4, "little")
    f = np.frombuffer(bytes(f), dtype=np.uint8)
    assert np.array_equal(F.decompress_frame_host(f), data)
    _check_measured_frame(f, data, True)


def test_frames_left_on_their_routes(mixed_data):
    from lz4mi import frame as F
    data = mixed_data[:600000]
    for f, js_exact, route in ((O.compress_frame(data, None, 65536, False, True, False), False, "host"),
                               (O.compress_frame(data, None, 65536, True, True, False), True, "host"),
                               (O.compress_frame(data, None, 65536, True, True, True), False, "layout")):
        want = F.decompress_frame_host(f, js_exact=js_exact)
        rep = {}
        got = F.decompress_frame_device(torch.from_numpy(f.copy()).cuda(), js_exact=js_exact, report=rep)
        assert rep == {"route": route}
        assert np.array_equal(got.cpu().numpy(), want)


def test_blocks_that_read_earlier_output_are_decoded_in_order(mixed_data):
    """An unsized frame flagged independent whose blocks reference earlier blocks' output (a
    dependent-block frame with FLG 0x20 set): the batch reports CROSS_BLOCK for them, each is then
    decoded alone in order, and the bytes are the host path's (a match offset has 16 bits, so the
    host path's 64 KiB window holds everything a block can reach)."""
    from lz4mi import frame as F
    data = mixed_data[:600000]
    f = O.compress_frame(data, None, 65536, False, True, False).copy()
    f[4] |= 0x20
    f[6] = (lz4mi.xxh32(f[4:6]) >> 8) & 0xFF
    want = F.decompress_frame_host(f)
    assert np.array_equal(want, data)
    rep = {}
    got = F.decompress_frame_device(torch.from_numpy(f.copy()).cuda(), report=rep)
    assert rep == {"route": "measured"}
    assert np.array_equal(got.cpu().numpy(), want)
