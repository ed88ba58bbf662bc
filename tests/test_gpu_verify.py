"""Frame block checksums (FLG 0x10) checked on the GPU: lz4mi_verify_blocks (host and device
pointers) against lz4mi_host_verify_blocks and the oracle hash, its footprint, and verify_blocks=True
through lz4mi_frame_decompress and every route of the frame layer (tests/verify_common.py)."""
import numpy as np
import pytest

import verify_common as V
from footprint_common import FILL, SENTINELS, assert_sentinels

lz4mi = pytest.importorskip("lz4mi")
torch = pytest.importorskip("torch")
from lz4mi import frame as F  # noqa: E402

pytestmark = pytest.mark.gpu
BAD = lz4mi.ERR_BLOCK_CHECKSUM


def _cuda(a, dt):
    return torch.from_numpy(np.ascontiguousarray(a).astype(dt)).cuda()


def _words(a):
    return np.ascontiguousarray(a, dtype=np.uint32).view(np.int32)


class Dev:
    """A record list on the device; verify() is one lz4mi_verify_blocks call on device pointers."""

    def __init__(self, arena, offs, words, frame_words=False):
        self.buf, self.n, self.fw = _cuda(arena, np.uint8), len(offs), frame_words
        self.off, self.word = _cuda(np.asarray(offs, dtype=np.uint64).view(np.int64), np.int64), _cuda(_words(words), np.int32)

    def verify(self, total=None):
        st = torch.full((self.n + SENTINELS,), FILL, dtype=torch.int32, device="cuda")
        lz4mi.verify_blocks_dev(self.buf.data_ptr(), self.buf.numel() if total is None else total, self.off.data_ptr(),
                                self.word.data_ptr(), st.data_ptr(), self.n, torch.cuda.current_stream().cuda_stream,
                                frame_words=self.fw)
        return st


@pytest.mark.parametrize("fill", V.FILLS)
def test_sweep(fill):
    arena, offs, lens = V.sweep(fill)
    want = V.expected(arena, offs, lens)
    assert not want.any() and np.array_equal(lz4mi.host_verify_blocks(arena, offs, lens), want)
    assert np.array_equal(lz4mi.verify_blocks(arena, offs, lens), want)
    d = Dev(arena, offs, lens)
    st = d.verify().cpu().numpy()
    assert np.array_equal(st[:d.n], want)
    assert_sentinels(st, d.n)
    assert np.array_equal(d.buf.cpu().numpy(), arena)


def test_damage_device_pointers():
    """One flipped bit per call, every site of every record: exactly that record fails."""
    arena, offs, lens = V.sweep(0x00)
    d = Dev(arena, offs, lens)
    got, want = [], []
    for b, (off, n) in enumerate(zip(offs, lens)):
        for k, pos in enumerate(V.damage_sites(int(off), int(n))):
            bit = 1 << ((b + k) % 8)
            d.buf[pos] ^= bit
            got.append(d.verify()[:d.n])
            d.buf[pos] ^= bit
            w = np.zeros(d.n, dtype=np.int32)
            w[b] = BAD
            want.append(w)
    got = torch.stack(got).cpu().numpy()
    bad = np.nonzero((got != np.stack(want)).any(axis=1))[0]
    assert bad.size == 0, (bad[:5], got[bad[0]].nonzero())
    assert np.array_equal(d.buf.cpu().numpy(), arena)


def test_damage_host_pointers():
    """The same through the staging path, one record per length (the residues in turn)."""
    arena, offs, lens = V.sweep(0xFF)
    for k in range(len(V.LENS)):
        b = 4 * k + k % 4
        for j, pos in enumerate(V.damage_sites(int(offs[b]), int(lens[b]))):
            arena[pos] ^= 1 << ((b + j) % 8)
            st = lz4mi.verify_blocks(arena, offs, lens)
            assert np.array_equal(st, lz4mi.host_verify_blocks(arena, offs, lens))
            arena[pos] ^= 1 << ((b + j) % 8)
            want = np.zeros(lens.size, dtype=np.int32)
            want[b] = BAD
            assert np.array_equal(st, want), (b, int(lens[b]), pos - int(offs[b]))


def test_frame_words_and_cut_records():
    arena, offs, lens = V.sweep(0xFF)
    words = lens | np.where(np.arange(lens.size) % 2 == 1, 0x80000000, 0).astype(np.uint32)
    assert not lz4mi.verify_blocks(arena, offs, words, frame_words=True).any()
    assert not Dev(arena, offs, words, frame_words=True).verify()[:lens.size].any().item()
    for st in (lz4mi.verify_blocks(arena, offs, words), Dev(arena, offs, words).verify()[:lens.size].cpu().numpy()):
        assert np.array_equal(st != 0, (words & 0x80000000) != 0)      # bit 31 is length without the flag
    for b in (0, 5, 17, len(offs) - 1):
        end = int(offs[b]) + int(lens[b]) + 4
        for total in sorted({end, end - 1, end - 2, end - 3, end - 4, end - 4 - int(lens[b]) // 2, int(offs[b])}):
            buf = arena[:total].copy()                         # the buffer really ends at in_total
            o, w = offs[:b + 1], words[:b + 1]
            want = V.expected(buf, o, w)
            assert want[b] == (0 if total == end else BAD) and not want[:b].any()
            assert np.array_equal(lz4mi.host_verify_blocks(buf, o, w, frame_words=True), want)
            assert np.array_equal(lz4mi.verify_blocks(buf, o, w, frame_words=True), want), (b, total - end)
            if total:
                assert np.array_equal(Dev(buf, o, w, frame_words=True).verify()[:b + 1].cpu().numpy(), want), (b, total - end)
    # in_total smaller than the buffer bounds the reads as well
    d = Dev(arena, offs, words, frame_words=True)
    total = int(offs[40]) + int(lens[40]) + 3
    assert np.array_equal(d.verify(total)[:d.n].cpu().numpy(), V.expected(arena, offs, words, total))
    assert lz4mi.verify_blocks(arena[:100].copy(), [200, 2 ** 63], [0, 5]).tolist() == [BAD, BAD]


@pytest.mark.parametrize("nb", (1, 16, 17, 65))
def test_footprint(nb):
    """Only status[0 .. nblocks) is written (64 sentinel entries behind it), the input is unchanged,
    and the statuses do not depend on the bytes around the records: the quad, wave and workgroup edges."""
    seen = []
    for fill in V.FILLS:
        arena, offs, lens = V.sweep(fill)
        arena[int(offs[nb // 2]) + int(lens[nb // 2]) + 1] ^= 0x40          # one failing record
        offs, lens = offs[:nb], lens[:nb]
        want = V.expected(arena, offs, lens)
        assert want[nb // 2] == BAD and np.count_nonzero(want) == 1
        d = Dev(arena, offs, lens)
        st = d.verify().cpu().numpy()
        assert_sentinels(st, nb, f"device pointers, fill {fill}")
        assert np.array_equal(d.buf.cpu().numpy(), arena)
        host = np.full(nb + SENTINELS, FILL, dtype=np.int32)
        before = arena.copy()
        assert lz4mi.lib().lz4mi_verify_blocks(arena.ctypes.data, arena.size, offs.ctypes.data, lens.ctypes.data,
                                               host.ctypes.data, nb, 0, None) == 0
        assert_sentinels(host, nb, f"host pointers, fill {fill}")
        assert np.array_equal(arena, before)
        assert np.array_equal(st[:nb], want) and np.array_equal(host[:nb], want)
        seen.append(st[:nb])
    assert np.array_equal(seen[0], seen[1])


MODES = ({}, {"js_exact": True}, {"linked": True}, {"linked": "exact"})


def _layout(f, **kw):
    """frame_decompress_dev on a host frame -> (info, the output buffer's content-size bytes)."""
    d = _cuda(f, np.uint8)
    out = torch.zeros(V.data().size, dtype=torch.uint8, device="cuda")
    info = lz4mi.frame_decompress_dev(d.data_ptr(), d.numel(), out.data_ptr(), out.numel(),
                                      torch.cuda.current_stream().cuda_stream, **kw)
    torch.cuda.synchronize()
    return info, out.cpu().numpy()


@pytest.mark.parametrize("mode", range(len(MODES)))
@pytest.mark.parametrize("indep", (True, False))
def test_frame_decompress(indep, mode):
    """lz4mi_frame_decompress with LZ4MI_VERIFY_BLOCKS on the sized frames. The frame cut inside its last
    checksum is one the function declines with or without the flag (the walk runs past the frame's end:
    LZ4MI_ERR_ARG, the header's rule "frames the function declines today still return LZ4MI_ERR_ARG"); the
    frame layer then reports ERR_BLOCK_CHECKSUM from the host route (test_frame_device_routes). The decoded
    bytes are the input in the spec modes and the oracle's reference decode in the reference modes (whose
    double-copy-tail rewrite changes bytes of the text blocks)."""
    kw = MODES[mode]
    f = V.frame(indep, True)
    want = V.decoded(indep, bool(kw.get("js_exact")) or kw.get("linked") == "exact")
    info, out = _layout(f, verify_blocks=True, **kw)
    assert info["status"] == 0 and info["written"] == V.data().size and np.array_equal(out, want)
    for how in ("payload0", "stored", "last_sum", "decode0"):
        info, _ = _layout(V.damaged(f, how), verify_blocks=True, **kw)
        assert info["status"] == BAD and info["written"] == 0, (how, info)
    for verify in (False, True):
        with pytest.raises(lz4mi.Lz4miError) as ei:
            _layout(V.damaged(f, "cut"), verify_blocks=verify, **kw)
        assert ei.value.status == lz4mi.ERR_ARG
    # the default skips the checksums, as before
    info, out = _layout(V.damaged(f, "last_sum"), **kw)
    assert info["status"] == 0 and np.array_equal(out, want)
    # a frame without FLG 0x10: the flag changes nothing
    plain = V.frame(indep, True, block_checksum=False)
    a, b = _layout(plain, **kw), _layout(plain, verify_blocks=True, **kw)
    assert a[0] == b[0] and a[0]["status"] == 0 and np.array_equal(a[1], b[1]) and np.array_equal(a[1], want)


ROUTES = (("layout", True, True, {}), ("layout", False, True, {}), ("measured", True, False, {}),
          ("linked", False, False, {"linked": True}), ("host", False, False, {}))


def _device(f, **kw):
    rep = {}
    try:
        out = F.decompress_frame_device(_cuda(f, np.uint8), report=rep, **kw)
    except lz4mi.Lz4miError as e:
        return rep.get("route"), e.status
    return rep.get("route"), out.cpu().numpy()


@pytest.mark.parametrize("route,indep,sized,kw", ROUTES)
def test_frame_device_routes(route, indep, sized, kw):
    f = V.frame(indep, sized)
    got = _device(f, verify_blocks=True, **kw)
    assert got[0] == route and np.array_equal(got[1], V.data())
    for how in V.DAMAGES:
        r, st = _device(V.damaged(f, how), verify_blocks=True, **kw)
        assert isinstance(st, int) and st == BAD, (how, st)
        assert r == ("host" if how == "cut" else route), (how, r)      # (a cut frame is every walk's overflow)
    # what was missing. A damaged checksum alone goes unnoticed by default, like in the reference ...
    got = _device(V.damaged(f, "last_sum"), **kw)
    assert got[0] == route and np.array_equal(got[1], V.data())
    # ... and so does a damaged stored block of a frame without a content checksum: wrong bytes, no error
    g = V.frame(indep, sized, content_checksum=False)
    r, out = _device(V.damaged(g, "stored"), **kw)
    assert r == route and isinstance(out, np.ndarray) and out.size == V.data().size
    diff = np.nonzero(out != V.data())[0]
    assert diff.tolist() == [2 * V.BS + 1000]
    assert _device(V.damaged(g, "stored"), verify_blocks=True, **kw) == (route, BAD)
    assert np.array_equal(_device(g, verify_blocks=True, **kw)[1], V.data())


def test_sharded_device_decoder():
    f = V.frame(True, True)
    out = F.decompress_frame_sharded(_cuda(f, np.uint8), decoder=F.DeviceDecoder(), verify_blocks=True)
    assert np.array_equal(out.cpu().numpy(), V.data())
    for how in ("payload0", "stored", "last_sum"):
        with pytest.raises(lz4mi.Lz4miError) as ei:
            F.decompress_frame_sharded(_cuda(V.damaged(f, how), np.uint8), decoder=F.DeviceDecoder(), verify_blocks=True)
        assert ei.value.status == BAD, how
    out = F.decompress_frame_sharded(_cuda(V.damaged(f, "last_sum"), np.uint8), decoder=F.DeviceDecoder())
    assert np.array_equal(out.cpu().numpy(), V.data())
    st = F.DeviceDecoder().verify(torch.from_numpy(f.copy()), torch.tensor([p for p, _, _ in V.blocks_of(f)]),
                                  torch.tensor([n | (0x80000000 if s else 0) for _, n, s in V.blocks_of(f)]))
    assert st.dtype == torch.int32 and st.cpu().tolist() == [0] * 5
