"""Frame block checksums (FLG 0x10) checked without a GPU: lz4mi_host_verify_blocks against the
oracle hash, the argument checks of lz4mi_verify_blocks (made before the device is looked at), and
the host frame route and the sharded plumbing with verify_blocks=True (tests/verify_common.py)."""
import ctypes

import numpy as np
import pytest

import oracle as O
import verify_common as V

lz4mi = pytest.importorskip("lz4mi")
from lz4mi import frame as F  # noqa: E402

BAD = lz4mi.ERR_BLOCK_CHECKSUM


@pytest.mark.parametrize("fill", V.FILLS)
def test_host_verify_sweep(fill):
    """Every length around the 128-stripe pipeline and the short tails, at the four start residues,
    in both surroundings: status 0."""
    arena, offs, lens = V.sweep(fill)
    assert lens.size == 4 * len(V.LENS) and sorted(set(int(o) % 4 for o in offs)) == [0, 1, 2, 3]
    st = lz4mi.host_verify_blocks(arena, offs, lens)
    assert st.dtype == np.int32 and st.shape == lens.shape
    assert np.array_equal(st, V.expected(arena, offs, lens)) and not st.any()


def test_host_verify_damage():
    """One flipped bit in the payload's first, middle or last byte or in a checksum byte: exactly
    that record fails."""
    arena, offs, lens = V.sweep(0x00)
    for b, (off, n) in enumerate(zip(offs, lens)):
        for k, pos in enumerate(V.damage_sites(int(off), int(n))):
            arena[pos] ^= 1 << ((b + k) % 8)
            st = lz4mi.host_verify_blocks(arena, offs, lens)
            arena[pos] ^= 1 << ((b + k) % 8)
            want = np.zeros(lens.size, dtype=np.int32)
            want[b] = BAD
            assert np.array_equal(st, want), (b, int(n), pos - int(off))
    assert not lz4mi.host_verify_blocks(arena, offs, lens).any()


def test_host_verify_frame_words_and_cut_records():
    arena, offs, lens = V.sweep(0xFF)
    words = lens | np.where(np.arange(lens.size) % 2 == 1, 0x80000000, 0).astype(np.uint32)
    assert not lz4mi.host_verify_blocks(arena, offs, words, frame_words=True).any()
    # without the flag bit 31 is length: such a record runs past the array
    st = lz4mi.host_verify_blocks(arena, offs, words)
    assert np.array_equal(st != 0, (words & 0x80000000) != 0)
    # a record cut by in_total, on a buffer that really ends there: the checksum's four bytes, the payload
    for b in (0, 5, 17, len(offs) - 1):                       # lengths 0, 15 and 4096, and the last record
        end = int(offs[b]) + int(lens[b]) + 4
        for total in sorted({end - 1, end - 2, end - 3, end - 4, end - 4 - int(lens[b]) // 2, int(offs[b])}):
            buf = arena[:total].copy()
            st = lz4mi.host_verify_blocks(buf, offs[:b + 1], words[:b + 1], frame_words=True)
            want = np.zeros(b + 1, dtype=np.int32)
            want[b] = BAD
            assert np.array_equal(st, want), (b, total - end)
            assert np.array_equal(st, V.expected(buf, offs[:b + 1], words[:b + 1]))
        buf = arena[:end].copy()
        assert not lz4mi.host_verify_blocks(buf, offs[:b + 1], words[:b + 1], frame_words=True).any()
    # an offset behind the array, and an empty array
    assert lz4mi.host_verify_blocks(arena[:100].copy(), [200, 2 ** 63], [0, 5]).tolist() == [BAD, BAD]
    assert lz4mi.host_verify_blocks(np.zeros(0, dtype=np.uint8), [0], [0]).tolist() == [BAD]
    assert lz4mi.host_verify_blocks(arena, [], []).size == 0


def test_verify_abi():
    L = lz4mi.lib()
    for name in ("lz4mi_verify_blocks", "lz4mi_host_verify_blocks"):
        assert name in lz4mi.EXPORTS and ctypes.cast(getattr(L, name), ctypes.c_void_p).value
    buf = V.record(O.generate("random", 1, 100))
    off, ln = np.zeros(1, dtype=np.uint64), np.array([100], dtype=np.uint32)
    st = np.full(1, 77, dtype=np.int32)
    args = (buf.ctypes.data, buf.size, off.ctypes.data, ln.ctypes.data)
    # both argument checks come before the device is looked at
    assert L.lz4mi_verify_blocks(*args, None, 1, 0, None) == lz4mi.ERR_ARG
    assert L.lz4mi_verify_blocks(None, 0, None, None, None, 0, 0, None) == lz4mi.ERR_ARG
    assert L.lz4mi_verify_blocks(None, 0, None, None, st.ctypes.data, 1, 0, None) == lz4mi.ERR_ARG
    others = {name: getattr(lz4mi, name) for name in ("JS_COMPAT", "JS_EXACT", "BLOCK_CHECKSUM", "XXH_STANDARD",
                                                        "LINKED", "LINKED_EXACT", "VERIFY_BLOCKS")}
    for name, flag in others.items():
        for base in (0, lz4mi.DEVICE_PTRS, lz4mi.FRAME_WORDS):
            assert L.lz4mi_verify_blocks(*args, st.ctypes.data, 1, base | flag, None) == lz4mi.ERR_ARG, name
        assert L.lz4mi_host_verify_blocks(*args, st.ctypes.data, 1, flag) == lz4mi.ERR_ARG, name
    assert L.lz4mi_host_verify_blocks(*args, st.ctypes.data, 1, lz4mi.DEVICE_PTRS) == lz4mi.ERR_ARG
    assert L.lz4mi_host_verify_blocks(*args, None, 1, 0) == lz4mi.ERR_ARG
    assert st[0] == 77
    assert L.lz4mi_host_verify_blocks(*args, st.ctypes.data, 1, 0) == 0 and st[0] == 0
    assert lz4mi.status_message(-10) == "LZ4: Block Checksum Error" and BAD == -10
    assert lz4mi.VERIFY_BLOCKS == 0x200
    every = [lz4mi.DEVICE_PTRS, lz4mi.FRAME_WORDS, lz4mi.XXH_LEN64] + [v for k, v in others.items() if k != "VERIFY_BLOCKS"]
    assert all(lz4mi.VERIFY_BLOCKS & f == 0 for f in every)


@pytest.mark.parametrize("indep", (True, False))
@pytest.mark.parametrize("sized", (True, False))
@pytest.mark.parametrize("how", V.DAMAGES)
def test_host_frame_route_raises_on_damage(indep, sized, how):
    """decompress_frame_host(verify_blocks=True) checks every record before the first block is decoded:
    a damaged frame raises without a GPU."""
    with pytest.raises(lz4mi.Lz4miError) as ei:
        F.decompress_frame_host(V.damaged(V.frame(indep, sized), how), verify_blocks=True)
    assert ei.value.status == BAD and str(ei.value) == "LZ4: Block Checksum Error"


def test_sharded_plumbing_on_the_host():
    """decompress_frame_sharded without torch.distributed, a host frame and a host decoder."""
    f = V.frame(True, True)
    out = F.decompress_frame_sharded(f.copy(), decoder=V.HostDecoder(), verify_blocks=True)
    assert np.array_equal(out.numpy(), V.data())
    for how in ("payload0", "stored", "last_sum"):
        with pytest.raises(lz4mi.Lz4miError) as ei:
            F.decompress_frame_sharded(V.damaged(f, how), decoder=V.HostDecoder(), verify_blocks=True)
        assert ei.value.status == BAD, how
    with pytest.raises(ValueError):
        F.decompress_frame_sharded(f.copy(), decoder=V.NoVerifyDecoder(), verify_blocks=True)
    # the default skips the checksums, like the reference: a damaged checksum changes nothing
    for dec in (V.HostDecoder(), V.NoVerifyDecoder()):
        out = F.decompress_frame_sharded(V.damaged(f, "last_sum"), decoder=dec)
        assert np.array_equal(out.numpy(), V.data())
    # a frame without block checksums: the keyword changes nothing
    plain = V.frame(True, True, block_checksum=False)
    out = F.decompress_frame_sharded(plain.copy(), decoder=V.HostDecoder(), verify_blocks=True)
    assert np.array_equal(out.numpy(), V.data())
