"""Damaged frames on the CPU: the oracle's frame decoder and shard.frame_blocks against what the
reference's decompressBuffer did with the same frames (tests/golden/damaged_frames.json, recorded
by tools/golden/gen_damaged_frames.mjs under node). test_gpu_damaged_frames.py takes its expected
bytes from the oracle, which this module pins."""
import numpy as np
import pytest

import damaged_common as D
import oracle as O

# the oracle reports a content size above its caller's capacity as Output Buffer Too Small, where
# the reference fails to allocate (RangeError of new Uint8Array): the 2^48 case
ORACLE_ALLOC = -1


def test_fixture_shape_and_caps():
    """A few thousand cases; no unspecified case decodes into a content-sized (zero-initialised)
    result, and at most 15 % of an unsized base frame's cases are unspecified."""
    fx = D.fixture()
    assert fx["block"] == 65536
    names = D.base_names()
    assert len(names) == 13 and "E_iu" in names
    total = 0
    for name in names:
        b = D.base(name)
        allc = D.cases(name, specified=False)
        unspec = [(c, f) for _, c, f in allc if c.get("u")]
        total += len(allc)
        assert len(unspec) == b["unspecified"]
        assert len(allc) >= 40
        for c, f in unspec:
            assert "v" not in c and "n" not in c
            info, _ = D.walk(f)
            assert not (info[0] == 0 and info[2] > 0 and info[2] < 2 ** 32), (name, c)
        if b["size"]:
            assert not unspec, name
        else:
            assert len(unspec) <= 0.15 * len(allc), name
        kinds = {c["k"] for _, c, _ in allc}
        assert {"cut_head", "hdr_flg", "hdr_bd", "hdr_hc", "no_endmark", "garbage", "whole"} <= kinds
        if name != "E_iu":      # (the 11-byte empty frame: every cut is one of the first 33)
            assert {"cut_edge", "cut_block", "word", "dup", "drop", "swap", "stored_past", "payload"} <= kinds
    assert 1000 <= total <= 6000


@pytest.mark.parametrize("name", D.base_names())
def test_undamaged_frames_decode_to_their_content(name):
    f = D.base_frame(name)
    whole = [c for _, c, g in D.cases(name) if c["k"] == "whole"]
    data = D.base_content(name)
    # (verified, the reference fails its own frames with a content checksum: the text blocks' double-copy-tail
    # rewrites, SURVEY F1, change bytes of its result)
    assert len(whole) == 1 and whole[0]["n"][:2] == [1, data.size]
    assert whole[0]["v"] == (whole[0]["n"] if not D.base(name)["csum"] else [0, "Error", "LZ4: Content Checksum Error"])
    st, out = O.decompress_frame(f, js_compat=False)
    assert st == 0 and np.array_equal(out, data)


@pytest.mark.parametrize("name", D.base_names())
def test_oracle_reproduces_the_reference(name):
    """Status (by message), length and XXH32 of every specified case, verifyChecksum both ways."""
    bad = []
    for k, c, f in D.cases(name):
        for verify, key in ((True, "v"), (False, "n")):
            want = c[key]
            st, out = O.decompress_frame(f, verify_checksum=verify, js_compat=True)
            exp = D.expected_status(want)
            if exp == "alloc":
                assert c["k"] == "hdr_size_2p48"
                exp = ORACLE_ALLOC
            got = [1, int(out.size), "%08x" % O.xxh32(out)] if st == 0 else st
            if got != (want if exp == 0 else exp):
                bad.append((k, c["k"], verify, want, got))
    assert not bad, (len(bad), bad[:6])


@pytest.mark.parametrize("name", D.base_names())
def test_frame_blocks_lists_the_reference_walk(name):
    """shard.frame_blocks against the byte-wise restatement of the reference's walk, for every case
    (the unspecified ones too: the walk does not depend on the decode)."""
    from lz4mi import shard
    bad = []
    for k, c, f in D.cases(name, specified=False):
        info, blocks = D.walk(f)
        if info[0] == -5:
            with pytest.raises(ValueError):
                shard.frame_blocks(f)
            continue
        hi, hb = shard.frame_blocks(f)
        if info[0] == -6:
            if ((hi["flg"] & 0xC0) >> 6) == 1 or hi["flg"] != info[1]:
                bad.append((k, c["k"], "version", hi["flg"], info[1]))
            continue
        want = [(p, w & 0x7FFFFFFF, bool(w & 0x80000000)) for p, w in blocks]
        got = (hi["flg"], hi["content_size"], hi["block_max"], hi["end"], hi["checksum"], hi["independent"])
        exp = (info[1], info[2], info[6], info[5], bool(info[1] & 4), bool(info[1] & 0x20))
        if got != exp or list(hb) != want:
            bad.append((k, c["k"], got, exp, hb[-1:], want[-1:]))
    assert not bad, (len(bad), bad[:6])


def test_host_block_read_end():
    """Where the reference's walk of a block stops reading: at most the block's end for every block
    of the base frames, behind it when an offset's second byte or a length's continuation bytes lie
    there (the frame's real bytes in the reference, zeros past the array)."""
    lz4mi = pytest.importorskip("lz4mi")
    from lz4mi import shard
    for name in ("A_is", "B_du"):
        f = D.base_frame(name)
        blocks = shard.frame_blocks(f)[1]
        assert len(blocks) == 3
        for p, n, stored in blocks:
            if not stored:
                assert lz4mi.host_block_read_end(f, p, n) == p + n
                # one byte more: the next record's first byte is a token, an offset follows or it is malformed
                assert lz4mi.host_block_read_end(f, p, n + 1) in (p + n + 1, p + n + 2)
    a = np.frombuffer(b"\x10a\x05\x07", dtype=np.uint8)
    assert lz4mi.host_block_read_end(a, 0, 3) == 4          # the offset's second byte
    assert lz4mi.host_block_read_end(a, 0, 4) == 4
    b = np.frombuffer(b"\x1fa\x01\x00\xff\xff\x03\x50", dtype=np.uint8)
    assert lz4mi.host_block_read_end(b, 0, 5) == 7          # match length bytes up to the first below 255
    assert lz4mi.host_block_read_end(b[:6], 0, 5) == 7      # past the array: zeros
    assert lz4mi.host_block_read_end(b, 2, 0) == 2
    with pytest.raises(lz4mi.Lz4miError):
        lz4mi.host_block_read_end(b, -1, 2)
