"""Decoded sizes without decoding, host side (no GPU needed): lz4mi_host_decoded_size, the
sequence walk of blockDecompress.js:55-139 with the copies left out and the checker of the
GPU size pass, against the oracle's decoder and an independent pure-Python walker."""
import ctypes

import numpy as np
import pytest

import oracle as O
import sizes_common as C

lz4mi = pytest.importorskip("lz4mi")

CAP = 4 << 20


@pytest.fixture(scope="module")
def scratch():
    return np.zeros(CAP, dtype=np.uint8)


def oracle_size(comp, scratch):
    """The oracle's decode with a 4 MiB capacity: (status, written)."""
    st, w, _ = O.decompress_block(comp, CAP, out=scratch)
    return st, w


@pytest.mark.parametrize("kind", C.GENERATOR_KINDS)
def test_generator_sweep(kind, scratch):
    for n in C.SOURCE_SIZES:
        src = O.generate(kind, 5, n)
        comp = O.compress_block_bytes(src)
        assert lz4mi.host_decoded_size(comp) == (0, n), (kind, n)
        est, ew = oracle_size(comp, scratch)
        assert (est, ew) == (0, n), (kind, n)


def test_every_prefix_equals_the_oracle(scratch):
    """Status of every prefix == the oracle's; the size == the oracle's `written` where the oracle
    reports one (it leaves 0 behind when it returns an error, as the reference returns nothing
    when it throws) and == the walker's outPos - outputOffset at the throw for every prefix."""
    pre = C.prefixes()
    assert len(pre) == 11561
    seen = set()
    for p in pre:
        est, ew = oracle_size(p, scratch)
        seen.add(est)
        assert est in (0, -2, -3), p.size            # nothing is skipped
        st, size = lz4mi.host_decoded_size(p)
        assert st == est, p.size
        if est == 0:
            assert size == ew, p.size
        else:
            assert ew == 0
        assert (st, size) == C.walk(p), p.size
    assert seen == {0, -2, -3}


@pytest.mark.parametrize("which,share", [(0, 1 / 4), (1, 9 / 10)], ids=["text", "tiles216"])
def test_mutations_equal_the_walker_and_the_oracle(which, share, scratch):
    muts = C.mutations()[which]
    assert len(muts) == 2000
    comparable = 0
    for k, m in enumerate(muts):
        got = lz4mi.host_decoded_size(m)
        assert got == C.walk(m), k
        est, ew = oracle_size(m, scratch)
        if est in (0, -2, -3):                       # the rest depend on output positions (DICT_OOB)
            comparable += 1
            assert got[0] == est and (est != 0 or got[1] == ew), k   # (no `written` with an error)
    print("comparable share:", comparable / len(muts))
    assert comparable >= share * len(muts)


def _hand_built():
    cases = {
        "empty": b"",
        "00": b"\x00",
        "literals_only_last": C.seq(5, 8, 3) + C.seq(7),
        "ends_after_match": C.seq(5, 8, 3) + C.seq(0, 20, 1),
        "long_literal_last": C.seq(5000),
        "malformed_literals": C.seq(3, 4, 1) + b"\x90abc",
        "offset0": C.seq(3, 4, 1) + C.seq(2, 9, 0) + C.seq(4),
        "offset_cut": C.seq(3, 4, 1) + b"\x10a\x05",
        "offset_cut_zero": C.seq(3, 4, 1) + b"\x10a\x00",
        "match_field_cut": C.seq(3, 4, 1) + b"\x1fa\x01\x00\xff\xff",
        "literal_field_cut": C.seq(3, 4, 1) + b"\xf0\xff\xff",
    }
    for k in (1, 2, 5, 300):
        cases[f"literal_ext{k}"] = C.seq(2, 6, 2) + C.seq(C.ext_len(k), 5, 1) + C.seq(3)
        cases[f"match_ext{k}"] = C.seq(2, 6, 2) + C.seq(1, C.ext_len(k) + 4, 1) + C.seq(3)
        cases[f"both_ext{k}_last"] = C.seq(C.ext_len(k), C.ext_len(k) + 4, 7)
    return cases


@pytest.mark.parametrize("name", sorted(_hand_built()))
def test_hand_built_streams(name):
    comp = _hand_built()[name]
    want = C.walk(comp)
    assert lz4mi.host_decoded_size(C.arr(comp)) == want, name
    if name in ("empty", "00"):
        assert want == (0, 0)
    if name == "malformed_literals":
        assert want == (-2, 7)
    if name == "offset0":
        assert want == (-3, 9)


def test_total_above_the_largest_block_is_output_too_small():
    comp = b"\x1fa\x01\x00" + b"\xff" * (17 << 19)   # one literal, offset 1, 8.5 MiB of extension bytes
    assert C.walk(comp) == (-1, 0x7FFFFFFF)
    assert lz4mi.host_decoded_size(C.arr(comp)) == (lz4mi.ERR_OUTPUT_TOO_SMALL, 0x7FFFFFFF)


def test_positions_inside_a_larger_array():
    """in_off / in_size select the block; with in_total == in_off + in_size bytes past it read 0."""
    a, b = C.base_blocks()
    both = np.concatenate([a, b])
    assert lz4mi.host_decoded_size(both, 0, a.size) == (0, 8192)
    assert lz4mi.host_decoded_size(both, a.size) == (0, 8192)
    assert lz4mi.host_decoded_size(both, a.size, 0) == (0, 0)


def test_abi_argument_checks():
    L = lz4mi.lib()
    buf = np.zeros(16, dtype=np.uint8)
    assert L.lz4mi_host_decoded_size(buf.ctypes.data, 16, 0, 16, None) == lz4mi.ERR_ARG
    st = ctypes.c_int32(0)
    assert L.lz4mi_host_decoded_size(buf.ctypes.data, 16, -1, 16, ctypes.addressof(st)) == lz4mi.ERR_ARG
    off = np.zeros(1, dtype=np.uint64)
    ln = np.array([16], dtype=np.uint32)
    out_len = np.zeros(1, dtype=np.uint32)
    status = np.zeros(1, dtype=np.int32)
    # checked before any device is touched: a NULL status, decode-only flags
    assert L.lz4mi_decoded_sizes(buf.ctypes.data, off.ctypes.data, ln.ctypes.data, out_len.ctypes.data, None, 1, 0,
                                 None) == lz4mi.ERR_ARG
    for flag in (lz4mi.JS_COMPAT, lz4mi.JS_EXACT, lz4mi.BLOCK_CHECKSUM, lz4mi.XXH_STANDARD):
        assert L.lz4mi_decoded_sizes(buf.ctypes.data, off.ctypes.data, ln.ctypes.data, out_len.ctypes.data,
                                     status.ctypes.data, 1, flag, None) == lz4mi.ERR_ARG
