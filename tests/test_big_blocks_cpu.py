"""The claims tests/test_gpu_big_blocks.py rests on (tests/big_blocks_common.py), checked without a GPU: the
hand-assembled blocks decode, on the CPU oracle, to the image the construction names, in spec and in reference mode;
the reference-mode cases change bytes; and the host decoder and the host size walker agree, up to the last block size
the ABI allows (LZ4MI_MAX_BLOCK = 2^31 - 1)."""
import numpy as np
import pytest

import big_blocks_common as B
import oracle as O

lz4mi = pytest.importorskip("lz4mi")

T27 = 1 << 27


def _full(blk, js):
    st, w, out = O.decompress_block(blk.comp, blk.n, js_compat=js)
    assert st == 0 and w == blk.n, (blk.name, st, w)
    return out


@pytest.mark.parametrize("js", [False, True], ids=["spec", "js_compat"])
@pytest.mark.parametrize("per", B.PERIODS)
@pytest.mark.parametrize("kind", B.KINDS)
def test_construction_claim_small(kind, per, js):
    """np.resize(literals, target) + the body decoded behind a 64 KiB window == the oracle's decode of the whole
    block, at target ~ 2^20."""
    blk = B.small_block(kind, per, B.KINDS.index(kind))
    got = _full(blk, js)
    want = blk.image(js)
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, (blk.name, js, int(bad[0]), blk.where(int(bad[0])))


@pytest.fixture(scope="module")
def at_2_27():
    """The blocks of the 2^27 case with the oracle's full decode in both modes (computed once, left unchanged)."""
    rows = []
    for blk in B.case("2^27"):
        rows.append((blk, {js: _full(blk, js) for js in (False, True)}))
    return rows


def test_construction_claim_at_2_27(at_2_27):
    for blk, full in at_2_27:
        for js in (False, True):
            assert np.array_equal(full[js][blk.target:], blk.tail(js)), (blk.name, js)
            k = blk.target // blk.per
            assert np.array_equal(full[js][:k * blk.per].reshape(k, blk.per), np.broadcast_to(B.literals(blk.per), (k, blk.per)))
            assert np.array_equal(full[js][k * blk.per:blk.target], B.literals(blk.per)[:blk.target - k * blk.per])


@pytest.mark.parametrize("spec", [True, False], ids=["spec", "reference"])
def test_host_decoder_at_2_27(at_2_27, spec):
    for blk, full in at_2_27:
        out = np.zeros(blk.n, dtype=np.uint8)
        n = lz4mi.host_decompress_raw(blk.comp, 0, blk.comp.size, out, 0, spec=spec)
        assert n == blk.n, (blk.name, n)
        bad = np.nonzero(out != full[not spec])[0]
        assert bad.size == 0, (blk.name, spec, int(bad[0]), blk.where(int(bad[0])))


@pytest.mark.parametrize("name", list(B.CASES) + ["top"])
def test_placement_and_host_sizes(name):
    """Every case lies where its name says, and the host walker measures (0, n) -- at the top edge n = 2^31 - 1."""
    B.check_case(name)
    for blk in B.case(name):
        assert lz4mi.host_decoded_size(blk.comp) == (0, blk.n), blk.name
    if name == "top":
        assert all(blk.n == B.MAX_BLOCK for blk in B.case(name))


def test_one_byte_past_the_limit():
    blk = B.too_long()
    assert blk.n == 1 << 31
    assert lz4mi.host_decoded_size(blk.comp) == (lz4mi.ERR_OUTPUT_TOO_SMALL, 0x7FFFFFFF)
    # (the same edit on a small block is a valid block one byte longer, so the edit itself is sound)
    small = B.Block(B.TOP[0][0], B.TOP[0][1], (1 << 20) + 3, longer=True)
    st, w, out = O.decompress_block(small.comp, small.n)
    assert st == 0 and w == small.n and np.array_equal(out[small.target:-1], small.body_src) and out[-1] == 0x5A


@pytest.mark.parametrize("kind", ["text", "copy"])
def test_reference_mode_is_not_vacuous(kind):
    """The reference's tail rewrite changes bytes of these bodies, none below them (Block.tail asserts the latter):
    a reference-mode decode that equals the spec decode would fail the GPU test."""
    for name in list(B.CASES) + ["top"]:
        for blk in B.case(name):
            if blk.kind == kind:
                assert np.array_equal(blk.tail(False), blk.body_src), blk.name
                changed = int((blk.tail(True) != blk.body_src).sum())
                assert changed > 1000, (blk.name, changed)


def test_filler_block():
    src, comp = B.filler()
    assert src.size == B.FILLER_N and lz4mi.host_decoded_size(comp) == (0, B.FILLER_N)
