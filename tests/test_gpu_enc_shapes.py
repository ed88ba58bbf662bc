"""The encoder shapes of tests/enc_shapes_common.py on the GPU: the batch encoder with its table in
LDS and in global memory (compress_block_gts), through host and device pointers, and the chain kernel
(compress_block_chain) behind lz4mi_compress_chain and lz4mi_compress_block_table. Every comparison
is bit-exact against the CPU oracle (pinned to the reference on these very cases by
tests/test_enc_shapes_cpu.py::test_reference_pin); there are no tolerances. What each family reaches in
the kernels is in the common module's docstring and claims.

Run on a real MI355X: python -m pytest tests/test_gpu_enc_shapes.py -m gpu
"""
import numpy as np
import pytest

import enc_shapes_common as E
import oracle as O
from footprint_common import layout

lz4mi = pytest.importorskip("lz4mi")

pytestmark = pytest.mark.gpu

GLOBAL_TABLE_BLOCKS = 769     # above kLdsTableMaxBlocks (768): the tables in global memory (GtsShared)
FILL = 77


@pytest.fixture(scope="module", autouse=True)
def _device():
    lz4mi.init(0)


def _batch():
    """Families A to E as independent blocks (all start at 0 with a fresh table)."""
    cases = E.all_cases("ABCDE")
    assert all(c.start == 0 and c.table is None and c.block_size is None for c in cases)
    return cases, [c.src[:c.len] for c in cases], [E.expected(c.name)[0][0] for c in cases]


def _same(case, block, got, want):
    assert got.size == want.size and np.array_equal(got, want), E.explain(case, block, got, want)


@pytest.mark.parametrize("table", ["lds", "global"])
def test_batch_encoder(table):
    """A to E in one lz4mi_compress_blocks call; `global` pads the call with empty blocks to 769,
    which takes the kernel with the 15-bit tables in global memory. Bytes and lengths == the
    oracle's, and the result decodes to the sources."""
    cases, srcs, wants = _batch()
    pad = GLOBAL_TABLE_BLOCKS - len(srcs) if table == "global" else 0
    assert len(srcs) <= 768 and pad >= 0
    comps = lz4mi.compress_blocks(srcs + [np.zeros(0, dtype=np.uint8)] * pad)
    assert len(comps) == len(srcs) + pad
    for c, got, want in zip(cases, comps, wants):
        _same(c, 0, got, want)
    for got in comps[len(srcs):]:
        assert got.tolist() == [0]
    st, outs, _ = lz4mi.decompress_blocks(comps[:len(srcs)], [s.size for s in srcs])
    assert (st == 0).all()
    for c, s, o in zip(cases, srcs, outs):
        assert np.array_equal(s, o), c.name


def test_batch_encoder_device_pointers():
    """The same cases through lz4mi_compress_blocks with device pointers: the input blocks at
    offsets congruent to 1, 5 and 15 (mod 16), output slots of exactly the bound, sentinels behind
    out_len[nblocks). The whole output array == the image the oracle gives."""
    torch = pytest.importorskip("torch")
    cases, srcs, wants = _batch()
    n = len(srcs)
    in_off = layout([s.size for s in srcs], guard=48, page=-1)
    assert {o % 16 for o in in_off} == {1, 5, 15}
    arena = np.full(in_off[-1] + srcs[-1].size + 64, 0xA5, dtype=np.uint8)
    for o, s in zip(in_off, srcs):
        arena[o:o + s.size] = s
    bounds = [lz4mi.compress_bound(s.size) for s in srcs]
    out_off = layout(bounds, guard=48, page=-1)
    image = np.full(out_off[-1] + bounds[-1] + 64, FILL, dtype=np.uint8)
    dev = lambda a, dt: torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=dt))).cuda()
    d_in, d_out = dev(arena, np.uint8), dev(image, np.uint8)
    d_ioff, d_ilen, d_ooff = dev(in_off, np.int64), dev([s.size for s in srcs], np.int32), dev(out_off, np.int64)
    d_len = torch.full((n + 64,), FILL, dtype=torch.int32, device="cuda")
    lz4mi.compress_blocks_dev(d_in.data_ptr(), d_ioff.data_ptr(), d_ilen.data_ptr(), d_out.data_ptr(), d_ooff.data_ptr(),
                              d_len.data_ptr(), n, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    lens, out = d_len.cpu().numpy(), d_out.cpu().numpy()
    assert (lens[n:] == FILL).all(), "a sentinel behind out_len[nblocks) was written"
    for c, o, ln, want in zip(cases, out_off, lens, wants):
        _same(c, 0, out[o:o + int(ln)], want)
        image[o:o + want.size] = want
    assert np.array_equal(out, image), "bytes outside the blocks' [off, off + len) changed"
    assert np.array_equal(d_in.cpu().numpy(), arena), "the input changed"


def _chain(c, block_size):
    """One lz4mi_compress_chain call against the oracle's carried-table loop."""
    blocks, want_t = E.expected(c.name) if block_size == c.block_size else E.oracle_run(c, block_size)
    t = np.zeros(16384, dtype=np.int32) if c.table is None else c.table.copy()
    got = lz4mi.compress_chain(c.src, c.start, c.len, block_size or max(c.len, 1), t)
    assert len(got) == (len(blocks) if c.len else 0), c.name
    for b, (g, w) in enumerate(zip(got, blocks)):
        _same(c._replace(block_size=block_size), b, g, w)
    bad = np.nonzero(t != want_t)[0]
    assert bad.size == 0, (c.name, "table slot", int(bad[0]), int(t[bad[0]]), int(want_t[bad[0]]), bad.size)


@pytest.mark.parametrize("fam", "ABCDEG")
def test_chain_kernel(fam):
    """A to E each as one lz4mi_compress_chain call with block_size = len, G with its block sizes:
    every block's bytes and the final table == the oracle's carried-table loop."""
    for c in E.families()[fam].cases:
        _chain(c, c.block_size)


def test_caller_tables():
    """Family F through lz4mi_compress_block_table with room for the bound (its GPU route) and
    through lz4mi_compress_chain, as one block and as three: the output, the return value and all
    16384 table slots == the oracle's."""
    for c in E.families()["F"].cases:
        (want,), want_t = E.expected(c.name)
        out = np.full(lz4mi.compress_bound(c.len) + 7, FILL, dtype=np.uint8)
        t = c.table.copy()
        n = lz4mi.compress_raw(c.src, out, c.start, c.len, t, 7)
        assert n == want.size, (c.name, n, want.size)
        _same(c, 0, out[7:7 + n], want)
        assert (out[:7] == FILL).all() and (out[7 + n:] == FILL).all(), c.name
        bad = np.nonzero(t != want_t)[0]
        assert bad.size == 0, (c.name, "table slot", int(bad[0]), int(t[bad[0]]), int(want_t[bad[0]]), bad.size)
        _chain(c, None)
        _chain(c, c.len // 3 + 1)
