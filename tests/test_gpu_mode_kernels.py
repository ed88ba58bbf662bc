"""The batch kernel's two instantiations (csrc/lz4mi_decompress.hip: lz4mi_decompress_kernel for LZ4 spec,
lz4mi_decompress_ref_kernel for LZ4MI_JS_EXACT) and the short literal runs of the pre-loop pass
(dealt_literals), on the blocks of mode_kernels_common: status, out_len and bytes against the CPU oracle.

Device arrays lie inside sentinel margins, the slots are pre-filled and separated by guard bytes, status[] and
out_len[] hold sentinels before the call (test_gpu_rewrite_shapes' dev_call / check_batch, footprint_common's
arenas)."""
import numpy as np
import pytest

import footprint_common as F
import mode_kernels_common as M
import rewrite_shapes_common as X
import test_gpu_rewrite_shapes as R
from test_gpu_seqtable import _check

MODES = ["spec", "reference"]


# ------------------------------------------------------------------------------------------- kernel selection
@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
def test_batch_launch_takes_the_modes_kernel(mode):
    """SMALL_BLOCKS + 8 blocks (the batch kernel) whose two decodes differ: each mode gives its own oracle's
    bytes, and the rewrite that reads below its slot is ERR_CROSS_BLOCK in reference mode only."""
    lz4mi = pytest.importorskip("lz4mi")
    lz4mi.init(0)
    names = M.SELECT + (M.BELOW,)
    picks = [M.shape(names[j % len(names)]) for j in range(lz4mi.SMALL_BLOCKS + 8)]
    est = R.check_batch(lz4mi, R.dev_call, picks, mode)
    assert est[:len(names)] == [0, 0, 0, 0, X.CROSS if mode == "reference" else 0]


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
def test_lone_block_past_the_export_limits(mode):
    """A capacity of 4 MiB + 1: one wave of the export launch decodes the block in the caller's mode (the
    run-time flag), with history below it and with a dictionary."""
    lz4mi = pytest.importorskip("lz4mi")
    lz4mi.init(0)
    for name in M.LONE_HISTORY + M.LONE_DICTIONARY:
        R.check_lone(lz4mi, R.dev_call, M.shape(name), mode, R.BIG)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["spec", "js_exact"])
def test_frame_words_batch_with_a_stored_block(mode):
    """LZ4MI_FRAME_WORDS sends a batch of any size to the batch kernel: the selection shapes around a stored
    block of 100 bytes and one of 4099."""
    lz4mi = pytest.importorskip("lz4mi")
    lz4mi.init(0)
    rng = np.random.default_rng(13300)
    shapes = [M.shape(n) for n in M.SELECT]
    pays = [shapes[0].comp, rng.integers(0, 256, 100, dtype=np.uint8), shapes[1].comp, shapes[2].comp,
            rng.integers(0, 256, 4099, dtype=np.uint8), shapes[3].comp]
    caps = [shapes[0].cap, 100, shapes[1].cap, shapes[2].cap, 4100, shapes[3].cap]
    b = F.Batch("mode_kernels_frame_words", pays, caps, mode=mode, stored=[False, True, False, False, True, False],
                frame_words=True)
    st = F.check_batch(b, lambda bt, run: F.dev_decode(lz4mi, bt, run))
    assert st == [0] * 6


@pytest.mark.gpu
def test_small_batch_redo_launch_takes_the_reference_kernel():
    """Reference mode, a lone block on the small path whose rewrite changes bytes below its slot: the pointer pass
    hands it back through redo[], and the redo launch decodes it with the reference instantiation."""
    lz4mi = pytest.importorskip("lz4mi")
    lz4mi.init(0)
    for name in M.LONE_HISTORY:
        for call in (R.host_call, R.dev_call):
            R.check_lone(lz4mi, call, M.shape(name), "reference")
            R.check_lone(lz4mi, call, M.shape(name), "spec")


# --------------------------------------------------------------------------------------------- short literals
@pytest.mark.gpu
@pytest.mark.parametrize("js", [False, True], ids=["spec", "js_exact"])
def test_short_literals_small_path(js):
    lz4mi = pytest.importorskip("lz4mi")
    lz4mi.init(0)
    M.claims()
    for name, (comp, cap, says, ref) in M.all_cases().items():
        st, outs, lens = lz4mi.decompress_blocks([comp], [cap], js_exact=js)
        _check(lz4mi, name, comp, cap, ref, js, st[0], outs[0], lens[0])


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["spec", "js_exact"])
def test_short_literals_batch_kernel(mode):
    """Every case in turn, SMALL_BLOCKS + 8 blocks in one call, each in a slot of exactly its decoded size at an
    odd offset with a guard behind it (every third one directly behind its predecessor): the final literals end
    at the capacity, and the whole arena outside the decoded bytes comes back unchanged."""
    lz4mi = pytest.importorskip("lz4mi")
    lz4mi.init(0)
    cs = list(M.all_cases().values())
    count = lz4mi.SMALL_BLOCKS + 8
    picks = [cs[k % len(cs)] for k in range(count)]
    b = F.Batch("mode_kernels_short", [c[0] for c in picks], [c[1] for c in picks], mode=mode,
                contiguous=tuple(range(2, count, 3)))
    st = F.check_batch(b, lambda bt, run: F.dev_decode(lz4mi, bt, run))
    assert all(s == 0 for s in st), st


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["spec", "js_exact"])
def test_short_literals_small_batch_leaves_the_guards(mode):
    """Three blocks (the export path and its expand kernels) in slots of exactly their decoded size."""
    lz4mi = pytest.importorskip("lz4mi")
    lz4mi.init(0)
    cs = M.all_cases()
    for names in (("places_1", "places_15", "dense_row_cycle"), ("remap_15_c1", "list_flush", "places_8"),
                  ("list_flush_short", "remap_3_c1", "dense_row_ones"), ("slack_8_far", "slack_12_near", "places_3")):
        b = F.Batch("mode_kernels_small_" + names[0], [cs[n][0] for n in names], [cs[n][1] for n in names], mode=mode,
                    contiguous=(2,))
        st = F.check_batch(b, lambda bt, run: F.dev_decode(lz4mi, bt, run))
        assert st == [0, 0, 0], st
