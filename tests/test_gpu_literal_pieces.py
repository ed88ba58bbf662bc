"""The decoder's literal output and the edge of its staged window (csrc/lz4mi_decompress.hip:
dealt_literals, short_literals, the cut sequence) on the hand-assembled blocks of
literal_pieces_common: bytes, status and out_len against the CPU oracle in spec and js_exact mode,
through the small-batch path (1 and 3 blocks) and the batch kernel (SMALL_BLOCKS + 8 copies); and
the blocks packed at odd output offsets in an arena of known bytes, which must come back unchanged
outside the decoded bytes (a last piece that spills, a first piece that starts early)."""
import numpy as np
import pytest

import footprint_common as F
import literal_pieces_common as C
from test_gpu_seqtable import _check


@pytest.mark.gpu
@pytest.mark.parametrize("js", [False, True], ids=["spec", "js_exact"])
def test_small_batch_path(js):
    lz4mi = pytest.importorskip("lz4mi")
    lz4mi.init(0)
    for name, (comp, cap, opts, ref) in C.all_cases().items():
        st, outs, lens = lz4mi.decompress_blocks([comp], [cap], js_exact=js)
        _check(lz4mi, name, comp, cap, ref, js, st[0], outs[0], lens[0])
        st, outs, lens = lz4mi.decompress_blocks([comp] * 3, [cap] * 3, js_exact=js)
        for j in range(3):
            _check(lz4mi, name, comp, cap, ref, js, st[j], outs[j], lens[j], batched_at=j * cap)


@pytest.mark.gpu
@pytest.mark.parametrize("js", [False, True], ids=["spec", "js_exact"])
def test_batch_kernel(js):
    lz4mi = pytest.importorskip("lz4mi")
    lz4mi.init(0)
    copies = lz4mi.SMALL_BLOCKS + 8
    for name, (comp, cap, opts, ref) in C.all_cases().items():
        st, outs, lens = lz4mi.decompress_blocks([comp] * copies, [cap] * copies, js_exact=js)
        for j in range(copies):
            _check(lz4mi, name, comp, cap, ref, js, st[j], outs[j], lens[j], batched_at=j * cap)


def _packed(mode, count):
    """The valid blocks in turn, `count` of them, each in a slot of exactly its decoded size: at
    odd offsets with a guard between two slots, every third one directly behind its predecessor."""
    cs = [(n, c) for n, c in C.all_cases().items() if "want" not in c[2]]
    picks = [cs[k % len(cs)] for k in range(count)]
    return F.Batch(f"literal_pieces_{count}", [c[0] for _, c in picks], [c[1] for _, c in picks], mode=mode,
                   contiguous=tuple(range(2, count, 3)))


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["spec", "js_exact"])
@pytest.mark.parametrize("path", ["small", "batch"])
def test_packed_at_odd_offsets_leave_the_guards(path, mode):
    lz4mi = pytest.importorskip("lz4mi")
    lz4mi.init(0)
    count = 3 if path == "small" else max(lz4mi.SMALL_BLOCKS + 8, len(C.all_cases()))
    if path == "small":
        cs = C.all_cases()
        names = ("final_17", "final_33_after_run", "ladder_all", "edge_1000_1089_ends", "max_runs", "final_40")
        for k in range(0, len(names), 3):
            b = F.Batch(f"literal_pieces_small{k}", [cs[n][0] for n in names[k:k + 3]], [cs[n][1] for n in names[k:k + 3]],
                        mode=mode, contiguous=(2,))
            st = F.check_batch(b, lambda bt, run: F.dev_decode(lz4mi, bt, run))
            assert all(s == 0 for s in st), st
        return
    b = _packed(mode, count)
    st = F.check_batch(b, lambda bt, run: F.dev_decode(lz4mi, bt, run))
    assert all(s == 0 for s in st), st
