"""Hand-assembled dependent frames through the chain kernel of LZ4MI_FRAMES_CHAINS (lz4mi_frames_decompress): the
one-wave decoder with each block's sources in the bytes the block before has just written. The inputs and their
claims are tests/chain_blocks_common.py; the expected bytes and statuses are the CPU oracle's, cross-checked against
the single-frame call. One index call and one decode call per group of frames, fill byte and mode."""
import numpy as np
import pytest

import chain_blocks_common as B
import frames_chains_decode_common as D
import frames_common as C
from test_gpu_frames_chains_decode import MODES, alone, assert_untouched_outside, check_frames, run, slot

pytestmark = pytest.mark.gpu


def group_run(name, fill, exact, chains=True):
    assert B.claims()
    return run(B.arena(name, fill), fill, exact, True, chains=chains, measure=B.measured(name))


def check_group(name, fill, exact):
    r = group_run(name, fill, exact)
    frames = B.group(name)
    wrong, declined = [], 0
    for k, f in enumerate(frames):
        st, failed, out, wrote = B.want(f, exact)
        if f.kind == "measured" and st:
            # the header's contract: a measured frame with a failing block is declined (LAYOUT), whatever its
            # bytes inside the slot
            if not (r.result[k][1] == C.LAYOUT and 0 <= r.finfo[k, 3] <= f.total):
                wrong.append((f.name, "not declined LAYOUT", r.result[k]))
            declined += 1
            continue
        wst = st if st else D.want(f.data, exact, True)[0]
        assert wst == st or (st == 0 and wst == D.ERR_CHECKSUM and f.csum and exact), f.name
        if r.result[k] != (wst, 0):
            wrong.append((f.name, "status, decline", r.result[k], "want", (wst, 0)))
            continue
        if r.total[k] != f.total or r.finfo[k, 3] != wrote:
            wrong.append((f.name, "finfo[3]", int(r.finfo[k, 3]), "want", wrote))
        got = slot(r, k)
        bad = np.nonzero(got[:wrote] != out[:wrote])[0]
        if bad.size:
            wrong.append((f.name, "bytes", bad.size, "first at", int(bad[0]), "last at", int(bad[-1])))
        # after-failure rule: the failing block and the blocks behind it write nothing
        if not (got[wrote:] == fill).all():
            wrong.append((f.name, "written behind the failing block"))
    assert not wrong, (len(wrong), wrong[:12])
    # the oracle on the whole frame and the single-frame call. A frame of OVER_READ was checked above against the
    # bytes the header documents for the batch (a block ends where its size word says); the single-frame call
    # gives the reference's
    over = {k for k, f in enumerate(frames) if f.name in B.OVER_READ}
    assert check_frames(r, [f.data for f in frames], True, skip=over) == sum(1 for f in frames if not f.says.get("fails")) - len(over)
    for k in over:
        wst, wbytes = D.want(frames[k].data, exact, True)
        ast, abytes = alone(frames[k].data.tobytes(), exact, True)
        assert ast == wst == 0 and (abytes == wbytes).all(), frames[k].name
    assert declined == sum(1 for f in frames if f.kind == "measured" and f.says.get("fails"))
    # (the slots end at odd positions: the guard behind each and the next frame's first bytes are in this check)
    assert_untouched_outside(r, (name, fill, exact))
    assert r.off[r.live[0]] == 0 and len(r.live) == len(frames)


@MODES
@pytest.mark.parametrize("fill", D.FILLS)
@pytest.mark.parametrize("name", B.GROUPS)
def test_chain_blocks(name, fill, exact):
    check_group(name, fill, exact)


def test_without_the_flag_the_frames_are_declined():
    """chains=False, one call in the reference mode: the dependent frames, and the frames flagged independent whose
    named block reads below itself -- flagged_rewrite_64 through the reference's rewrite alone --, are declined
    DEPENDENT; so is errors_below_frame, whose block 1 reads the block before it (and on below the frame)."""
    r = group_run("measured", 0x00, True, chains=False)
    frames = B.group("measured")
    assert len(frames) == 15
    for k, f in enumerate(frames):
        assert r.result[k] == (0, C.DEPENDENT), (f.name, r.result[k])
    assert_untouched_outside(r, "no chains")


# ------------------------------------------------------------------- a lone block with history and a dictionary
def test_lone_block_over_the_callers_bytes_with_a_dictionary():
    """nblocks == 1 at out_off = 64 KiB + r (and 40 + r, reaching the dictionary): the default route. The cases
    boundary_oldest_r1 / _r7 / _r15 in the reference mode are the regression cases of the history that
    lz4mi_decompress_blocks stages for host pointers (65536 + 8 bytes in the reference modes: a rewrite of the bytes
    just below the block reads up to 65539 bytes below its start)."""
    assert B.lone_claims()
    wrong = B.lone_mismatches()
    assert not wrong, (len(wrong), wrong[:12])


def test_lone_block_with_a_dictionary_through_the_batch_kernel():
    """The same with LZ4MI_SMALL_SCRATCH_MB=0, where the batch kernel decodes the block: every case in one fresh
    process (the cap is read once per process)."""
    import os
    import subprocess
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    root = os.path.dirname(here)
    code = r"""
import os, sys
sys.path[:0] = [%r, os.path.join(%r, "oracle"), os.path.join(%r, "divortio-lz4_amd")]
import chain_blocks_common as B
wrong = B.lone_mismatches()
print(len(wrong), wrong[:12])
print("ok" if not wrong else "wrong")
""" % (here, root, root)
    r = subprocess.run([sys.executable, "-c", code], env={**os.environ, "LZ4MI_SMALL_SCRATCH_MB": "0"},
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.stdout[-2000:], r.stderr[-1500:])
