"""LZ4MI_FRAMES_CHAINS on the host twins (lz4mi_host_frames_plan / lz4mi_host_frames_compress, include/lz4mi.h):
dependent frames of more than one block, one table carried across a frame's blocks, against the oracle's frames
(LZ4.compress with blockIndependence = false) and a closed-form plan, on the zoo of tests/frames_chain_common.py.
No GPU needed."""
import os

import numpy as np
import pytest

import frames_chain_common as C
import lz4mi

GUARD = 0xA5
DEP, CH, PACKED = lz4mi.FRAMES_DEPENDENT, getattr(lz4mi, "FRAMES_CHAINS", 0x10000), lz4mi.FRAMES_PACKED
ALL = (True, True, True)


def flags_of(combo, packed=False, chains=True):
    csum, sized, bsum = combo
    return (lz4mi.frames_enc_flags(False, csum, sized, bsum, packed=packed) | (CH if chains else 0))


def plan(group, fill, combo, cap=None, packed=False, chains=True):
    a, off, ln = C.arena(group, fill)
    cap = C.need_blocks(group) if cap is None else cap
    return lz4mi.host_frames_plan(off, ln, C.GROUPS[group][0], cap, flags_of(combo, packed, chains)), a, off, ln


def compress_packed(group, fill, combo):
    p, a, off, ln = plan(group, fill, combo, packed=True)
    out = np.full(int(p["totals"][2]) + 64, GUARD, dtype=np.uint8)
    fi = lz4mi.host_frames_compress(a, p, out[:int(p["totals"][2])], flags_of(combo, True))
    return fi, out, p


def test_zoo_claims_hold_on_the_oracle():
    C.shapes()
    for group in C.GROUPS:
        a, off, ln = C.arena(group, 0)
        assert [int(o) % 16 for o in off] == [C.RESIDUES[k % 4] for k in range(off.size)]
        assert C.chain_names(group)
    assert int(C.arena("c64k", 0)[1][C.GROUPS["c64k"][2].index("tiles300k")]) % 16 != 0


@pytest.mark.parametrize("group", C.GROUPS)
@pytest.mark.parametrize("combo", C.COMBOS, ids=C.combo_id)
def test_packed_frames_are_the_oracles(group, combo):
    _, bs, names = C.GROUPS[group]
    outs = []
    for fill in C.FILLS:
        fi, out, p = compress_packed(group, fill, combo)
        assert not fi[:, 7].any(), fi[:, 7].tolist()
        at = 0
        for k, name in enumerate(names):
            want = C.expected(name, bs, combo)
            assert fi[k, 3] == want.size and fi[k, 5] == at, (name, fi[k].tolist())
            assert np.array_equal(out[at:at + want.size], want), name
            assert want.size <= lz4mi.frame_bound(C.content(name).size, bs), name
            at += want.size
        assert (out[at:] == GUARD).all() and at <= p["totals"][2]
        outs.append(out)
    assert np.array_equal(outs[0], outs[1])


@pytest.mark.parametrize("group", C.GROUPS)
@pytest.mark.parametrize("combo", C.COMBOS, ids=C.combo_id)
def test_slot_frames_are_the_oracles(group, combo):
    _, bs, names = C.GROUPS[group]
    wants = [C.expected(name, bs, combo) for name in names]
    caps = np.array([w.size for w in wants], dtype=np.uint64)   # every slot exactly its frame
    offs = (np.cumsum(caps + 48) - caps).astype(np.uint64)
    for fill in C.FILLS:
        p, a, off, ln = plan(group, fill, combo)
        out = np.full(int(offs[-1] + caps[-1]) + 64, GUARD, dtype=np.uint8)
        fi = lz4mi.host_frames_compress(a, p, out, flags_of(combo), slots=(offs, caps))
        assert not fi[:, 7].any() and fi[:, 5].tolist() == offs.tolist() and fi[:, 3].tolist() == caps.tolist()
        for k, want in enumerate(wants):
            lo = int(offs[k])
            assert np.array_equal(out[lo:lo + want.size], want), names[k]
            assert (out[lo + want.size:lo + want.size + 48] == GUARD).all(), names[k]


def test_flag_needs_dependent_and_belongs_to_the_encoder_only():
    L = lz4mi.lib()
    a, off, ln = C.arena("c64k", 0)
    n, cap = off.size, C.need_blocks("c64k")
    fi, tot = np.zeros(8 * n, dtype=np.int64), np.zeros(4, dtype=np.int64)
    lists = [np.zeros(cap, dtype=np.uint64), np.zeros(cap, dtype=np.uint32), np.zeros(cap, dtype=np.uint32),
             np.zeros(cap, dtype=np.uint64)]
    lp = [x.ctypes.data for x in lists]
    args = [off.ctypes.data, ln.ctypes.data, n, 65536, *lp, cap, fi.ctypes.data, tot.ctypes.data]
    D = lz4mi.DEVICE_PTRS
    assert L.lz4mi_host_frames_plan(*args, DEP | CH | PACKED) == 0 and tot[1] == cap
    work, out = np.zeros(int(tot[3]), dtype=np.uint8), np.zeros(int(tot[2]), dtype=np.uint8)
    cargs = [a.ctypes.data, *lp, cap, fi.ctypes.data, n, work.ctypes.data, work.size, out.ctypes.data, out.size,
             None, None]
    for extra in (0, PACKED, lz4mi.FRAMES_CONTENT_CHECKSUM | PACKED):
        assert L.lz4mi_host_frames_plan(*args, CH | extra) == lz4mi.ERR_ARG
        assert L.lz4mi_frames_plan(*args, D | CH | extra, None) == lz4mi.ERR_ARG
        assert L.lz4mi_host_frames_compress(*cargs, CH | PACKED | extra) == lz4mi.ERR_ARG
        assert L.lz4mi_frames_compress(*cargs, D | CH | PACKED | extra, None) == lz4mi.ERR_ARG
    assert L.lz4mi_host_frames_compress(*cargs, DEP | CH | PACKED) == 0 and not fi.reshape(n, 8)[:, 7].any()
    # the other batch calls do not know the flag
    z = np.zeros(64, dtype=np.uint64)
    zp = z.ctypes.data
    assert L.lz4mi_decompress_blocks(zp, zp, zp, zp, zp, zp, None, 0, zp, zp, 1, D | CH, None) == lz4mi.ERR_ARG
    assert L.lz4mi_decompress_blocks(zp, zp, zp, zp, zp, zp, None, 0, zp, zp, 1, CH, None) == lz4mi.ERR_ARG
    assert L.lz4mi_frames_index(zp, zp, zp, 1, zp, zp, zp, zp, 1, zp, zp, D | CH, None) == lz4mi.ERR_ARG
    assert L.lz4mi_frames_decompress(zp, zp, zp, zp, zp, 1, zp, 1, zp, zp, zp, D | CH, None) == lz4mi.ERR_ARG


@pytest.mark.parametrize("combo", (ALL, (False, False, False)), ids=C.combo_id)
def test_plan_is_the_closed_form(combo):
    for group, (bm, bs, names) in C.GROUPS.items():
        need = C.need_blocks(group)
        for cap in (need, need - 1, need + 3):
            for chains in (True, False):
                p, a, off, ln = plan(group, 0, combo, cap, chains=chains)
                rows, totals, *lists = C.closed_form_plan(ln.tolist(), off.tolist(), bs, combo, cap, chains)
                assert p["finfo"].tolist() == rows and p["totals"].tolist() == totals, (group, cap, chains)
                for key, want in zip(("blk_in_off", "blk_len", "blk_frame", "blk_work_off"), lists):
                    assert p[key][:totals[1]].tolist() == want and not p[key][totals[1]:].any(), (group, key, cap)
        p, *_ = plan(group, 0, combo, need)
        assert not p["finfo"][:, 7].any() and p["totals"][0] == p["totals"][1] == need
    # the longest chain, and the first length that is too long for int32 positions: arithmetic on lengths alone
    lens, offs, bs = [300, 0x7FFFFFFE, 13, 0x7FFFFFFF, 2 * 4194304 + 5], [0, 1 << 32, 1 << 33, 1 << 34, 1 << 35], 4194304
    noc = (False,) + combo[1:]   # (0x7FFFFFFF is below the content checksum's 4 GiB limit either way)
    for c in (combo, noc):
        for cap in (517, 100):
            p = lz4mi.host_frames_plan(offs, lens, bs, cap, flags_of(c))
            rows, totals, *lists = C.closed_form_plan(lens, offs, bs, c, cap)
            assert p["finfo"].tolist() == rows and p["totals"].tolist() == totals, cap
            for key, want in zip(("blk_in_off", "blk_len", "blk_frame", "blk_work_off"), lists):
                assert p[key][:totals[1]].tolist() == want, (key, cap)
            # (a frame behind one that does not fit does not fit either: the scan has counted its blocks)
            late = 0 if cap == 517 else C.CAP_BLOCKS
            assert p["finfo"][:, 7].tolist() == [0, late, late, C.DEPENDENT, late]
            assert p["finfo"][1, 6] == 512 and p["totals"][0] == 1 + 512 + 1 + 3


def test_plan_with_the_flag_and_compress_without_it():
    _, bs, names = C.GROUPS["c64k"]
    p, a, off, ln = plan("c64k", 0, ALL, packed=True)
    assert not p["finfo"][:, 7].any()
    out = np.full(int(p["totals"][2]) + 64, GUARD, dtype=np.uint8)
    fi = lz4mi.host_frames_compress(a, p, out[:int(p["totals"][2])], flags_of(ALL, True, chains=False))
    at = 0
    for k, name in enumerate(names):
        if len(C.SHAPES[name]) > 1:
            assert fi[k, 7] == C.DEPENDENT, name
            continue
        want = C.expected(name, bs, ALL)
        assert fi[k, 7] == 0 and fi[k, 5] == at and np.array_equal(out[at:at + want.size], want), name
        at += want.size
    assert (out[at:] == GUARD).all() and (fi[:, 7] == C.DEPENDENT).sum() == len(C.chain_names("c64k"))


def test_plan_without_the_flag_and_compress_with_it():
    _, bs, names = C.GROUPS["c64k"]
    p, a, off, ln = plan("c64k", 0, ALL, packed=True, chains=False)
    declined = [len(C.SHAPES[n]) > 1 for n in names]
    assert (p["finfo"][:, 7] == C.DEPENDENT).tolist() == declined
    out = np.full(int(p["totals"][2]) + 64, GUARD, dtype=np.uint8)
    fi = lz4mi.host_frames_compress(a, p, out[:int(p["totals"][2])], flags_of(ALL, True))
    assert (fi[:, 7] == C.DEPENDENT).tolist() == declined and not fi[~np.array(declined), 7].any()
    at = sum(C.expected(n, bs, ALL).size for n, d in zip(names, declined) if not d)
    assert (out[at:] == GUARD).all()


def test_out_total_one_byte_short_of_the_last_chain():
    _, bs, names = C.GROUPS["c64k"]
    assert len(C.SHAPES[names[-1]]) > 1
    lens = np.array([C.expected(n, bs, ALL).size for n in names])
    total = int(lens.sum())
    p, a, off, ln = plan("c64k", 0, ALL, packed=True)
    out = np.full(total + 64, GUARD, dtype=np.uint8)
    fi = lz4mi.host_frames_compress(a, p, out[:total - 1], flags_of(ALL, True))
    assert fi[:-1, 7].tolist() == [0] * (len(names) - 1) and fi[-1, 7] == C.OUT_CAP
    assert (fi[:-1, 5] == np.cumsum(lens)[:-1] - lens[:-1]).all()
    assert (out[total - int(lens[-1]):] == GUARD).all()
    at = 0
    for name in names[:-1]:
        want = C.expected(name, bs, ALL)
        assert np.array_equal(out[at:at + want.size], want), name
        at += want.size


def test_work_too_small_is_an_argument_error():
    p, a, off, ln = plan("c64k", 0, ALL, packed=True)
    out = np.zeros(int(p["totals"][2]), dtype=np.uint8)
    for short in (int(p["totals"][3]) - 1, 15):
        with pytest.raises(lz4mi.Lz4miError) as e:
            lz4mi.host_frames_compress(a, p, out, flags_of(ALL, True), work=np.zeros(short, dtype=np.uint8))
        assert e.value.status == lz4mi.ERR_ARG


def test_constant_is_declared():
    with open(os.path.join(os.path.dirname(lz4mi.PKG_DIR), "include", "lz4mi.h")) as f:
        header = f.read()
    assert "#define LZ4MI_FRAMES_CHAINS 0x10000u" in header and lz4mi.FRAMES_CHAINS == 0x10000
    assert lz4mi.frames_enc_flags(independent=False, chains=True) == DEP | lz4mi.FRAMES_CHAINS
    assert lz4mi.frames_enc_flags(independent=False) == DEP
