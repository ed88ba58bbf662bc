"""Shared by tests/test_linked_exact_cpu.py and tests/test_gpu_linked_exact.py (LZ4MI_LINKED_EXACT,
include/lz4mi.h): the fixture tests/golden/linked_exact.json, the expected result -- the oracle's
reference-mode decoder (js_compat) run on the blocks in index order on one array -- and a NumPy
model of the kernels' pointer form."""
import json
import os

import numpy as np

import oracle as O

ERR_CROSS_BLOCK = -9
MESSAGES = {"LZ4: Output Buffer Too Small": -1, "LZ4: Malformed Input": -2, "LZ4: Invalid Offset 0": -3,
            "LZ4: Dictionary Offset Out of Bounds": -4}


def fixture_cases():
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "linked_exact.json")
    with open(path) as f:
        doc = json.load(f)
    out = []
    for c in doc["cases"]:
        h = lambda s: np.frombuffer(bytes.fromhex(s), dtype=np.uint8).copy()
        out.append({"name": c["name"], "blocks": [h(b) for b in c["blocks"]], "stored": list(c["stored"]),
                    "out_off": list(c["out_off"]), "out_cap": list(c["out_cap"]), "init": h(c["init"]),
                    "dict": None if c["dict"] is None else h(c["dict"]), "after": h(c["after"]),
                    "results": list(c["results"])})
    return out


def in_order(pay, out_off, out_cap, init, dictionary=None, stored=None, first=0, count=None):
    """The oracle's reference-mode decoder on blocks [first, first + count) in index order on one
    array (a copy of `init`); each call sees the array up to its slot's end. A stored block is
    copied. The contract's failure rule: the first failing block and every block after it write
    nothing and the later ones report ERR_CROSS_BLOCK. -> (statuses, lengths, array)."""
    out = np.array(init, dtype=np.uint8, copy=True)
    n = len(pay) if count is None else first + count
    st, ln, failed = [], [], False
    for b in range(first, n):
        off, cap = int(out_off[b]), int(out_cap[b])
        if failed:
            st.append(ERR_CROSS_BLOCK)
            ln.append(0)
            continue
        if stored is not None and stored[b]:
            if pay[b].size > cap:
                st.append(-8)
                ln.append(0)
                failed = True
                continue
            out[off:off + pay[b].size] = pay[b]
            st.append(0)
            ln.append(int(pay[b].size))
            continue
        trial = out.copy()
        s, w, _ = O.decompress_block(pay[b], cap, out=trial[:off + cap], out_off=off, dictionary=dictionary,
                                     js_compat=True)
        st.append(int(s))
        ln.append(int(w) if s == 0 else 0)
        if s == 0:
            out = trial
        else:
            failed = True
    return st, ln, out


def parse(comp):
    """The sequences (literal position, literal length, offset, match length) of a well-formed
    block; the last one may have offset 0 (no match)."""
    c = bytes(comp)
    p, n, seqs = 0, len(c), []
    while p < n:
        tok = c[p]
        p += 1
        ll = tok >> 4
        if ll == 15:
            while True:
                v = c[p]
                p += 1
                ll += v
                if v != 255:
                    break
        lp = p
        p += ll
        if p >= n:
            seqs.append((lp, ll, 0, 0))
            break
        off = c[p] | (c[p + 1] << 8)
        p += 2
        ml = tok & 15
        if ml == 15:
            while True:
                v = c[p]
                p += 1
                ml += v
                if v != 255:
                    break
        seqs.append((lp, ll, off, ml + 4))
    return seqs


def pointer_model(pay, out_off, init, dictionary=None, stored=None):
    """The pointer form of a linked reference-mode decode of valid blocks, as the kernels compute
    it: (1) every output byte of every block gets a pointer -- a literal or dictionary byte
    (final) or the position `offset` below it; (2) then every rewrite of the reference's tail
    copy (offset >= 8, match length < 8, source inside the array) overwrites the pointers of its
    region [s + ml - 8, s) with p - offset, those below the block's start -- in the predecessor or
    the caller's bytes -- included; applied LAST block first, since the argument says the order
    does not matter; (3) the pointers are resolved by jumping. -> the array."""
    init = np.asarray(init, dtype=np.uint8)
    n = init.size
    d = np.zeros(0, dtype=np.uint8) if dictionary is None else np.asarray(dictionary, dtype=np.uint8)
    pool = [init, np.zeros(1, dtype=np.uint8), d]
    zero, dbase, at = n, n + 1, n + 1 + d.size
    ptr = -(1 + np.arange(n, dtype=np.int64))            # negative: -(1 + pool index): a final byte
    rewrites = []
    for b, c in enumerate(pay):
        base = at
        pool.append(np.asarray(c, dtype=np.uint8))
        at += len(c)
        o = int(out_off[b])
        if stored is not None and stored[b]:
            ptr[o:o + len(c)] = -(1 + base + np.arange(len(c), dtype=np.int64))
            continue
        for lp, ll, off, ml in parse(c):
            ptr[o:o + ll] = -(1 + base + lp + np.arange(ll, dtype=np.int64))
            o += ll
            if not off:
                break
            x = np.arange(o, o + ml, dtype=np.int64)
            src = x - off
            ptr[o:o + ml] = np.where(src >= 0, src, -(1 + dbase + d.size + src))
            if off >= 8 and ml < 8 and o - off >= 0:
                rewrites.append((o, off, ml))
            o += ml
    for s, off, ml in reversed(rewrites):
        for p in range(max(0, s + ml - 8), s):
            ptr[p] = p - off if p - off >= 0 else -(1 + zero)
    for _ in range(64):
        un = np.nonzero(ptr >= 0)[0]
        if un.size == 0:
            break
        assert (ptr[un] < un).all()                      # every pointer points strictly lower
        ptr[un] = ptr[ptr[un]]
    assert not (ptr >= 0).any()
    return np.concatenate(pool)[-(ptr + 1)]


def dependent_blocks(data, sizes):
    """`data` cut into blocks of `sizes`, compressed in order with one carried table."""
    table = np.zeros(16384, dtype=np.int32)
    pay, pos = [], 0
    for n in sizes:
        w, out, table = O.compress_block(data, pos, n, table)
        pay.append(out[:w].copy())
        pos += n
    return pay
