"""Shared by tests/test_enc_shapes_cpu.py and tests/test_gpu_enc_shapes.py: encoder inputs BUILT to
reach the special machinery of the two encoder kernels (csrc/lz4mi_compress.hip) instead of meeting
it by accident: equal-step hit chains at the steps where the emission and the window paths change
(A), equal hashes inside one speculative batch at every lane distance (B), candidates at the window
edge 65535 / 65536 beside every 32 KiB epoch edge (C), table entries exactly four epochs old (D),
every way a block can end (E), caller tables with stale, future, negative and misplaced entries at
starts around 65536 (F) and dependent chains with tiny blocks and tiny last blocks (G).

Every family is (name, cases, claim, every, some). A case is (name, src, start, len, block_size or
None, table or None). claim(case) returns the set of tags the case earns, decided from the CPU
oracle alone (its compressBlock restatement, the table it returns, and the parse of its output):
`every` names the tags each case of the family must carry, `some` the (name prefix, tag) pairs at
least one case with that prefix must carry. Where a claim depends on the random filler the builder
moves its seed on until the claim holds (at most 32 moves, then it raises); no case is skipped.

The batch model behind the lane claims (B, E) restates the kernels' acceptance rule: after a hit of
step S the next up to 8 probes i, i+S, ... form one batch; a probe stays in it while it is a hit
that ends on the next probe (and is not the batch's last lane, nor a match that fills the 128-byte
window); the first probe that is not ends the batch.
"""
import collections
import functools
import json
import os

import numpy as np

import oracle as O
from linked_exact_common import parse

Case = collections.namedtuple("Case", "name src start len block_size table")
Family = collections.namedtuple("Family", "name cases claim every some")
META = {}                     # case name -> the builder's figures (P, Q, D, S, ...), read by the claims
MOVES = 32                    # seed moves before a builder gives up
STEPS = (4, 5, 8, 16, 19, 20, 64, 127, 128, 129, 273, 274, 300, 1000)
TILES = 12
DRAWS = 400
EDGE_D = (65534, 65535, 65536, 65537)
EDGE_K = (3, 4, 5)
EDGE_R = (-2, -1, 0, 1, 100)
STARTS = (0, 1) + tuple(range(65519, 65554)) + (100000,)
CHAIN_BLOCKS = (13, 64, 1000, 4096, 65536)
SPEC_K, SPEC_W = 8, 128       # kSpecK, kSpecW of csrc/lz4mi_compress.hip


# ------------------------------------------------------------------------------------ the oracle
def h4(src, p):
    """Math.imul(seq, 2654435761) >>> 18 of the 4 bytes at p."""
    v = int(src[p]) | int(src[p + 1]) << 8 | int(src[p + 2]) << 16 | int(src[p + 3]) << 24
    return ((v * 2654435761) & 0xFFFFFFFF) >> 18


def all_h4(src):
    """h4 at every position p <= len - 4, and the 4-gram values."""
    s = np.asarray(src, dtype=np.uint8).astype(np.uint64)
    v = s[:-3] | s[1:-2] << np.uint64(8) | s[2:-1] << np.uint64(16) | s[3:] << np.uint64(24)
    return (((v * np.uint64(2654435761)) & np.uint64(0xFFFFFFFF)) >> np.uint64(18)).astype(np.int64), v


def block_sizes(case):
    if case.block_size is None:
        return [case.len]
    return [min(case.block_size, case.len - p) for p in range(0, case.len, case.block_size)]


def oracle_run(case, block_size="case"):
    """The oracle's carried-table loop over the case's blocks -> (list of compressed blocks, final
    table). block_size None: one compressBlock call over [start, start + len), empty included."""
    bs = case.block_size if block_size == "case" else block_size
    table = np.zeros(16384, dtype=np.int32) if case.table is None else case.table.copy()
    blocks, pos = [], case.start
    for n in block_sizes(case._replace(block_size=bs)):
        w, out, table = O.compress_block(case.src, pos, n, table)
        blocks.append(out[:w].copy())
        pos += n
    return blocks, table


def matches_of(comp, start):
    """The matches of one block's parse in absolute source positions: [(mpos, ml, off, ll)]."""
    out, pos = [], start
    for _, ll, off, ml in parse(comp):
        if not off:
            break
        out.append((pos + ll, ml, off, ll))
        pos += ll + ml
    return out


def probes_of(ms, start, end):
    """Every probe of the parse in order, the miss chains' included: [(p, hit, match end)].
    Asserts that the matches sit where the reference's skip schedule can reach them."""
    out, i, c, mflimit = [], start, 67, end - 12
    for mpos, ml, _, _ in ms:
        while i < mpos:
            out.append((i, False, i))
            i += c >> 6
            c += 1
        assert i == mpos, (i, mpos)
        out.append((mpos, True, mpos + ml))
        i, c = mpos + ml, 67
    while i < mflimit:
        out.append((i, False, i))
        i += c >> 6
        c += 1
    return out


def hit_batches(pr, end, epochs):
    """The speculative hit batches the kernels form over the probes `pr` (module docstring):
    [(S, [probe positions, lane 0 first])]. epochs: the batch encoder's batches also stop at
    32 KiB epoch edges; the chain kernel's do not."""
    mflimit, matchlimit = end - 12, end - 5
    out, cur, S, K = [], None, 0, 0

    def lanes(i, S):
        lim = mflimit - 1 - i
        if epochs:
            lim = min(mflimit - 1, (((i >> 15) + 1) << 15) - 1) - i
        return min(SPEC_K, 1 + lim // S)

    for p, hit, e in pr:
        if cur is None:
            if hit:
                S, cur = e - p, []
                K = lanes(e, S)
            continue
        lane = len(cur)
        cur.append(p)
        lng = hit and e - p >= SPEC_W and p + SPEC_W < matchlimit
        if hit and not lng and lane + 1 < K and e == p + S:
            continue
        out.append((S, cur))
        if hit:
            S, cur = e - p, []
            K = lanes(e, S)
        else:
            cur = None
    if cur:
        out.append((S, cur))
    return out


def runs_of(ms):
    """Maximal runs of back-to-back matches (0 literals after the first) of equal length."""
    out = []
    for m in ms:
        if out and m[3] == 0 and m[1] == out[-1][-1][1]:
            out[-1].append(m)
        else:
            out.append([m])
    return out


def single_parse(case):
    """The parse of the case as ONE block with its table: (matches, probes, tags). The tag
    parse_ok: the oracle's block decodes to the source and every match sits on the skip schedule."""
    (comp,), _ = oracle_run(case, None)
    ms = matches_of(comp, case.start)
    pr = probes_of(ms, case.start, case.start + case.len)
    end = case.start + case.len
    out = np.zeros(end, dtype=np.uint8)
    out[:case.start] = case.src[:case.start]          # a caller's table may point below the block
    st, w, out = O.decompress_block(comp, case.len, out=out, out_off=case.start)
    ok = st == 0 and w == case.len and np.array_equal(out, case.src[:end])
    return ms, pr, ({"parse_ok"} if ok else set())


def settle(make, claim, need, seed, what):
    """make(seed) until claim(case) carries `need`, moving the seed at most MOVES times."""
    for move in range(MOVES + 1):
        case = make(seed + 7919 * move)
        if set(need) <= claim(case):
            return case
    raise AssertionError(f"{what}: the claim {sorted(need)} does not hold after {MOVES} seed moves")


# ------------------------------------------------------------------------ A: equal-step chains
def tile_stream(rng, S, shared=False, collide=False):
    tiles = rng.integers(0, 256, (TILES, S), dtype=np.uint8)
    if shared:      # tiles k and T-1-k: the same first 4 bytes, another byte 4
        for k in range(3):
            tiles[TILES - 1 - k, :4] = tiles[k, :4]
            tiles[TILES - 1 - k, 4] = tiles[k, 4] ^ 0x5A
    if collide:     # another 4-gram of the same hash (3983)
        tiles[0, :4] = (0x01, 0x02, 0x03, 0x04)
        tiles[TILES - 1, :4] = (0x99, 0x11, 0x00, 0x00)
    return tiles


def claim_A(case):
    """run1 .. run8, run9+: the parse has runs (runs_of) of each of these lengths, so chains end inside
    a batch at every lane and cross whole batches; steps: at least 250 matches of step S and 10 of 2S."""
    S = META[case.name]["S"]
    ms, _, tags = single_parse(case)
    lens = {len(r) for r in runs_of(ms)}
    tags |= {f"run{k}" for k in range(1, 9) if k in lens}
    if lens and max(lens) >= 9:
        tags.add("run9+")
    step = sum(1 for m in ms if m[1] == S)
    if step >= 250 and sum(1 for m in ms if m[1] == 2 * S) >= 10:
        tags.add("steps")
    return tags


EVERY_A = ("parse_ok", "steps", "run9+") + tuple(f"run{k}" for k in range(1, 9))


def family_A():
    cases = []
    for S in STEPS:
        name = f"A_S{S}"
        META[name] = {"S": S}

        def make(seed, S=S, name=name):
            rng = np.random.default_rng(seed)
            tiles = tile_stream(rng, S)
            idx = np.concatenate([np.arange(TILES), rng.integers(0, TILES, DRAWS)])
            if S < 8:    # (E) a match reaches from below mflimit to the limit only over two tiles
                idx[-4:] = idx[TILES:TILES + 4]
            src = tiles[idx].reshape(-1).copy()
            return Case(name, src, 0, src.size, None, None)

        # the streams family E cuts must also end in every way E claims (E_NEED)
        need = EVERY_A + tuple("cuts:" + t for t in E_NEED.get(S, ()))
        cases.append(settle(make, lambda c: claim_A(c) | cut_tags(c), need, 1000 + S, name))
    return Family("A", cases, claim_A, EVERY_A, ())


# ------------------------------------------------------- B: same-hash probes inside a batch
def claim_B(case):
    """d1 .. d7: one hit batch of step S (in the batch encoder's model and in the chain kernel's) has
    two probes d lanes apart with equal hashes and different tiles; variant: with the same 4 bytes
    (the later one matches 4 bytes: a step change in mid chain) or with another 4-gram (it misses);
    triple: three probes of one batch share a hash; step_changes: the shared prefixes do cut matches."""
    meta = META[case.name]
    S, src = meta["S"], case.src
    ms, pr, tags = single_parse(case)
    end = case.start + case.len
    per_model = []
    for epochs in (False, True):
        t = set()
        for bS, pos in hit_batches(pr, end, epochs):
            if bS != S:
                continue
            pos = [p for p in pos if p + S <= end]
            hs = [h4(src, p) for p in pos]
            for b in range(len(pos)):
                same = [a for a in range(b) if hs[a] == hs[b]]
                if len(same) >= 2:
                    t.add("triple")
                for a in same:
                    if not np.array_equal(src[pos[a]:pos[a] + S], src[pos[b]:pos[b] + S]):
                        t.add(f"d{b - a}")
                        gram = np.array_equal(src[pos[a]:pos[a] + 4], src[pos[b]:pos[b] + 4])
                        t.add("same_gram" if gram else "hash_only")
        per_model.append(t)
    tags |= per_model[0] & per_model[1]
    if meta["variant"] in tags:
        tags.add("variant")
    n4 = sum(1 for m in ms if m[1] == 4)
    if meta["variant"] == "hash_only" or (n4 >= 20 and (S < 8 or sum(1 for m in ms if m[1] == S - 4) >= 20)):
        tags.add("step_changes")
    return tags


EVERY_B = ("parse_ok", "variant", "triple", "step_changes") + tuple(f"d{d}" for d in range(1, 8))


def family_B():
    cases = []
    for variant in ("same_gram", "hash_only"):
        for S in STEPS:
            if S < 5 or S >= SPEC_W:      # a match that fills the 128-byte window ends its batch: one lane
                continue
            name = f"B_{'shared' if variant == 'same_gram' else 'collide'}_S{S}"
            META[name] = {"S": S, "variant": variant}

            def make(seed, S=S, name=name, variant=variant):
                rng = np.random.default_rng(seed)
                tiles = tile_stream(rng, S, shared=variant == "same_gram", collide=variant == "hash_only")
                pairs = [(k, TILES - 1 - k) for k in range(3)] if variant == "same_gram" else [(0, TILES - 1)]
                paired = {t for p in pairs for t in p}
                others = [t for t in range(TILES) if t not in paired]

                def some(n):     # n other tiles, no tile twice in a row
                    out = []
                    while len(out) < n:
                        t = int(rng.choice(others))
                        if not out or out[-1] != t:
                            out.append(t)
                    return out

                idx = list(range(TILES))
                for rep in range(3):
                    for d in range(1, 8):     # X, X, d-1 others, X': X' probes d lanes behind the X whose position it finds
                        x, xp = pairs[(d + rep) % len(pairs)]
                        if rng.random() < 0.5:
                            x, xp = xp, x
                        idx += some(int(rng.integers(1, 5))) + [x, x] + some(d - 1) + [xp]
                    x, xp = pairs[rep % len(pairs)]
                    idx += some(2) + [x, some(1)[0], x, some(1)[0], xp]     # three probes of one hash
                idx += [int(t) for t in rng.integers(0, TILES, max(0, TILES + DRAWS - len(idx)))]
                src = tiles[np.array(idx)].reshape(-1).copy()
                return Case(name, src, 0, src.size, None, None)

            cases.append(settle(make, claim_B, EVERY_B, 2000 + S, name))
    return Family("B", cases, claim_B, EVERY_B, ())


# ---------------------------------------------------------------------------- markers (C, D)
MARKER = 512


def marker(rng):
    """512 bytes of period 3 (three different bytes): wherever the miss chain enters it, a probe
    soon finds an earlier probe of the same phase inside it, and the match runs to the marker's
    end -- so the position behind a marker is probed. -> (bytes, the byte that would continue it)."""
    a, b, c = (int(x) for x in rng.choice(256, 3, replace=False))
    m = np.resize(np.array([a, b, c], dtype=np.uint8), MARKER)
    return m, int(m[MARKER % 3])


def after_marker(rng, cont, n=40):
    """n random bytes whose first one ends the marker's match."""
    u = rng.integers(0, 256, n, dtype=np.uint8)
    if int(u[0]) == cont:
        u[0] ^= 0x55
    return u


def slot_before(src, P, gram_at):
    """The oracle's table slot of the 4 bytes at gram_at when the parse reaches P (a chain call
    over src[0, P): it probes what the whole parse probes below the last match before P)."""
    _, _, table = O.compress_block(src, 0, P)
    return int(table[h4(src, gram_at)])


# ------------------------------------------------------------------------------ C: window edge
def claim_C(case):
    """probed: the parse probes at Q and at P. edge: for D <= 65535 the match at P has offset D and
    covers the 40 bytes; for D >= 65536 no match has offset D, none starts at P, and the slot of the
    bytes at Q still holds Q + 1 when the parse reaches P (so it is the distance that rejects)."""
    m = META[case.name]
    P, Q, D = m["P"], m["Q"], m["D"]
    ms, pr, tags = single_parse(case)
    probed = {p for p, _, _ in pr}
    at_P = [x for x in ms if x[0] == P]
    if Q in probed and P in probed:
        tags.add("probed")
        if D <= 65535 and at_P and at_P[0][2] == D and at_P[0][1] >= 40:
            tags.add("edge")
        if D >= 65536 and not any(x[2] == D for x in ms) and not at_P and slot_before(case.src, P, Q) == Q + 1:
            tags.add("edge")
    return tags


EVERY_C = ("parse_ok", "probed", "edge")


def family_C():
    cases = []
    for D in EDGE_D:
        for k in EDGE_K:
            for r in EDGE_R:
                P = k * 32768 + r
                Q = P - D
                name = f"C_D{D}_k{k}_r{r}"
                META[name] = {"P": P, "Q": Q, "D": D}

                def make(seed, P=P, Q=Q, name=name):
                    rng = np.random.default_rng(seed)
                    src = rng.integers(0, 256, P + 200, dtype=np.uint8)
                    M, cont = marker(rng)
                    src[64:64 + MARKER] = M
                    src[Q - MARKER:Q] = M
                    src[P - MARKER:P] = M
                    src[Q:Q + 40] = after_marker(rng, cont)
                    src[P:P + 40] = src[Q:Q + 40]
                    return Case(name, src, 0, src.size, None, None)

                cases.append(settle(make, claim_C, EVERY_C, 3000 + D + 11 * k + r, name))
    return Family("C", cases, claim_C, EVERY_C, ())


# ------------------------------------------------------------------------------ D: stale epoch
def claim_D(case):
    """Per planted pair (x, P = x + 131072 + d): the slot of the 4 bytes at P holds x + 1 when the
    parse reaches P (x is four epochs back), the bytes at x + 131072 equal those at P (what a
    decode into the current code cycle would compare), P is probed and no match starts there."""
    ms, pr, tags = single_parse(case)
    probed = {p for p, _, _ in pr}
    starts = {m[0] for m in ms}
    good = 0
    for x, P in META[case.name]["pairs"]:
        src = case.src
        assert (x >> 15) + 4 == (x + 131072) >> 15 and P > x + 131072
        good += int(P in probed and P not in starts and slot_before(src, P, P) == x + 1
                    and np.array_equal(src[x:x + 4], src[P:P + 4])
                    and np.array_equal(src[x + 131072:x + 131076], src[P:P + 4])
                    and h4(src, P - MARKER) != h4(src, P) and h4(src, P - MARKER + 1) != h4(src, P)
                    and h4(src, P - MARKER + 2) != h4(src, P))
    if good == len(META[case.name]["pairs"]):
        tags.add("stale")
    return tags


EVERY_D = ("parse_ok", "stale")


def family_D():
    cases = []
    q = 1024
    for d in (1, 4096, 65535):
        name = f"D_d{d}"

        def make(seed, d=d, name=name):
            rng = np.random.default_rng(seed)
            M, cont = marker(rng)
            if d == 1:
                # the alias q + 131072 = P - 1 overlaps P, so the 40 bytes are a run of the marker's
                # last byte; the probe at q misses, the one at q + 1 finds q: the slot's entry is
                # x = q + 1, and P = x + 131072 + 1
                U = np.full(40, M[MARKER - 1], dtype=np.uint8)
                x = q + 1
            else:
                U = after_marker(rng, cont)
                x = q
            P = x + 131072 + d
            src = rng.integers(0, 256, P + 200, dtype=np.uint8)
            src[q - MARKER:q] = M
            src[q:q + 40] = U
            if d != 1:
                src[q + 131072:q + 131072 + 40] = U
            src[P - MARKER:P] = M
            src[P:P + 40] = U
            META[name] = {"pairs": [(x, P)]}
            return Case(name, src, 0, src.size, None, None)

        cases.append(settle(make, claim_D, EVERY_D, 4000 + d, name))

    def make9(seed):
        # 9 epochs: patterns planted in epochs 0..3, each again four epochs on (+ d), the first
        # once more four epochs after that: entries age through two full code cycles
        rng = np.random.default_rng(seed)
        src = rng.integers(0, 256, 9 * 32768, dtype=np.uint8)
        pairs = []
        for k, d in enumerate((1000, 600, 5000, 20000)):
            M, cont = marker(rng)
            U = after_marker(rng, cont)
            chain = [k * 32768 + 5000]
            while chain[-1] + 131072 + d + 200 < src.size:
                chain.append(chain[-1] + 131072 + d)
            for j, p in enumerate(chain):
                src[p - MARKER:p] = M
                src[p:p + 40] = U
                if j:
                    src[chain[j - 1] + 131072:chain[j - 1] + 131072 + 40] = U
                    pairs.append((chain[j - 1], p))
        META["D_9epochs"] = {"pairs": pairs}
        assert len(pairs) >= 5
        return Case("D_9epochs", src, 0, src.size, None, None)

    cases.append(settle(make9, claim_D, EVERY_D, 4900, "D_9epochs"))
    return Family("D", cases, claim_D, EVERY_D, ())


# -------------------------------------------------------------------------------- E: block ends
def claim_E(case):
    """ends_at_limit: the last match ends at n - 5. last_first / last_mid / last_in_miss_batch: the
    block's last probe is lane 0 of a hit batch, a later lane, or a probe of the miss chain (the same
    in the batch encoder's model and the chain kernel's)."""
    ms, pr, tags = single_parse(case)
    end = case.start + case.len
    if ms and ms[-1][0] + ms[-1][1] == end - 5:
        tags.add("ends_at_limit")
    if pr:
        where = []
        for epochs in (False, True):
            lane = None
            for _, pos in hit_batches(pr, end, epochs):
                if pr[-1][0] in pos:
                    lane = pos.index(pr[-1][0])
            where.append("last_in_miss_batch" if lane is None else "last_first" if lane == 0 else "last_mid")
        if where[0] == where[1]:
            tags.add(where[0])
    return tags


# what the cuts of each stream must show between them (a match of 128 bytes or more fills the
# window and ends its batch, so the S = 129 stream has one-lane batches only)
E_NEED = {5: ("ends_at_limit", "last_first", "last_mid"), 64: ("ends_at_limit", "last_first", "last_mid"),
          129: ("ends_at_limit", "last_first")}


def cuts_of(case):
    """The stream of an A case cut at n = N0 - r for every r in 0 .. S + 12."""
    S = META[case.name]["S"]
    return [Case(f"E_S{S}_r{r}", case.src[:case.len - r], 0, case.len - r, None, None) for r in range(0, S + 13)]


def cut_tags(case):
    if META[case.name]["S"] not in E_NEED:
        return set()
    return {"cuts:" + t for c in cuts_of(case) for t in claim_E(c)}


def family_E(A):
    cases, some = [], []
    by = {c.name: c for c in A.cases}
    for S in sorted(E_NEED):
        cases += cuts_of(by[f"A_S{S}"])
        some += [(f"E_S{S}_", t) for t in E_NEED[S]]
    for n in range(33):
        cases.append(Case(f"E_zeros_{n}", np.zeros(n, dtype=np.uint8), 0, n, None, None))
        cases.append(Case(f"E_ramp_{n}", np.arange(n, dtype=np.uint8), 0, n, None, None))
        cases.append(Case(f"E_per3_{n}", np.resize(np.array([7, 200, 31], dtype=np.uint8), n), 0, n, None, None))
    some += [("E_zeros_", "ends_at_limit"), ("E_per3_", "ends_at_limit")]
    return Family("E", cases, claim_E, ("parse_ok",), tuple(some))


# ------------------------------------------------------------------------------ F: caller tables
CATEGORIES = ("zero", "negative", "int32_min", "int32_max", "anywhere", "near_start", "future", "self",
              "foreign_prewarm", "true_stale")
F_LEN = 40000


def foreign_hash(v):
    """Another 14-bit hash of a 4-gram than the encoder's: entries filed under it sit in wrong buckets."""
    v = (v ^ (v >> np.uint64(15))) * np.uint64(2246822519) & np.uint64(0xFFFFFFFF)
    return (v >> np.uint64(18)).astype(np.int64)


def caller_table(rng, src, start, length, hs, vs):
    """One table for compressBlock(src, out, start, length, table, 0), each slot from a category
    drawn at random -> (table, the slots' categories)."""
    cat = rng.integers(0, len(CATEGORIES), 16384)
    t = np.zeros(16384, dtype=np.int64)
    n = int(src.size)
    sel = lambda name: np.nonzero(cat == CATEGORIES.index(name))[0]
    k = sel("negative")
    t[k] = -rng.integers(1, 1 << 31, k.size)
    t[sel("int32_min")] = -(1 << 31)
    t[sel("int32_max")] = (1 << 31) - 1
    k = sel("anywhere")
    t[k] = rng.integers(0, n, k.size) + 1
    k = sel("near_start")
    t[k] = rng.integers(start - 65540, start + 1, k.size) + 1
    k = sel("future")
    t[k] = rng.integers(start + length, start + length + 70000, k.size) + 1
    # a prewarm over src[start - 65536, start) filed under another hash: real positions inside
    # the window, in wrong buckets (what the reference's dictionary prewarm leaves)
    lo = max(0, start - 65536)
    if start - lo >= 4:
        pos = np.arange(lo, start - 3)
        fh = foreign_hash(vs[lo:start - 3])
        warm = np.zeros(16384, dtype=np.int64)
        warm[fh] = pos + 1                                  # the last position of a bucket wins
        k = sel("foreign_prewarm")
        t[k] = warm[k]
    # true stale: the slot of src[x, x + 4), x in the block, points at the nearest earlier equal
    # 4-gram within 65535
    order = np.lexsort((np.arange(vs.size), vs))
    prev = np.full(vs.size, -1, dtype=np.int64)
    same = vs[order][1:] == vs[order][:-1]
    prev[order[1:][same]] = order[:-1][same]
    xs = np.arange(start, start + length - 12)
    xs = xs[(prev[xs] >= 0) & (xs - prev[xs] <= 65535)]
    slots, first = np.unique(hs[xs], return_index=True)
    stale = np.zeros(16384, dtype=np.int64)
    stale[slots] = prev[xs[first]] + 1
    k = sel("true_stale")
    t[k] = stale[k]
    table = t.astype(np.int32)
    # self: p + 1 in the slot of a p the parse (with the table so far) probes
    (comp,), _ = oracle_run(Case("", src, start, length, None, table), None)
    for mpos, _, _, _ in matches_of(comp, start):
        s = int(hs[mpos])
        if cat[s] == CATEGORIES.index("self"):
            table[s] = mpos + 1
    return table, cat


def claim_F(case):
    """partial_table: the call changed some slots and left others. stale_hit: a match whose candidate
    is a true-stale entry of the initial table (the slot's first probe of the call finds it)."""
    ms, pr, tags = single_parse(case)
    t0, hs = case.table, META[case.name]["hs"]
    (_,), t1 = oracle_run(case, None)
    if 0 < int((t0 != t1).sum()) < 16384:
        tags.add("partial_table")
    seen, off_at = set(), {m[0]: m[2] for m in ms}
    for p, hit, e in pr:
        s = int(hs[p])
        if hit and s not in seen:
            off = off_at[p]
            if int(t0[s]) == p - off + 1 and META[case.name]["cat"][s] == CATEGORIES.index("true_stale"):
                tags.add("stale_hit")
        seen.add(s)
    return tags


EVERY_F = ("parse_ok", "partial_table", "stale_hit")


def family_F():
    src = np.concatenate([O.generate("text", 71, 50000), O.generate("copy", 72, 40000), O.generate("tiles216", 73, 50000)])
    hs, vs = all_h4(src)
    cases = []
    for start in STARTS:
        name = f"F_start{start}"
        length = min(F_LEN, src.size - start)

        def make(seed, start=start, length=length, name=name):
            rng = np.random.default_rng(seed)
            table, cat = caller_table(rng, src, start, length, hs, vs)
            META[name] = {"hs": hs, "cat": cat}
            return Case(name, src, start, length, None, table)

        cases.append(settle(make, claim_F, EVERY_F, 6000 + start, name))
    return Family("F", cases, claim_F, EVERY_F, ())


# ---------------------------------------------------------------------------- G: chain geometry
def claim_G(case):
    """boundary_in_run: a block boundary lies inside an equal-step run of the one-block parse;
    boundary_between_QP: one lies between Q and P of a C source; short_last_block: 1..13 bytes
    behind a full block."""
    m = META[case.name]
    ms, _, tags = single_parse(case)
    cuts = [case.start + k * case.block_size for k in range(1, -(-case.len // case.block_size))]
    for run in runs_of(ms):
        if len(run) >= 2 and any(run[0][0] < b < run[-1][0] + run[-1][1] for b in cuts):
            tags.add("boundary_in_run")
            break
    if "Q" in m and any(m["Q"] < b <= m["P"] for b in cuts):
        tags.add("boundary_between_QP")
    if case.len % case.block_size in range(1, 14) and case.len > case.block_size:
        tags.add("short_last_block")
    return tags


def family_G(A, B, C):
    sources = [("A64", next(c for c in A.cases if c.name == "A_S64")),
               ("B64", next(c for c in B.cases if c.name == "B_shared_S64")),
               ("C35", next(c for c in C.cases if c.name == "C_D65535_k3_r0")),
               ("C36", next(c for c in C.cases if c.name == "C_D65536_k3_r0"))]
    cases, some = [], []
    for tag, base in sources:
        for bs in CHAIN_BLOCKS:
            full = (base.len - 13) // bs
            k = min(full, 20) if bs < 1000 else min(full, 30) if bs == 1000 else full
            if k < 1:
                continue
            for r in range(1, 14):
                name = f"G_{tag}_b{bs}_r{r}"
                META[name] = dict(META[base.name])
                cases.append(Case(name, base.src, 0, k * bs + r, bs, None))
        some.append((f"G_{tag}_", "short_last_block"))
        some.append((f"G_{tag}_", "boundary_between_QP" if tag.startswith("C") else "boundary_in_run"))
    return Family("G", cases, claim_G, ("parse_ok",), tuple(some))


# --------------------------------------------------------------------------------- all of them
SIZES = {"A": 14, "B": 14, "C": 60, "D": 4, "E": 336, "F": 38, "G": 234}


@functools.lru_cache(maxsize=None)
def families():
    A = family_A()
    B = family_B()
    C = family_C()
    D = family_D()
    return {f.name: f for f in (A, B, C, D, family_E(A), family_F(), family_G(A, B, C))}


def all_cases(names="ABCDEFG"):
    return [c for n in names for c in families()[n].cases]


@functools.lru_cache(maxsize=None)
def expected(name):
    """The oracle's blocks and final table of a case (computed once, shared, never written to)."""
    case = next(c for c in all_cases() if c.name == name)
    blocks, table = oracle_run(case)
    for b in blocks:
        b.flags.writeable = False
    table.flags.writeable = False
    return blocks, table


def explain(case, block, got, want):
    """Names the first differing byte of a block and the sequence of the oracle's parse it lies in."""
    got, want = np.asarray(got, dtype=np.uint8), np.asarray(want, dtype=np.uint8)
    n = min(got.size, want.size)
    diff = np.nonzero(got[:n] != want[:n])[0]
    at = int(diff[0]) if diff.size else n
    bs = case.block_size or case.len
    pos, cp, where = case.start + block * bs, 0, "the end of the block"
    for k, (lp, ll, off, ml) in enumerate(parse(want)):
        nxt = lp + ll + (2 if off else 0) + (1 + (ml - 19) // 255 if off and ml >= 19 else 0)
        if at < nxt:
            where = (f"sequence {k} of the oracle's parse (compressed [{cp}, {nxt}): {ll} literals at source "
                     f"{pos}, match of {ml} at {pos + ll} with offset {off})")
            break
        cp, pos = nxt, pos + ll + ml
    return (f"{case.name} block {block}: {got.size} bytes, the oracle has {want.size}; first difference at "
            f"compressed byte {at} (got {int(got[at]) if at < got.size else None}, expected "
            f"{int(want[at]) if at < want.size else None}), in {where}")


def table_bytes(table):
    t = np.zeros(16384, dtype="<i4") if table is None else np.asarray(table, dtype="<i4")
    return t.view(np.uint8)


def digests(case, blocks, table):
    """What tests/golden/enc_shapes.json holds per case: XXH32 of the source and of the initial
    table, the blocks' lengths, the XXH32 over their XXH32s (little-endian u32s in order) and the
    XXH32 of the final table."""
    return ["%08x" % O.xxh32(case.src), "%08x" % O.xxh32(table_bytes(case.table)), [int(b.size) for b in blocks],
            "%08x" % O.digest_of_digests([O.xxh32(b) for b in blocks]), "%08x" % O.xxh32(table_bytes(table))]


def dump(directory):
    """The cases for tools/golden/gen_enc_shapes.mjs: cases.json and one file per distinct source
    and table (named by its XXH32)."""
    os.makedirs(directory, exist_ok=True)
    rows, written = [], set()

    def put(arr):
        name = "%08x_%d.bin" % (O.xxh32(arr), arr.size)
        if name not in written:
            arr.tofile(os.path.join(directory, name))
            written.add(name)
        return name

    for c in all_cases():
        rows.append({"name": c.name, "src": put(np.ascontiguousarray(c.src)), "start": c.start, "len": c.len,
                     "block_size": c.block_size, "table": None if c.table is None else put(table_bytes(c.table))})
    with open(os.path.join(directory, "cases.json"), "w") as f:
        json.dump(rows, f)
    return len(rows)

