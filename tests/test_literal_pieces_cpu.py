"""CPU: the hand-assembled blocks of literal_pieces_common are what they claim -- each decodes on
the oracle to the intended bytes and status, and the tokens lie where the case names say."""
import numpy as np

import literal_pieces_common as C
from footprint_common import reads_below


def test_valid_blocks_decode_to_the_intended_bytes():
    raw, cs = C.raw_cases(), C.all_cases()
    for name, (comp, cap, opts, ref) in cs.items():
        if "want" in opts:
            continue
        seqs, fin = raw[name][0], raw[name][1]
        want = C.expected_bytes(seqs, fin)
        assert cap == want.size, name
        for js in (False, True):
            st, n, out = ref[js]
            assert st == C.OK and n == want.size, (name, js, st)
        assert np.array_equal(ref[False][2][:want.size], want), name
        # no tail rewrite of the reference reads below the block: in a batch of independent blocks
        # the reference modes decode it too, so js_exact is compared byte for byte everywhere
        assert not reads_below(comp), name


def test_failing_blocks_fail_as_intended():
    cs = C.all_cases()
    seen = set()
    for name, (comp, cap, opts, ref) in cs.items():
        if "want" in opts:
            assert ref[False][0] == opts["want"] and ref[True][0] == opts["want"], (name, ref[False][0])
            seen.add(opts["want"])
    assert seen == {C.TOO_SMALL, C.MALFORMED, C.OFFSET0}
    # the failing sequence is the 100-byte run behind 20 valid four-byte sequences
    comp = cs["run_overruns_input"][0]
    assert comp.size == 80 + 2 + 50 and comp[80] >> 4 == 15 and comp[81] == 100 - 15
    comp = cs["offset0_after_run"][0]
    assert comp[80] >> 4 == 15 and comp[81] == 85 and comp[182] == 0 and comp[183] == 0


def test_ladder_and_list_limits():
    raw, cs = C.raw_cases(), C.all_cases()
    assert [len(s[0]) for s in raw["ladder_all"][0][:len(C.LADDER)]] == list(C.LADDER)
    for n in C.LADDER:
        assert len(raw[f"ladder_{n}"][0][3][0]) == n
    toks = C.tokens_of(cs["max_runs"][0])
    assert sum(1 for t in toks if t < C.CHUNK) == 52 and all(len(s[0]) == 16 for s in raw["max_runs"][0])
    seqs = raw["late_runs"][0]
    assert all(len(s[0]) < 16 for s in seqs[:257]) and all(len(s[0]) == 17 for s in seqs[257:])
    toks = C.tokens_of(cs["late_runs"][0])
    assert len(seqs) == 267 and toks[266] < C.CHUNK
    for n in C.FINALS:
        comp, cap, _, ref = cs[f"final_{n}"]
        assert len(raw[f"final_{n}"][1]) == n and ref[False][1] == cap


def test_remap_sources_lie_where_intended():
    raw = C.raw_cases()
    for name, (seqs, fin, _, _) in raw.items():
        if not name.startswith("remap_"):
            continue
        k = 256 if name.endswith("_c1") else 3
        a = sum(len(s[0]) + s[2] for s in seqs[:k])             # output start of the run
        run, own = len(seqs[k][0]), seqs[k][2]
        ms = a + run + own + 1
        src, ml = ms - seqs[k + 1][1], seqs[k + 1][2]
        assert run >= 16 and ml >= 16
        if "inside" in name:
            assert a <= src and src + ml <= a + run, name
        else:
            assert a <= src < a + run < src + ml <= a + run + own, name
        if k == 256:
            assert C.size_of(seqs[:k]) == C.CHUNK
            assert a + run - seqs[k][1] + own <= a, name          # the run's own match reads the chunk before


def test_window_edge_tokens():
    cs = C.all_cases()
    for name, (comp, cap, opts, ref) in cs.items():
        if "token" not in opts:
            continue
        toks = C.tokens_of(comp)
        assert opts["token"] in toks, name
        k = toks.index(opts["token"])
        assert comp[toks[k]] >> 4 == 15, name                       # a literal run of >= 15 bytes
        if name.endswith("_last"):
            assert toks[k + 1] == opts["land"] and k + 2 == len(toks), name
        elif name.endswith("_ends"):
            assert k + 1 == len(toks) and comp.size == opts["land"], name
        else:
            assert toks[k + 1] == opts["land"], name
        if name.endswith("_ml2"):
            assert list(comp[opts["land"] - 2:opts["land"]]) == [255, 40], name
            assert comp.size - opts["token"] > C.LIM + 300, name    # the fast next-token table is in use
    for tok in (1000, 828):
        toks = C.tokens_of(cs[f"twice_{tok}"][0])
        assert tok in toks and C.LIM + 40 in toks and C.LIM + 40 + tok in toks
        assert toks[toks.index(C.LIM + 40 + tok) + 1] == C.LIM + 40 + C.LIM + 1
    assert cs["first_too_long"][0].size > 1100
