#!/usr/bin/env python3
"""CPU model of what the decoder's 1 KiB chunks contain (csrc/lz4mi_decompress.hip), from the oracle's
generators and encoder only: per generator, the literal-run classes of a block, the whole-wave
iterations of a lane-serial literal loop (rows of 64 consecutive sequences of a chunk, two 16-byte
pieces per lane and iteration, the row's longest run sets the count) against the rows of the same
pieces dealt 64 to a row, and the cut sequences per block with and without deferring a last
sequence that would fit a window of its own to the next chunk.

  python tools/proto/literal_chunk_model.py [--size BYTES] [--seed N] [--gens a,b,...]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import oracle as O  # noqa: E402

CHUNK, LIM = 1024, 1024 + 64      # kChunk, kLim
FAST_REM = LIM + 300              # kFastRem: the fast next-token table is used farther than this from the end
LANE_BYTES = 256                  # longer runs were written by the whole wave


def parse(c):
    """-> [(token, literal length, match length or 0, next token, next token as the fast table sees it)]."""
    c = bytes(c)
    n, ip, out = len(c), 0, []
    while ip < n:
        tok = ip
        t = c[ip]
        ip += 1
        ll = t >> 4
        raw_ok = True
        if ll == 15:
            raw_ok = c[ip] != 255          # a literal length field of 2+ bytes stops the fast table's chain
            while True:
                b = c[ip]
                ip += 1
                ll += b
                if b != 255:
                    break
        ip += ll
        if ip >= n:
            out.append((tok, ll, 0, n, n if raw_ok else None))
            break
        ip += 2
        ml = t & 15
        raw = ip + (1 if ml == 15 else 0)
        if ml == 15:
            while True:
                b = c[ip]
                ip += 1
                ml += b
                if b != 255:
                    break
        out.append((tok, ll, ml + 4, ip, raw if raw_ok else None))
    return out


def chunks(seqs, size, defer):
    """The kernel's chunking -> ([sequence index ranges of the tables], cuts)."""
    tables, cuts, k, nseq = [], 0, 0, len(seqs)
    while k < nseq:
        ip = seqs[k][0]
        e = k
        while e < nseq and seqs[e][0] < ip + CHUNK:
            e += 1
        tok, ll, ml, nxt, raw = seqs[e - 1]
        fast = size - ip > FAST_REM
        cut = nxt - ip > LIM or (fast and raw is None)
        if cut and defer and fast and e - 1 > k and raw is not None and raw - tok <= LIM:
            tables.append((k, e - 1))           # the chunk ends at that token; the next one starts there
            k = e - 1
        elif cut:
            tables.append((k, e - 1))           # the last sequence is parsed from memory
            cuts += 1
            k = e
        else:
            tables.append((k, e))
            k = e
    return tables, cuts


def model(gen, seed, size):
    comp = O.compress_block_bytes(O.generate(gen, seed, size))
    seqs = parse(comp)
    runs = [s[1] for s in seqs if s[1]]
    cls = (("1-15", 1, 15), ("16-%d" % LANE_BYTES, 16, LANE_BYTES), ("> %d" % LANE_BYTES, LANE_BYTES + 1, 1 << 30))
    print(f"{gen}: seed {seed}, {size} -> {len(comp)} bytes, {len(seqs)} sequences, {len(runs)} with literals "
          f"({sum(runs)} literal bytes, {100.0 * sum(runs) / len(comp):.0f} % of the compressed stream)")
    for name, lo, hi in cls:
        r = sorted(x for x in runs if lo <= x <= hi)
        med = f", median {r[len(r) // 2]}, p90 {r[len(r) * 9 // 10]}" if r else ""
        print(f"  literal runs of {name} B: {len(r)} holding {sum(r)} bytes{med}")
    sizes = sorted(s[3] - s[0] for s in seqs)
    print(f"  sequences of 4 bytes: {100.0 * sum(1 for x in sizes if x == 4) / len(sizes):.0f} %")
    for defer in (False, True):
        tables, cuts = chunks(seqs, len(comp), defer)
        iters = pieces = rows = 0
        for a, b in tables:
            total = 0
            for r0 in range(a, b, 64):
                np_ = [(s[1] + 15) >> 4 for s in seqs[r0:min(r0 + 64, b)] if 16 <= s[1] <= LANE_BYTES]
                iters += (max(np_) + 1) // 2 if np_ else 0
                total += sum(np_)
            pieces += total
            rows += (total + 63) // 64
        n = len(tables)
        print(f"  {'deferred' if defer else 'as parsed'}: {n} chunks, {cuts} cuts; per chunk {iters / n:.1f} lane-serial "
              f"iterations for {pieces / n:.1f} pieces = {rows / n:.2f} dealt rows")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=4 << 20)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--gens", default="tiles216,text,copy,runs,random")
    args = ap.parse_args()
    for gen in args.gens.split(","):
        model(gen, args.seed, args.size)


if __name__ == "__main__":
    main()
