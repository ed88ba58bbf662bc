#!/usr/bin/env python3
"""Decode times of the tree's library against another build of it (--base OTHER.so), shape by
shape in one process, the two builds alternating rep by rep on the same device buffers: whole
batches of 4 MiB blocks per generator (microbench.make_raw: the device generators, bench.py's mix
and mixc, the oracle's text / copy / runs) and small batches (--small-gens, --counts: the
small-batch path). Per shape: min / median / max of each build and `slower`, whether the tree's
median exceeds the base's by more than the base's own max - min.

  python tools/ab_shapes.py --base old/liblz4mi.so --gens random,repetitive,mix,mixc,text,copy
"""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "divortio-lz4_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
BLOCK = 4 << 20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--base", required=True, help="the other build of liblz4mi.so")
    ap.add_argument("--gens", default="random,repetitive,mix,mixc,text,copy")
    ap.add_argument("--blocks", type=int, default=4096)
    ap.add_argument("--small-gens", default="tiles216,text")
    ap.add_argument("--counts", default="1,64")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--js-exact", action="store_true")
    args = ap.parse_args()
    import torch
    import lz4mi
    from microbench import make_raw
    lz4mi.init(0)
    base = ctypes.CDLL(os.path.abspath(args.base))
    base.lz4mi_decompress_blocks.restype = ctypes.c_int32
    base.lz4mi_decompress_blocks.argtypes = lz4mi.lib().lz4mi_decompress_blocks.argtypes
    base.lz4mi_init.restype = ctypes.c_int32
    assert base.lz4mi_init(0) == 0
    libs = (("base", base), ("tree", lz4mi.lib()))
    s = torch.cuda.Stream()
    torch.cuda.set_stream(s)
    sp = s.cuda_stream
    flags = 1 | (8 if args.js_exact else 0)
    res = {}

    def shape(gen, n, counts):
        raw = make_raw(torch, lz4mi, gen, n, sp)
        slot = (lz4mi.compress_bound(BLOCK) + 255) & ~255
        comp = torch.zeros(n * slot, dtype=torch.uint8, device="cuda")
        roff = torch.arange(n, dtype=torch.int64, device="cuda") * BLOCK
        rlen = torch.full((n,), BLOCK, dtype=torch.int32, device="cuda")
        coff = torch.arange(n, dtype=torch.int64, device="cuda") * slot
        clen = torch.zeros(n, dtype=torch.int32, device="cuda")
        lz4mi.compress_blocks_dev(raw.data_ptr(), roff.data_ptr(), rlen.data_ptr(), comp.data_ptr(), coff.data_ptr(),
                                  clen.data_ptr(), n, sp)
        dec = torch.empty(n * BLOCK, dtype=torch.uint8, device="cuda")
        dlen = torch.zeros(n, dtype=torch.int32, device="cuda")
        st = torch.zeros(n, dtype=torch.int32, device="cuda")
        for b in counts:
            times, ok = {"base": [], "tree": []}, {}
            for name, L in libs:                       # warm-up and the bytes
                dec.zero_()
                assert L.lz4mi_decompress_blocks(comp.data_ptr(), coff.data_ptr(), clen.data_ptr(), dec.data_ptr(),
                                                 roff.data_ptr(), rlen.data_ptr(), None, 0, dlen.data_ptr(),
                                                 st.data_ptr(), b, flags, sp) == 0
                torch.cuda.synchronize()
                ok[name] = bool(torch.equal(dec[:b * BLOCK], raw[:b * BLOCK])) and bool((st[:b] == 0).all())
            for _ in range(args.reps):
                for name, L in libs:
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(s)
                    assert L.lz4mi_decompress_blocks(comp.data_ptr(), coff.data_ptr(), clen.data_ptr(), dec.data_ptr(),
                                                     roff.data_ptr(), rlen.data_ptr(), None, 0, dlen.data_ptr(),
                                                     st.data_ptr(), b, flags, sp) == 0
                    e1.record(s)
                    torch.cuda.synchronize()
                    times[name].append(e0.elapsed_time(e1))
            row = {}
            for name in times:
                t = sorted(times[name])
                row[name] = {"min": round(t[0], 4), "median": round(t[len(t) // 2], 4), "max": round(t[-1], 4), "ok": ok[name]}
            row["slower"] = row["tree"]["median"] - row["base"]["median"] > row["base"]["max"] - row["base"]["min"]
            res[f"{gen}/{b}"] = row
            print(f"{gen}/{b}", json.dumps(row), flush=True)
        del raw, comp, dec
        torch.cuda.empty_cache()

    for gen in [g for g in args.gens.split(",") if g]:
        shape(gen, args.blocks, [args.blocks])
    counts = [int(x) for x in args.counts.split(",")]
    for gen in [g for g in args.small_gens.split(",") if g]:
        shape(gen, max(counts), counts)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
