#!/usr/bin/env python3
"""Dependent frames of more than one block in the frame batch (LZ4MI_FRAMES_CHAINS: one chain per frame, one
workgroup each, all in one launch) against what there was before, the per-frame chain, and against the
independent batch of the same buffers. In one process, on device-resident buffers, per shape (frames x bytes per
frame @ block size) and content (tiles216, text), no content checksum:

  - a, chains:       lz4mi_frames_plan + lz4mi_frames_compress with DEPENDENT | CHAINS (packed), HIP events on the
                     launch stream (device time, nothing read back);
  - b, loop:         frame.compress_frames_device(independent=False, chains=False): the batch declines every frame and
                     completes each alone through lz4mi.compress_chain (a host-pointer call: the source staged to
                     the device, one workgroup, two synchronisations per frame). Wall clock -- it synchronises
                     itself --, over the first --loop-frames frames (fewer for long frames: --loop-bytes) and scaled
                     to the shape's frame count (every frame costs the same);
  - c, independent:  the same two calls without DEPENDENT (every block through the batch encoder), HIP events.

The text is this tool's own (a seeded word sampler: the GPU machine needs nothing but liblz4mi); frame f is a
window of one 32 MiB text at its own start. Writes one JSON document (--out, default
profiles/frames_chains/bench.json) and prints it.

  python tools/bench_frames_chains.py [--reps 5] [--warmup 2] [--small] [--shapes 256x1M@64K,...]

--chains-only times leg a alone and writes nothing: the run to put under a profiler.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "divortio-lz4_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

# name, frames, bytes per frame, block size
SHAPES = [("256x1M@64K", 256, 1 << 20, 65536), ("1024x256K@64K", 1024, 256 << 10, 65536),
          ("64x16M@4M", 64, 16 << 20, 4 << 20)]
TEXT_BYTES = 32 << 20


def make_text(n, seed=1):
    """n bytes of words drawn from a 4096-word vocabulary with a Zipf-like law, separated by spaces."""
    rng = np.random.default_rng(seed)
    nv = 4096
    wlen = rng.integers(2, 11, nv)
    letters = rng.integers(97, 123, (nv, 10)).astype(np.uint8)
    p = 1.0 / np.arange(1, nv + 1)
    idx = rng.choice(nv, size=n // 4 + 16, p=p / p.sum())
    step = wlen[idx] + 1
    offs = np.cumsum(step) - step
    out = np.full(int(offs[-1] + step[-1]), 32, dtype=np.uint8)
    for j in range(10):
        m = wlen[idx] > j
        out[offs[m] + j] = letters[idx[m], j]
    assert out.size >= n
    return out[:n]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--loop-frames", type=int, default=32)
    ap.add_argument("--loop-bytes", type=int, default=64 << 20, help="at most this many source bytes in leg b")
    ap.add_argument("--shapes", default="", help="comma-separated shape names (default: all)")
    ap.add_argument("--contents", default="tiles216,text", help="comma-separated contents")
    ap.add_argument("--chains-only", action="store_true", help="only leg a, no JSON file (for a profiler run)")
    ap.add_argument("--small", action="store_true", help="an eighth of the frames of every shape (a quick look)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "frames_chains", "bench.json"))
    args = ap.parse_args()
    assert args.reps >= 5 or args.chains_only or args.small, "the committed numbers are medians of at least 5 runs"

    import torch
    import lz4mi
    from lz4mi import frame as F

    lz4mi.init(0)
    stream_obj = torch.cuda.current_stream()
    stream = stream_obj.cuda_stream
    cus = torch.cuda.get_device_properties(0).multi_processor_count

    def stats(ts):
        return {"median_ms": round(statistics.median(ts), 4), "min_ms": round(min(ts), 4), "max_ms": round(max(ts), 4)}

    def event_ms(fn):
        for _ in range(args.warmup):
            fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(args.reps):
            e0 = torch.cuda.Event(enable_timing=True)
            e1 = torch.cuda.Event(enable_timing=True)
            e0.record(stream_obj)
            fn()
            e1.record(stream_obj)
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1))
        return stats(ts)

    def wall_ms(fn, reps, warmup):
        for _ in range(warmup):
            fn()
        ts = []
        for _ in range(reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        return stats(ts)

    text = torch.from_numpy(make_text(TEXT_BYTES)).cuda()
    res = {"device": torch.cuda.get_device_name(0), "compute_units": cus, "build_id": lz4mi.build_id(),
           "timing": f"chains and independent: HIP events on the launch stream, {args.warmup} warm-ups, median of "
                     f"{args.reps}; loop: wall clock around calls that synchronise, 1 warm-up, median of 5, over the "
                     f"first frames (loop_frames_measured), scaled to the frame count",
           "shapes": {}}
    for name, nf, n, bs in SHAPES:
        if args.shapes and name not in args.shapes.split(","):
            continue
        if args.small:
            nf = max(4, nf // 8)
        nb = nf * (n // bs)
        for content in args.contents.split(","):
            raw = torch.empty(nf * n, dtype=torch.uint8, device="cuda")
            if content == "tiles216":
                lz4mi.generate_blocks_dev(raw.data_ptr(), "tiles216", 1, n, nf, stream)
            else:
                for f in range(nf):
                    o = (f * 1048583) % (TEXT_BYTES - n)
                    raw[f * n:(f + 1) * n] = text[o:o + n]
            src_off = torch.arange(nf, dtype=torch.int64, device="cuda") * n
            src_len = torch.full((nf,), n, dtype=torch.int64, device="cuda")
            blk64 = torch.zeros((2, nb), dtype=torch.int64, device="cuda")
            blk32 = torch.zeros((2, nb), dtype=torch.int32, device="cuda")
            fin = torch.zeros(8 * nf + 4, dtype=torch.int64, device="cuda")
            work = torch.empty(16 + nb * (bs + bs // 255 + 32), dtype=torch.uint8, device="cuda")
            out = torch.empty(nf * lz4mi.frame_bound(n, bs), dtype=torch.uint8, device="cuda")

            def batch(flags):
                lz4mi.frames_plan_dev(src_off.data_ptr(), src_len.data_ptr(), nf, bs, blk64[0].data_ptr(),
                                      blk32[0].data_ptr(), blk32[1].data_ptr(), blk64[1].data_ptr(), nb, fin.data_ptr(),
                                      fin.data_ptr() + 64 * nf, stream, flags=flags)
                lz4mi.frames_compress_dev(raw.data_ptr(), blk64[0].data_ptr(), blk32[0].data_ptr(), blk32[1].data_ptr(),
                                          blk64[1].data_ptr(), nb, fin.data_ptr(), nf, work.data_ptr(), work.numel(),
                                          out.data_ptr(), out.numel(), None, None, stream, flags=flags)

            def info():
                return fin[:8 * nf].cpu().numpy().reshape(nf, 8).copy()

            fa = lz4mi.frames_enc_flags(independent=False, packed=True, chains=True)
            fc = lz4mi.frames_enc_flags(independent=True, packed=True)
            r = {"frames": nf, "frame_source_bytes": n, "block_bytes": bs, "content": content, "raw_bytes": nf * n}
            r["chains"] = event_ms(lambda: batch(fa))
            r["chains_GBps_raw"] = round(r["raw_bytes"] / r["chains"]["median_ms"] / 1e6, 2)
            key = f"{name}_{content}"
            if args.chains_only:
                print(key, json.dumps(r), flush=True)
                continue
            ia = info()
            r["frame_bytes_dependent"] = int(ia[:, 3].sum())
            nloop = max(1, min(nf, args.loop_frames, args.loop_bytes // n))
            offs, lens = list(range(0, nloop * n, n)), [n] * nloop
            rep, kept = {}, []

            def loop():
                kept[:] = F.compress_frames_device(raw, block_size=bs, independent=False, chains=False, report=rep,
                                                   offsets=offs, lengths=lens)

            lp = wall_ms(loop, 5, 1)
            ok = bool((ia[:, 7] == 0).all()) and rep["routes"] == ["chain"] * nloop
            for f in range(nloop):        # the batch's frames are the loop's
                ok = ok and torch.equal(out[int(ia[f, 5]):int(ia[f, 5] + ia[f, 3])], kept[f])
            r["chains_verified"] = ok
            r["loop_frames_measured"] = nloop
            r["loop"] = {k: round(v * nf / nloop, 3) for k, v in lp.items()}
            r["loop_per_frame_ms"] = round(lp["median_ms"] / nloop, 4)
            r["loop_GBps_raw"] = round(r["raw_bytes"] / r["loop"]["median_ms"] / 1e6, 3)
            r["independent"] = event_ms(lambda: batch(fc))
            ic = info()
            r["independent_verified"] = bool((ic[:, 7] == 0).all())
            r["frame_bytes_independent"] = int(ic[:, 3].sum())
            r["independent_GBps_raw"] = round(r["raw_bytes"] / r["independent"]["median_ms"] / 1e6, 2)
            r["a_over_b"] = round(r["loop"]["median_ms"] / r["chains"]["median_ms"], 2)
            r["a_over_c"] = round(r["independent"]["median_ms"] / r["chains"]["median_ms"], 3)
            r["chains_per_cu"] = round(nf / cus, 2)   # one workgroup per CU at a time: the rounds of the launch
            res["shapes"][key] = r
            print(key, json.dumps(r), flush=True)
            del raw, work, out, kept
            torch.cuda.empty_cache()

    if args.chains_only:
        return
    text_json = json.dumps(res, indent=1)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text_json + "\n")
    print(text_json)


if __name__ == "__main__":
    main()
