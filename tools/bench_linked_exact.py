#!/usr/bin/env python3
"""Dependent-block frames (content size present) decoded in the reference decoder's bytes, four legs
per shape -- the frames and the method of tools/bench_linked.py:

  (a) lz4mi_frame_decompress with LZ4MI_LINKED_EXACT: the compressed blocks in one linked call;
  (b) the same call with LZ4MI_JS_EXACT and no linked flag: the batch reports LZ4MI_ERR_CROSS_BLOCK
      for the dependent blocks, which are then decoded one per launch in order;
  (c) lz4mi_host_decompress_block with LZ4MI_JS_EXACT in block order on one core, host memory;
  (d) lz4mi_frame_decompress with LZ4MI_LINKED (spec mode) on the same frame in the same process:
      (a) / (d) is what reference mode costs.

Shapes: tiles216 256 x 4 MiB, tiles216 1 GiB in 64 KiB blocks, text 64 x 4 MiB; the frames are
written by the oracle's encoder. Before timing, (a), (b) and (c) are compared with the oracle's
reference-mode frame decode (js_compat) and (d) with the input. (a), (b), (d): device-resident, HIP
events on the launch stream around the call (it synchronises inside), warm-up, median of --reps;
(c): wall clock, median of --reps. For (a) the windows, the scratch held and the resumes behind
refused blocks are recorded.

--legs b --lib OTHER/liblz4mi.so runs leg (b) on another build of the library (the parent commit's);
--parent-json FILE embeds such a run's result.

Writes one JSON document (--out, default profiles/linked_exact/bench.json) and prints it.

  python tools/bench_linked_exact.py [--shapes tiles216_4m,tiles216_64k,text_4m] [--legs abcd] [--reps 5]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "divortio-lz4_amd"), os.path.join(ROOT, "oracle"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

SHAPES = {"tiles216_4m": ("tiles216", 256 * (4 << 20), 4 << 20),
          "tiles216_64k": ("tiles216", 1 << 30, 65536),
          "text_4m": ("text", 64 * (4 << 20), 4 << 20)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="tiles216_4m,tiles216_64k,text_4m")
    ap.add_argument("--legs", default="abcd")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--scale", type=int, default=1, help="divide every shape's size by this (quick runs)")
    ap.add_argument("--lib", default=None, help="another build of liblz4mi.so (leg b on the parent commit)")
    ap.add_argument("--parent-json", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "linked_exact", "bench.json"))
    args = ap.parse_args()

    import numpy as np
    import torch
    import lz4mi
    import oracle as O
    from lz4mi import shard

    if args.lib:
        lz4mi.LIB_PATH = os.path.abspath(args.lib)
    lz4mi.init(0)
    stream_obj = torch.cuda.current_stream()
    stream = stream_obj.cuda_stream

    def frame_call(dev, out, size, flags):
        info = np.zeros(8, dtype=np.int64)
        st = lz4mi.lib().lz4mi_frame_decompress(dev.data_ptr(), dev.numel(), out.data_ptr(), size, info.ctypes.data,
                                                lz4mi.DEVICE_PTRS | flags, stream)
        assert st == 0 and info[0] == 0 and info[3] == size, (st, info.tolist())

    def med(ts):
        return {"median_ms": round(statistics.median(ts), 3), "min_ms": round(min(ts), 3), "max_ms": round(max(ts), 3)}

    def gpu_leg(dev, out, want_dev, size, flags):
        out.zero_()
        frame_call(dev, out, size, flags)
        torch.cuda.synchronize()
        assert torch.equal(out, want_dev), "decoded frame differs from the expected bytes"
        for _ in range(args.warmup):
            frame_call(dev, out, size, flags)
        ev, wall = [], []
        for _ in range(args.reps):
            e0 = torch.cuda.Event(enable_timing=True)
            e1 = torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            e0.record(stream_obj)
            frame_call(dev, out, size, flags)
            e1.record(stream_obj)
            torch.cuda.synchronize()
            wall.append((time.perf_counter() - t0) * 1e3)
            ev.append(e0.elapsed_time(e1))
        r = med(ev)
        r["wall_median_ms"] = round(statistics.median(wall), 3)
        r["GBps"] = round(size / r["median_ms"] / 1e6, 2)
        return r

    res = {"device": torch.cuda.get_device_name(0), "build_id": lz4mi.build_id(), "library": args.lib or "this tree",
           "timing": f"(a), (b), (d): HIP events around lz4mi_frame_decompress, {args.warmup} warm-up, median of "
                     f"{args.reps}; (c): wall clock, median of {args.reps}", "shapes": {}}
    for name in args.shapes.split(","):
        kind, total, bs = SHAPES[name]
        total //= args.scale
        data = O.generate(kind, 1, total)   # (one generator run: the blocks do reference their predecessors)
        frame = O.compress_frame(data, None, bs, False, False, True)
        est, want = O.decompress_frame(frame, verify_checksum=False, js_compat=True, out_cap=total + 64)
        assert est == 0 and want.size == total
        info, blocks = shard.frame_blocks(frame)
        r = {"kind": kind, "raw_bytes": int(data.size), "block_bytes": bs, "blocks": len(blocks),
             "stored_blocks": sum(1 for b in blocks if b[2]), "frame_bytes": int(frame.size),
             "bytes_differing_from_input": int((want != data).sum())}
        dev = torch.from_numpy(frame).cuda()
        want_dev = torch.from_numpy(want).cuda()
        out = torch.empty(data.size, dtype=torch.uint8, device="cuda")
        if "a" in args.legs:
            r["a_linked_exact"] = gpu_leg(dev, out, want_dev, data.size, lz4mi.LINKED_EXACT)
            stats = (ctypes.c_ulonglong * 4)()
            L = lz4mi.lib()
            L.lz4mi_debug_linked_stats(stats)
            L.lz4mi_debug_linked_resumes.restype = ctypes.c_ulonglong
            r["a_linked_exact"].update({"windows_last_call": int(stats[0]), "scratch_bytes": int(stats[1]),
                                        "x_in_max": int(stats[2]), "x_out_max": int(stats[3]),
                                        "resumes": int(L.lz4mi_debug_linked_resumes())})
        if "b" in args.legs:
            r["b_js_exact_unflagged"] = gpu_leg(dev, out, want_dev, data.size, lz4mi.JS_EXACT)
        if "d" in args.legs:
            data_dev = torch.from_numpy(data).cuda()
            r["d_linked_spec"] = gpu_leg(dev, out, data_dev, data.size, lz4mi.LINKED)
            del data_dev
            if "a" in args.legs:
                r["a_over_d"] = round(r["a_linked_exact"]["median_ms"] / r["d_linked_spec"]["median_ms"], 3)
        del dev, want_dev, out
        torch.cuda.empty_cache()
        if "c" in args.legs:
            host = np.zeros(data.size, dtype=np.uint8)
            ts = []
            for rep in range(args.reps + 1):
                t0 = time.perf_counter()
                pos = 0
                for p, n, stored in blocks:
                    if stored:
                        host[pos:pos + n] = frame[p:p + n]
                        pos += n
                    else:
                        pos += lz4mi.host_decompress_raw(frame, p, n, host, pos)
                ts.append((time.perf_counter() - t0) * 1e3)
                if rep == 0:
                    assert pos == data.size and np.array_equal(host, want), "host decode differs from the oracle's"
            r["c_host_one_core"] = med(ts[1:])
            r["c_host_one_core"]["GBps"] = round(data.size / r["c_host_one_core"]["median_ms"] / 1e6, 2)
            del host
        res["shapes"][name] = r
        del data, frame, want
    if args.parent_json:
        with open(args.parent_json) as f:
            pj = json.load(f)
        res["parent_commit"] = {"build_id": pj["build_id"],
                                "b_js_exact_unflagged": {k: v.get("b_js_exact_unflagged") for k, v in pj["shapes"].items()}}

    text = json.dumps(res, indent=1)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
