#!/usr/bin/env python3
"""A batch of device-resident buffers compressed into one frame each by one lz4mi_frames_plan +
lz4mi_frames_compress pair against the only way there was before: a loop of DeviceCodec.records + header, one
frame per iteration with its synchronisations. In one process, on device-resident buffers, per shape (frames x
bytes per frame, one block each, tiles216), with and without the content checksum:

  - batch:   both calls (packed), HIP events on the launch stream (device time, nothing read back);
  - loop:    DeviceCodec.records + frame.header per frame (with the content checksum: the source copied to the
             host and hashed there, as the per-frame path does), wall clock -- it synchronises itself; measured
             over the first --loop-frames frames and scaled to the shape's frame count (every frame costs the same);
  - floor:   compress_blocks_dev of the same blocks with precomputed lists, HIP events;
  - wrapper: frame.compress_frames_device end to end, wall clock, allocations and both read-backs included.

Writes one JSON document (--out, default profiles/frames_compress/bench.json) and prints it.

  python tools/bench_frames_compress.py [--reps 5] [--warmup 2] [--small] [--shapes 16384x4K,...]

--batch-only times the batch alone and writes nothing: the run to put under `rocprofv3 --kernel-trace --stats`,
whose per-kernel averages then belong to the batch's passes.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "divortio-lz4_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

# name, frames, bytes per frame (= the block size)
SHAPES = [("16384x4K", 16384, 4096), ("4096x64K", 4096, 65536), ("256x4M", 256, 4 << 20)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--loop-frames", type=int, default=1024)
    ap.add_argument("--shapes", default="", help="comma-separated shape names (default: all)")
    ap.add_argument("--batch-only", action="store_true", help="only the batch legs, no JSON file (for a profiler run)")
    ap.add_argument("--small", action="store_true", help="a sixteenth of the frames of every shape (a quick look)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "frames_compress", "bench.json"))
    args = ap.parse_args()

    import torch
    import lz4mi
    from lz4mi import frame as F

    lz4mi.init(0)
    stream_obj = torch.cuda.current_stream()
    stream = stream_obj.cuda_stream

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

    res = {"device": torch.cuda.get_device_name(0), "build_id": lz4mi.build_id(), "content": "tiles216",
           "timing": f"batch and floor: HIP events on the launch stream, {args.warmup} warm-ups, median of {args.reps}; "
                     f"loop: wall clock around calls that synchronise, 1 warm-up, median of 3, over the first "
                     f"--loop-frames frames, scaled to the frame count; wrapper: wall clock, 1 warm-up, median of 3",
           "shapes": {}}
    for name, nf, n in SHAPES:
        if args.shapes and name not in args.shapes.split(","):
            continue
        if args.small:
            nf = max(4, nf // 16)
        bs = {4: 65536, 5: 262144, 6: 1048576, 7: 4194304}[F.block_id(n)]
        raw = torch.empty(nf * n, dtype=torch.uint8, device="cuda")
        lz4mi.generate_blocks_dev(raw.data_ptr(), "tiles216", 1, n, nf, stream)
        src_off = torch.arange(nf, dtype=torch.int64, device="cuda") * n
        src_len = torch.full((nf,), n, dtype=torch.int64, device="cuda")
        blk64 = torch.zeros((2, nf), dtype=torch.int64, device="cuda")
        blk32 = torch.zeros((2, nf), dtype=torch.int32, device="cuda")
        fin = torch.zeros(8 * nf + 4, dtype=torch.int64, device="cuda")

        def plan(flags):
            lz4mi.frames_plan_dev(src_off.data_ptr(), src_len.data_ptr(), nf, n, blk64[0].data_ptr(), blk32[0].data_ptr(),
                                  blk32[1].data_ptr(), blk64[1].data_ptr(), nf, fin.data_ptr(), fin.data_ptr() + 64 * nf,
                                  stream, flags=flags)

        plan(lz4mi.frames_enc_flags(content_checksum=True, packed=True))
        totals = fin[8 * nf:].cpu().tolist()
        work = torch.empty(int(totals[3]), dtype=torch.uint8, device="cuda")
        out = torch.empty(int(totals[2]), dtype=torch.uint8, device="cuda")

        # the floor: the same blocks through the plain batch encoder
        comp_len = torch.zeros(nf, dtype=torch.int32, device="cuda")
        def plain():
            lz4mi.compress_blocks_dev(raw.data_ptr(), blk64[0].data_ptr(), blk32[0].data_ptr(), work.data_ptr(),
                                      blk64[1].data_ptr(), comp_len.data_ptr(), nf, stream)

        floor = None if args.batch_only else event_ms(plain)
        codec = F.DeviceCodec()
        nloop = min(nf, args.loop_frames)
        for csum in (False, True):
            flags = lz4mi.frames_enc_flags(content_checksum=csum, packed=True)

            def batch():
                plan(flags)
                lz4mi.frames_compress_dev(raw.data_ptr(), blk64[0].data_ptr(), blk32[0].data_ptr(), blk32[1].data_ptr(),
                                          blk64[1].data_ptr(), nf, fin.data_ptr(), nf, work.data_ptr(), work.numel(),
                                          out.data_ptr(), out.numel(), None, None, stream, flags=flags)

            def one(f):
                src = raw[f * n:(f + 1) * n]
                rec = codec.records(src, bs, False)
                head = F.header(bs, True, csum, n)
                tail = b"\0\0\0\0" + (int(lz4mi.XXHash32(0, len64=True).update(src.cpu().numpy()).digest())
                                      .to_bytes(4, "little") if csum else b"")
                return head, rec, tail

            def loop():
                for f in range(nloop):
                    one(f)

            r = {"frames": nf, "frame_source_bytes": n, "block_bytes": bs, "content_checksum": csum, "raw_bytes": nf * n}
            r["batch"] = event_ms(batch)
            if args.batch_only:
                print(name, csum, json.dumps(r), flush=True)
                continue
            info = fin[:8 * nf].cpu().numpy().reshape(nf, 8)
            r["frame_bytes"] = int(info[:, 3].sum())
            ok = bool((info[:, 7] == 0).all())
            for f in (0, nloop - 1):        # the batch's frames are the loop's
                head, rec, tail = one(f)
                got = out[int(info[f, 5]):int(info[f, 5] + info[f, 3])].cpu().numpy().tobytes()
                ok = ok and got == head + rec.cpu().numpy().tobytes() + tail
            r["batch_verified"] = ok
            r["plan_only"] = event_ms(lambda: plan(flags))
            r["floor_compress_blocks"] = floor
            lp = wall_ms(loop, 3, 1)
            r["loop_frames_measured"] = nloop
            r["loop"] = {k: round(v * nf / nloop, 3) for k, v in lp.items()}
            r["loop_per_frame_ms"] = round(lp["median_ms"] / nloop, 4)
            rep = {}
            r["wrapper"] = wall_ms(lambda: F.compress_frames_device(raw, block_size=n, content_checksum=csum, report=rep,
                                                                    offsets=range(0, nf * n, n), lengths=[n] * nf), 3, 1)
            r["wrapper_routes_batch"] = rep["routes"].count("batch")
            r["loop_over_batch"] = round(r["loop"]["median_ms"] / r["batch"]["median_ms"], 2)
            r["loop_over_wrapper"] = round(r["loop"]["median_ms"] / r["wrapper"]["median_ms"], 2)
            r["batch_over_floor"] = round(r["batch"]["median_ms"] / floor["median_ms"], 3)
            r["batch_GBps_raw"] = round(r["raw_bytes"] / r["batch"]["median_ms"] / 1e6, 2)
            key = name + ("_checksum" if csum else "")
            res["shapes"][key] = r
            print(key, json.dumps(r), flush=True)
        del raw, work, out, codec
        torch.cuda.empty_cache()

    if args.batch_only:
        return
    text = json.dumps(res, indent=1)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
