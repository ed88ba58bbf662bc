#!/usr/bin/env python3
"""The size pass (lz4mi_decoded_sizes) against the only other way to learn decoded sizes, the
batch decode into block_max slots, in one process on device-resident buffers:

  - 4096 x 4 MiB tiles216, random, repetitive and the 50/50 random/tiles216 mix: size pass and
    batch decode (HIP events on the launch stream, warm-up, median of --reps);
  - 256 x 4 MiB text (generated on the host by the oracle, compressed on the GPU): the same;
  - a lone 4 MiB tiles216 block and a lone 4 MiB text block: size pass and decode latency;
  - a 1 GiB tiles216 frame of independent blocks without a content size, end to end through
    lz4mi.frame.decompress_frame_device (the measured route) and through decompress_frame_host
    plus the copies around it (what the host route does).

Writes one JSON document (--out, default profiles/sizes/bench.json) and prints it.

  python tools/bench_sizes.py [--blocks 4096] [--text-blocks 256] [--frame-blocks 256] [--reps 7]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "divortio-lz4_amd"), os.path.join(ROOT, "oracle"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

BLOCK = 4 << 20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=4096)
    ap.add_argument("--text-blocks", type=int, default=256)
    ap.add_argument("--frame-blocks", type=int, default=256)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sizes", "bench.json"))
    args = ap.parse_args()

    import numpy as np
    import torch
    import lz4mi
    import oracle as O
    from bench import Batch  # the flagship benchmark's batch set-up
    from lz4mi import frame as F

    lz4mi.init(0)
    stream_obj = torch.cuda.current_stream()
    stream = stream_obj.cuda_stream

    def med_ms(fn):
        """Median launch-stream time of fn (HIP events), after warm-up; the spread beside it."""
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
        return {"median_ms": round(statistics.median(ts), 4), "min_ms": round(min(ts), 4), "max_ms": round(max(ts), 4)}

    def measure(batch, n, first=0):
        """Size pass and batch decode of blocks [first, first + n) of a compressed batch."""
        sizes = torch.full((n,), -1, dtype=torch.int32, device="cuda")
        st = torch.full((n,), -1, dtype=torch.int32, device="cuda")
        off = batch.comp_off[first:first + n].contiguous()
        ln = batch.comp_len[first:first + n].contiguous()
        out_off = batch.raw_off[:n].contiguous()

        def size_pass():
            lz4mi.decoded_sizes_dev(batch.comp.data_ptr(), off.data_ptr(), ln.data_ptr(), sizes.data_ptr(),
                                    st.data_ptr(), n, stream)

        def decode():
            lz4mi.decompress_blocks_dev(batch.comp.data_ptr(), off.data_ptr(), ln.data_ptr(), batch.dec.data_ptr(),
                                        out_off.data_ptr(), batch.raw_len.data_ptr(), batch.dec_len.data_ptr(),
                                        batch.status.data_ptr(), n, stream)

        r = {"blocks": n, "compressed_bytes": int(ln.to(torch.int64).sum().item()), "raw_bytes": n * BLOCK,
             "size_pass": med_ms(size_pass), "decode": med_ms(decode)}
        ok = bool((st == 0).all().item()) and bool((sizes == BLOCK).all().item()) and \
            bool((batch.status[:n] == 0).all().item())
        r["verified"] = ok
        r["size_over_decode"] = round(r["size_pass"]["median_ms"] / r["decode"]["median_ms"], 4)
        r["size_pass_compressed_GBps"] = round(r["compressed_bytes"] / r["size_pass"]["median_ms"] / 1e6, 2)
        return r

    res = {"device": torch.cuda.get_device_name(0), "build_id": lz4mi.build_id(), "block_bytes": BLOCK,
           "timing": f"HIP events on the launch stream, {args.warmup} warm-up launches, median of {args.reps}",
           "batches": {}, "lone_block": {}}
    for gen in ("tiles216", "random", "repetitive", "mix"):
        batch = Batch(torch, lz4mi, args.blocks, gen, 1, stream)
        batch.compress(lz4mi, stream)
        torch.cuda.synchronize()
        res["batches"][gen] = measure(batch, args.blocks)
        if gen == "tiles216":
            res["lone_block"]["tiles216"] = measure(batch, 1, first=3)
        del batch
        torch.cuda.empty_cache()

    n = args.text_blocks
    batch = Batch(torch, lz4mi, n, "repetitive", 1, stream)
    host = np.concatenate([O.generate("text", 100 + b, BLOCK) for b in range(n)])
    batch.raw.copy_(torch.from_numpy(host))
    del host
    batch.compress(lz4mi, stream)
    torch.cuda.synchronize()
    res["batches"]["text"] = measure(batch, n)
    res["lone_block"]["text"] = measure(batch, 1, first=3 % n)
    del batch
    torch.cuda.empty_cache()

    # a frame of independent blocks without a content size: what `lz4` and the reference's stream encoder write
    n = args.frame_blocks
    raw = torch.empty(n * BLOCK, dtype=torch.uint8, device="cuda")
    lz4mi.generate_blocks_dev(raw.data_ptr(), "tiles216", 1, BLOCK, n, stream)
    torch.cuda.synchronize()
    frame = F.compress_frame_sharded(raw, BLOCK, content_checksum=True, add_content_size=False)
    torch.cuda.synchronize()
    fr = {"raw_bytes": n * BLOCK, "frame_bytes": frame.numel(), "blocks": n, "content_checksum": True}
    for verify in (True, False):
        walls = []
        for _ in range(3):
            rep = {}
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = F.decompress_frame_device(frame, verify_checksum=verify, report=rep)
            torch.cuda.synchronize()
            walls.append(time.perf_counter() - t0)
            assert rep["route"] == "measured", rep
        fr["measured_route_ms" if verify else "measured_route_no_checksum_ms"] = [round(w * 1e3, 2) for w in walls]
        fr["verified"] = bool(torch.equal(out, raw))
        del out
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        host = F.decompress_frame_host(frame.cpu().numpy(), verify_checksum=verify)
        out = torch.from_numpy(host).to("cuda")
        torch.cuda.synchronize()
        fr["host_route_ms" if verify else "host_route_no_checksum_ms"] = round((time.perf_counter() - t0) * 1e3, 2)
        fr["host_verified"] = bool(torch.equal(out, raw))
        del out, host
    res["unsized_frame"] = fr

    text = json.dumps(res, indent=1)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
