#!/usr/bin/env python3
"""Block-checksum verification on the device (lz4mi_verify_blocks) on the frame of DESIGN §4.6:
1 GiB of tiles216 in 256 independent 4 MiB blocks, with block and content checksums, with and
without a content size, in one process on device-resident buffers.

  - kernel: verify_blocks_dev over the frame's real payload list (offsets at every residue mod 4)
    against xxh32_blocks_dev(standard=True) over the same list -- the hashing the JS layer's
    verifyBlockChecksum does today, and the yardstick: HIP events on the launch stream, the two
    alternating. The condition: verify's median exceeds xxh32's by no more than xxh32's own
    max - min of the run;
  - end to end: lz4mi.frame.decompress_frame_device with no check, with verify_blocks, and with
    the content checksum only, alternating, a host clock around a synchronise.

Every output is checked: the statuses, the hashes against the stored checksums, one damaged block
found, the decoded bytes against the generated ones. Writes one JSON document (--out, default
profiles/verify/bench.json) and prints it.

  python tools/bench_verify.py [--blocks 256] [--reps 20] [--warmup 3]
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
STEP_CYCLES = 40          # SIMD cycles per stripe step of one chain
CLOCK_HZ = 2.4e9


def stats(ts):
    return {"median_ms": round(statistics.median(ts), 4), "min_ms": round(min(ts), 4), "max_ms": round(max(ts), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=256)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "verify", "bench.json"))
    args = ap.parse_args()

    import torch
    import lz4mi
    from lz4mi import frame as F

    lz4mi.init(0)
    stream_obj = torch.cuda.current_stream()
    stream = stream_obj.cuda_stream
    n = args.blocks
    raw = torch.empty(n * BLOCK, dtype=torch.uint8, device="cuda")
    lz4mi.generate_blocks_dev(raw.data_ptr(), "tiles216", 1, BLOCK, n, stream)
    torch.cuda.synchronize()
    frames = {name: F.compress_frame_sharded(raw, BLOCK, content_checksum=True, add_content_size=sized,
                                             block_checksum=True).clone()
              for name, sized in (("sized", True), ("unsized", False))}
    torch.cuda.synchronize()

    res = {"device": torch.cuda.get_device_name(0), "build_id": lz4mi.build_id(), "block_bytes": BLOCK, "blocks": n,
           "raw_bytes": n * BLOCK,
           "timing": f"{args.warmup} warm-up rounds, {args.reps} timed rounds, the variants alternating within a round; "
                     "kernel: HIP events on the launch stream; end to end: host clock around a synchronise"}

    # ---- the kernel against the batched XXH32 over the same payload list
    frame = frames["sized"]
    meta, pay, word = F.frame_index(frame)
    assert pay.numel() == n and not meta["overflow"] and meta["flg"] & 0x10
    pay = pay.contiguous()
    lens = (word & 0x7FFFFFFF).to(torch.int32).contiguous()
    w32 = torch.where(word >= 2 ** 31, word - 2 ** 32, word).to(torch.int32).contiguous()
    hashes = torch.zeros(n, dtype=torch.int32, device="cuda")
    status = torch.full((n,), -1, dtype=torch.int32, device="cuda")

    def xxh32():
        lz4mi.xxh32_blocks_dev(frame.data_ptr(), pay.data_ptr(), lens.data_ptr(), hashes.data_ptr(), n, 0, stream,
                               standard=True)

    def verify():
        lz4mi.verify_blocks_dev(frame.data_ptr(), frame.numel(), pay.data_ptr(), w32.data_ptr(), status.data_ptr(), n,
                                stream, frame_words=True)

    def timed(fn):
        e0 = torch.cuda.Event(enable_timing=True)
        e1 = torch.cuda.Event(enable_timing=True)
        e0.record(stream_obj)
        fn()
        e1.record(stream_obj)
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    ts = {"xxh32_blocks": [], "verify_blocks": []}
    for r in range(args.warmup + args.reps):
        for name, fn in (("xxh32_blocks", xxh32), ("verify_blocks", verify)):
            t = timed(fn)
            if r >= args.warmup:
                ts[name].append(t)
    pay_h, len_h = pay.cpu().tolist(), lens.to(torch.int64).cpu().tolist()
    host = frame.cpu().numpy()
    stored = [int.from_bytes(host[p + m:p + m + 4].tobytes(), "little") for p, m in zip(pay_h, len_h)]
    got = (hashes.to(torch.int64) & 0xFFFFFFFF).cpu().tolist()
    bad = frame.clone()
    victim = n // 3
    bad[pay_h[victim] + len_h[victim] // 2] ^= 0x20
    st_bad = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    lz4mi.verify_blocks_dev(bad.data_ptr(), bad.numel(), pay.data_ptr(), w32.data_ptr(), st_bad.data_ptr(), n, stream,
                            frame_words=True)
    torch.cuda.synchronize()
    want_bad = [lz4mi.ERR_BLOCK_CHECKSUM if b == victim else 0 for b in range(n)]
    del bad
    k = {name: stats(v) for name, v in ts.items()}
    payload = sum(len_h)
    spread = k["xxh32_blocks"]["max_ms"] - k["xxh32_blocks"]["min_ms"]
    over = k["verify_blocks"]["median_ms"] - k["xxh32_blocks"]["median_ms"]
    res["kernel"] = {
        "frame_bytes": frame.numel(), "payload_bytes": payload, "largest_payload": max(len_h),
        "payload_offsets_mod4": [sum(1 for p in pay_h if p % 4 == r) for r in range(4)],
        "xxh32_blocks": k["xxh32_blocks"], "verify_blocks": k["verify_blocks"],
        "verify_minus_xxh32_median_ms": round(over, 4), "xxh32_max_minus_min_ms": round(spread, 4),
        "condition_met": bool(over <= spread),
        "verify_payload_GBps": round(payload / k["verify_blocks"]["median_ms"] / 1e6, 2),
        "xxh32_payload_GBps": round(payload / k["xxh32_blocks"]["median_ms"] / 1e6, 2),
        "chain_floor_estimate_ms": round(max(len_h) / 16 * STEP_CYCLES / CLOCK_HZ * 1e3, 4),
        "chain_floor_estimate": f"largest payload / 16 stripe steps x {STEP_CYCLES} cycles at {CLOCK_HZ / 1e9} GHz",
        "verified": bool((status == 0).all().item()) and got == stored and st_bad.cpu().tolist() == want_bad,
    }

    # ---- end to end through decompress_frame_device
    variants = (("no_check", {"verify_checksum": False}),
                ("verify_blocks", {"verify_checksum": False, "verify_blocks": True}),
                ("content_checksum", {"verify_checksum": True}))
    res["end_to_end"] = {}
    for fname, route in (("sized", "layout"), ("unsized", "measured")):
        frame = frames[fname]
        walls = {name: [] for name, _ in variants}
        ok = True
        for r in range(args.warmup + args.reps):
            for name, kw in variants:
                rep = {}
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                out = F.decompress_frame_device(frame, report=rep, **kw)
                torch.cuda.synchronize()
                t = (time.perf_counter() - t0) * 1e3
                assert rep["route"] == route, rep
                if r == 0:
                    ok = ok and bool(torch.equal(out, raw))
                del out
                if r >= args.warmup:
                    walls[name].append(t)
        res["end_to_end"][fname] = {"route": route, "frame_bytes": frame.numel(), "verified": ok,
                                    **{name: stats(v) for name, v in walls.items()}}

    text = json.dumps(res, indent=1)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
