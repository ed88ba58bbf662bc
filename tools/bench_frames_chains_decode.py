#!/usr/bin/env python3
"""Dependent frames of more than one block decoded in the frame batch (lz4mi_frames_decompress with
LZ4MI_FRAMES_CHAINS: one wave per frame walks the frame's blocks in order, all frames in one launch) against what
there was before -- the batch declines every such frame and each is decoded alone -- and against the independent
batch of the same contents. In one process, on device-resident frames, per shape (frames x bytes per frame @ block
size, those of tools/bench_frames_chains.py) and content (tiles216, that tool's text), no content checksum:

  - a, chains:        lz4mi_frames_index + lz4mi_frames_decompress with LZ4MI_FRAMES_CHAINS over the dependent frames,
                      HIP events on the launch stream (device time, nothing read back); a_exact: with LZ4MI_JS_EXACT;
  - b, loop:          frame.decompress_frame_device(linked=True) per frame (b_exact: linked="exact"), the route a
                      declined frame takes. Wall clock -- the calls synchronise themselves --, over the first
                      --loop-frames frames (fewer for long frames: --loop-bytes) and scaled to the frame count;
  - c, independent:   the same two calls, no flag, over the independent frames of the same contents, HIP events.

One more leg, on the independent text frames of 1024x256K@64K: the batch with LZ4MI_JS_EXACT without and with the
flag, and the share of frames the batch declines without it (a tail rewrite that reads below a block).
Every output is compared: spec results with the sources, reference-mode results with the loop's.
Writes one JSON document (--out, default profiles/frames_chains_decode/bench.json) and prints it.

  python tools/bench_frames_chains_decode.py [--reps 5] [--warmup 2] [--small] [--shapes 256x1M@64K,...]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "divortio-lz4_amd"), ROOT, os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

from bench_frames_chains import SHAPES, TEXT_BYTES, make_text   # noqa: E402

EXACT_LEG = "1024x256K@64K"
DEPENDENT = 9


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--loop-frames", type=int, default=32)
    ap.add_argument("--loop-bytes", type=int, default=64 << 20, help="at most this many content bytes in leg b")
    ap.add_argument("--shapes", default="", help="comma-separated shape names (default: all)")
    ap.add_argument("--contents", default="tiles216,text", help="comma-separated contents")
    ap.add_argument("--small", action="store_true", help="an eighth of the frames of every shape (a quick look)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "frames_chains_decode", "bench.json"))
    args = ap.parse_args()
    assert args.reps >= 5 or args.small, "the committed numbers are medians of at least 5 runs"

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

    def wall_ms(fn):
        for _ in range(args.warmup):
            fn()
        ts = []
        for _ in range(args.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        return stats(ts)

    class Batch:
        """The two calls over `frames` (a list of device tensors), the results in slots of `slot` bytes."""

        def __init__(self, frames, n, bs):
            self.nf, self.n = len(frames), n
            self.slot = (n + 15) & ~15
            lens = [int(f.numel()) for f in frames]
            offs = [0] * self.nf
            for k in range(1, self.nf):
                offs[k] = offs[k - 1] + lens[k - 1]
            self.arena = torch.cat(frames)
            self.span = torch.tensor([offs, lens], dtype=torch.int64, device="cuda")
            self.nb = self.nf * (-(-n // bs))
            self.blk_in_off = torch.zeros(self.nb, dtype=torch.int64, device="cuda")
            self.blk32 = torch.zeros((3, self.nb), dtype=torch.int32, device="cuda")
            self.fin = torch.zeros(8 * self.nf + 4, dtype=torch.int64, device="cuda")
            self.out = torch.zeros(self.nf * self.slot, dtype=torch.uint8, device="cuda")
            self.out_off = torch.arange(self.nf, dtype=torch.int64, device="cuda") * self.slot
            self.out_cap = torch.full((self.nf,), n, dtype=torch.int64, device="cuda")

        def __call__(self, chains, exact=False):
            lz4mi.frames_index_dev(self.arena.data_ptr(), self.span[0].data_ptr(), self.span[1].data_ptr(), self.nf,
                                   self.blk_in_off.data_ptr(), self.blk32[0].data_ptr(), self.blk32[1].data_ptr(),
                                   self.blk32[2].data_ptr(), self.nb, self.fin.data_ptr(),
                                   self.fin.data_ptr() + 64 * self.nf, stream, js_exact=exact)
            lz4mi.frames_decompress_dev(self.arena.data_ptr(), self.blk_in_off.data_ptr(), self.blk32[0].data_ptr(),
                                        self.blk32[1].data_ptr(), self.blk32[2].data_ptr(), self.nb,
                                        self.fin.data_ptr(), self.nf, self.out.data_ptr(), self.out_off.data_ptr(),
                                        self.out_cap.data_ptr(), stream, js_exact=exact, chains=chains)

        def info(self):
            return self.fin[:8 * self.nf].cpu().numpy().reshape(self.nf, 8).copy()

        def clean(self):
            i = self.info()
            return bool((i[:, 0] == 0).all() and (i[:, 7] == 0).all())

        def result(self, f):
            return self.out[f * self.slot:f * self.slot + self.n]

        def equals(self, raw):
            return all(bool(torch.equal(self.result(f), raw[f * self.n:(f + 1) * self.n])) for f in range(self.nf))

    text = torch.from_numpy(make_text(TEXT_BYTES)).cuda()
    res = {"device": torch.cuda.get_device_name(0), "compute_units": cus, "build_id": lz4mi.build_id(),
           "timing": f"chains and independent: HIP events on the launch stream around lz4mi_frames_index + "
                     f"lz4mi_frames_decompress, {args.warmup} warm-ups, median of {args.reps}; loop: wall clock around "
                     f"calls that synchronise, {args.warmup} warm-ups, median of {args.reps}, over the first frames "
                     f"(loop_frames_measured), scaled to the frame count",
           "shapes": {}}
    for name, nf, n, bs in SHAPES:
        if args.shapes and name not in args.shapes.split(","):
            continue
        if args.small:
            nf = max(4, nf // 8)
        for content in args.contents.split(","):
            raw = torch.empty(nf * n, dtype=torch.uint8, device="cuda")
            if content == "tiles216":
                lz4mi.generate_blocks_dev(raw.data_ptr(), "tiles216", 1, n, nf, stream)
            else:
                for f in range(nf):
                    o = (f * 1048583) % (TEXT_BYTES - n)
                    raw[f * n:(f + 1) * n] = text[o:o + n]
            offs, lens = list(range(0, nf * n, n)), [n] * nf
            rep = {}
            dep = F.compress_frames_device(raw, block_size=bs, independent=False, chains=True, offsets=offs,
                                           lengths=lens, report=rep)
            assert rep["routes"] == ["batch"] * nf
            ind = F.compress_frames_device(raw, block_size=bs, independent=True, offsets=offs, lengths=lens)
            r = {"frames": nf, "frame_content_bytes": n, "block_bytes": bs, "content": content, "raw_bytes": nf * n,
                 "frame_bytes_dependent": sum(int(f.numel()) for f in dep),
                 "frame_bytes_independent": sum(int(f.numel()) for f in ind)}
            A = Batch(dep, n, bs)
            r["chains"] = event_ms(lambda: A(True))
            r["chains_verified"] = A.clean() and A.equals(raw)
            A.out.zero_()
            A(False)
            torch.cuda.synchronize()
            r["declined_without_flag"] = int((A.info()[:, 7] == DEPENDENT).sum())
            A.out.zero_()
            r["chains_exact"] = event_ms(lambda: A(True, True))
            exact_clean = A.clean()

            nloop = max(1, min(nf, args.loop_frames, args.loop_bytes // n))
            kept = [None] * nloop

            def loop(linked):
                for f in range(nloop):
                    kept[f] = F.decompress_frame_device(dep[f], verify_checksum=False, linked=linked)

            # (the loop's reference-mode results against the batch's, which are still in A.out)
            lx = wall_ms(lambda: loop("exact"))
            r["chains_exact_verified"] = exact_clean and all(bool(torch.equal(A.result(f), kept[f])) for f in range(nloop))
            lp = wall_ms(lambda: loop(True))
            r["loop_verified"] = all(bool(torch.equal(kept[f], raw[f * n:(f + 1) * n])) for f in range(nloop))
            r["loop_frames_measured"] = nloop
            r["loop"] = {k: round(v * nf / nloop, 3) for k, v in lp.items()}
            r["loop_exact"] = {k: round(v * nf / nloop, 3) for k, v in lx.items()}
            r["loop_per_frame_ms"] = round(lp["median_ms"] / nloop, 4)
            del A
            Cb = Batch(ind, n, bs)
            r["independent"] = event_ms(lambda: Cb(False))
            r["independent_verified"] = Cb.clean() and Cb.equals(raw)
            r["loop_over_chains"] = round(r["loop"]["median_ms"] / r["chains"]["median_ms"], 2)
            r["loop_exact_over_chains_exact"] = round(r["loop_exact"]["median_ms"] / r["chains_exact"]["median_ms"], 2)
            r["chains_over_independent"] = round(r["chains"]["median_ms"] / r["independent"]["median_ms"], 2)
            r["chains_GBps_raw"] = round(r["raw_bytes"] / r["chains"]["median_ms"] / 1e6, 2)
            r["independent_GBps_raw"] = round(r["raw_bytes"] / r["independent"]["median_ms"] / 1e6, 2)
            r["chains_per_cu"] = round(nf / cus, 2)
            key = f"{name}_{content}"
            if name == EXACT_LEG and content == "text":
                # the reference mode on independent frames: what the batch declines without the flag
                e = {"frames": nf}
                e["without_flag"] = event_ms(lambda: Cb(False, True))
                i0 = Cb.info()
                e["declined_without_flag"] = int((i0[:, 7] == DEPENDENT).sum())
                e["declined_share"] = round(e["declined_without_flag"] / nf, 4)
                e["other_declines_or_errors"] = int(((i0[:, 7] != 0) & (i0[:, 7] != DEPENDENT)).sum() + (i0[:, 0] != 0).sum())
                Cb.out.zero_()
                e["with_flag"] = event_ms(lambda: Cb(True, True))
                ok = Cb.clean()
                for f in range(min(nf, 16)):
                    one = F.decompress_frame_device(ind[f], js_exact=True, verify_checksum=False)
                    ok = ok and bool(torch.equal(Cb.result(f), one))
                e["with_flag_verified"] = ok
                e["note"] = "without_flag times the batch alone: its declined frames still need one call each"
                r["js_exact_independent"] = e
            res["shapes"][key] = r
            print(key, json.dumps(r), flush=True)
            del raw, dep, ind, Cb, kept
            torch.cuda.empty_cache()

    text_json = json.dumps(res, indent=1)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text_json + "\n")
    print(text_json)


if __name__ == "__main__":
    main()
