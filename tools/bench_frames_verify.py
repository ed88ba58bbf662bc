#!/usr/bin/env python3
"""Block checksums of a frame batch checked on the device (lz4mi_frames_verify_blocks) against what there was: the
single-frame verify kernel over the same records, and the ways a caller could check a batch before. In one process,
on device-resident buffers, per shape of tools/bench_frames.py (frames x blocks per frame x block size), the frames
written by frame.compress_frames_device(block_checksum=True, content_checksum=True):

  (a) kernel time, HIP events on the launch stream, nothing read back:
        frames_verify  frames_verify_blocks_dev: the hash pass with per-frame bounds, then the fold;
        verify         verify_blocks_dev(frame_words=True) over the same records with in_total = the arena's size: the
                       parent's kernel on the same work, the yardstick;
        fold_bound     frames_verify_blocks_dev over the same lists with every size word 0: a hash pass with nothing
                       to hash, then the fold over statuses that all fail -- an upper bound of the fold alone;
  (b) end to end, wall clock around calls that synchronise, allocation and read-backs included:
        decompress_frames_device with verify_blocks, without any check, with the content checksum only, and the
        per-frame loop decompress_frame_device(verify_blocks=True);
  (c) every timed variant's output is checked: all statuses 0 and every frame's bytes, and one flipped payload byte
      is found in exactly its block.
Warm-up rounds, then timed rounds; the variants of a group alternate within each round.
Writes one JSON document (--out, default profiles/frames_verify/bench.json) and prints it.

  python tools/bench_frames_verify.py [--reps 10] [--warmup 3] [--small]
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

# name, frames, blocks per frame, block bytes (tools/bench_frames.py SHAPES)
SHAPES = [("4096x1x64K", 4096, 1, 65536), ("1024x16x64K", 1024, 16, 65536), ("64x64x4M", 64, 64, 4 << 20)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--small", action="store_true", help="a sixteenth of the frames of every shape (a quick look)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "frames_verify", "bench.json"))
    args = ap.parse_args()

    import numpy as np
    import torch
    import lz4mi
    from lz4mi import frame as F

    lz4mi.init(0)
    stream_obj = torch.cuda.current_stream()
    stream = stream_obj.cuda_stream

    def stats(ts):
        return {"median_ms": round(statistics.median(ts), 4), "min_ms": round(min(ts), 4), "max_ms": round(max(ts), 4)}

    def rounds(variants, timer):
        """variants: name -> (fn, prepare or None). Every round runs each variant once, the order rotating."""
        names = list(variants)
        ts = {n: [] for n in names}
        for r in range(args.warmup + args.reps):
            for k in range(len(names)):
                n = names[(k + r) % len(names)]
                fn, prepare = variants[n]
                if prepare:
                    prepare()
                t = timer(fn)
                if r >= args.warmup:
                    ts[n].append(t)
        return {n: stats(v) for n, v in ts.items()}

    def event_timer(fn):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream_obj)
        fn()
        e1.record(stream_obj)
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    def wall_timer(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    res = {"device": torch.cuda.get_device_name(0), "build_id": lz4mi.build_id(), "content": "tiles216",
           "timing": f"(a) HIP events on the launch stream, (b) wall clock around calls that synchronise; "
                     f"{args.warmup} warm-up and {args.reps} timed rounds, the variants alternating within a round; "
                     f"median (min, max)",
           "shapes": {}}
    for name, nf, nb, bs in SHAPES:
        if args.small:
            nf = max(4, nf // 16)
        n, content = nf * nb, nb * bs
        raw = torch.empty(n * bs, dtype=torch.uint8, device="cuda")
        lz4mi.generate_blocks_dev(raw.data_ptr(), "tiles216", 1, bs, n, stream)
        frames = F.compress_frames_device(raw, block_size=bs, content_checksum=True, block_checksum=True,
                                          offsets=[f * content for f in range(nf)], lengths=[content] * nf)
        flen = np.array([int(f.numel()) for f in frames], dtype=np.int64)
        foff = np.concatenate([[0], np.cumsum(flen)[:-1]])
        arena = torch.cat(frames)
        del frames
        d_foff, d_flen = torch.from_numpy(foff).cuda(), torch.from_numpy(flen).cuda()
        blk_in_off = torch.zeros(n, dtype=torch.int64, device="cuda")
        blk32 = torch.zeros((3, n), dtype=torch.int32, device="cuda")
        fin = torch.zeros(8 * nf + 4, dtype=torch.int64, device="cuda")
        lz4mi.frames_index_dev(arena.data_ptr(), d_foff.data_ptr(), d_flen.data_ptr(), nf, blk_in_off.data_ptr(),
                               blk32[0].data_ptr(), blk32[1].data_ptr(), blk32[2].data_ptr(), n, fin.data_ptr(),
                               fin.data_ptr() + 64 * nf, stream)
        fin0 = fin.clone()
        h = fin0.cpu().numpy()
        info0 = h[:8 * nf].reshape(nf, 8)
        assert int(h[8 * nf + 1]) == n and not info0[:, 0].any() and not info0[:, 7].any() and (info0[:, 1] & 0x10).all()
        st_new = torch.full((n,), 77, dtype=torch.int32, device="cuda")
        st_old = torch.full((n,), 77, dtype=torch.int32, device="cuda")
        zero_words = torch.zeros(n, dtype=torch.int32, device="cuda")
        pay = blk32[0].cpu().numpy().view(np.uint32) & 0x7FFFFFFF

        def frames_verify(words=blk32[0]):
            lz4mi.frames_verify_blocks_dev(arena.data_ptr(), d_foff.data_ptr(), d_flen.data_ptr(), nf, blk_in_off.data_ptr(),
                                           words.data_ptr(), blk32[1].data_ptr(), n, fin.data_ptr(), st_new.data_ptr(),
                                           stream)

        def verify():
            lz4mi.verify_blocks_dev(arena.data_ptr(), arena.numel(), blk_in_off.data_ptr(), blk32[0].data_ptr(),
                                    st_old.data_ptr(), n, stream, frame_words=True)

        def restore():
            fin.copy_(fin0)

        r = {"frames": nf, "blocks_per_frame": nb, "block_bytes": bs, "raw_bytes": n * bs, "frame_bytes": int(flen.sum()),
             "records": n, "payload_bytes": int(pay.sum()), "largest_payload": int(pay.max())}
        ka = rounds({"frames_verify": (frames_verify, restore), "verify": (verify, None),
                     "fold_bound": (lambda: frames_verify(zero_words), restore)}, event_timer)
        r["kernel"] = ka
        # (c) for (a): the statuses of the last intact round, then one flipped byte in the middle block of a middle frame
        restore()
        frames_verify()
        verify()
        torch.cuda.synchronize()
        ok = bool((st_new == 0).all().item()) and bool((st_old == 0).all().item()) and bool(torch.equal(fin, fin0))
        bf, bb = nf // 2, nb // 2
        b = bf * nb + bb
        pos = int(blk_in_off[b].item()) + int(pay[b]) // 2
        arena[pos] ^= 0x10
        frames_verify()
        verify()
        torch.cuda.synchronize()
        want = torch.zeros(n, dtype=torch.int32, device="cuda")
        want[b] = lz4mi.ERR_BLOCK_CHECKSUM
        fi = fin[:8 * nf].cpu().numpy().reshape(nf, 8)
        want_fi = info0.copy()
        want_fi[bf, 0] = lz4mi.ERR_BLOCK_CHECKSUM
        found = bool(torch.equal(st_new, want)) and bool(torch.equal(st_old, want)) and bool((fi == want_fi).all())
        r["kernel_verified"] = ok
        r["kernel_flip_found_in_its_block"] = found
        restore()
        spread = ka["verify"]["max_ms"] - ka["verify"]["min_ms"]
        r["kernel_excess_ms"] = round(ka["frames_verify"]["median_ms"] - ka["verify"]["median_ms"], 4)
        r["kernel_allowance_ms"] = round(spread + ka["fold_bound"]["median_ms"], 4)
        r["kernel_within_allowance"] = r["kernel_excess_ms"] <= r["kernel_allowance_ms"]
        r["frames_verify_GBps_payload"] = round(r["payload_bytes"] / ka["frames_verify"]["median_ms"] / 1e6, 1)

        # (b) end to end; the flipped byte is still in the arena for the first, checked call of every variant
        offs, lens = foff.tolist(), flen.tolist()
        last = {}

        def wrapper(key, **kw):
            def fn():
                last.pop(key, None)      # (the previous results go back to the allocator first)
                rep = {}
                last[key] = (F.decompress_frames_device(arena, offsets=offs, lengths=lens, return_errors=True,
                                                        report=rep, **kw), rep)
            return fn

        def loop():
            last.pop("loop_verify_blocks", None)
            out = []
            for f in range(nf):
                try:
                    out.append(F.decompress_frame_device(arena[offs[f]:offs[f] + lens[f]], verify_checksum=False,
                                                         verify_blocks=True))
                except lz4mi.Lz4miError as e:
                    out.append(e)
            last["loop_verify_blocks"] = (out, None)

        variants = {"batch_verify_blocks": (wrapper("batch_verify_blocks", verify_checksum=False, verify_blocks=True), None),
                    "batch_no_check": (wrapper("batch_no_check", verify_checksum=False), None),
                    "batch_content_only": (wrapper("batch_content_only", verify_checksum=True), None),
                    "loop_verify_blocks": (loop, None)}

        def outputs_ok(key, bad=None):
            out, rep = last[key]
            for f in range(nf):
                if f == bad:
                    if not (isinstance(out[f], lz4mi.Lz4miError) and out[f].status == lz4mi.ERR_BLOCK_CHECKSUM):
                        return False
                elif isinstance(out[f], Exception) or not torch.equal(out[f], raw[f * content:(f + 1) * content]):
                    return False
            if rep is not None and "bad_block" in rep:
                return rep["bad_block"] == [bb if f == bad else None for f in range(nf)]
            return True

        flip = {}
        for key in ("batch_verify_blocks", "loop_verify_blocks"):
            variants[key][0]()
            flip[key] = outputs_ok(key, bad=bf)
        r["end_to_end_flip_found_in_its_block"] = flip
        arena[pos] ^= 0x10
        torch.cuda.synchronize()
        r["end_to_end"] = rounds(variants, wall_timer)
        r["end_to_end_verified"] = {key: outputs_ok(key) for key in variants}
        r["end_to_end_routes_batch"] = last["batch_verify_blocks"][1]["routes"].count("batch")
        res["shapes"][name] = r
        print(name, json.dumps(r), flush=True)
        del raw, arena, last, blk_in_off, blk32
        torch.cuda.empty_cache()

    text = json.dumps(res, indent=1)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
