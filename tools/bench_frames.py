#!/usr/bin/env python3
"""A batch of device-resident frames decoded by one lz4mi_frames_index + lz4mi_frames_decompress pair against
the only way there was before: a loop of lz4mi_frame_decompress, one synchronous call per frame. In one
process, on device-resident buffers, per shape (frames x blocks per frame x block size):

  - batch:   both calls, HIP events on the launch stream (device time, nothing read back);
  - loop:    frame_decompress_dev per frame (frames without a content size: decompress_frame_device, the
             measured route), wall clock -- the calls synchronise themselves;
  - floor:   decompress_blocks_dev (LZ4MI_FRAME_WORDS) of the same blocks with precomputed lists;
  - wrapper: frame.decompress_frames_device end to end, wall clock, allocation and read-backs included;
  - with content checksums: the batch with LZ4MI_VERIFY_CONTENT, and the host chain
    (frame._verify_content_checksum per frame) over the same results.

Writes one JSON document (--out, default profiles/frames/bench.json) and prints it.

  python tools/bench_frames.py [--reps 5] [--warmup 2] [--small]
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

# name, frames, blocks per frame, block bytes, content size, content checksum
SHAPES = [("4096x1x64K", 4096, 1, 65536, True, False),
          ("1024x16x64K", 1024, 16, 65536, True, False),
          ("1024x16x64K_unsized", 1024, 16, 65536, False, False),
          ("1024x16x64K_checksum", 1024, 16, 65536, True, True),
          ("64x64x4M", 64, 64, 4 << 20, True, False),
          ("64x64x4M_checksum", 64, 64, 4 << 20, True, True)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--small", action="store_true", help="a sixteenth of the frames of every shape (a quick look)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "frames", "bench.json"))
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

    def wall_ms(fn, reps=None, warmup=None):
        for _ in range(args.warmup if warmup is None else warmup):
            fn()
        ts = []
        for _ in range(reps or args.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        return stats(ts)

    def i64(a):
        return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int64)).cuda()

    def build(nf, nb, bs, sized, csum):
        """nf frames of nb tiles216 blocks of bs bytes, back to back in one device array, assembled on the device:
        compress_blocks_dev, frame_pack_dev for the records, one scatter for the headers and checksums."""
        n = nf * nb
        raw = torch.empty(n * bs, dtype=torch.uint8, device="cuda")
        lz4mi.generate_blocks_dev(raw.data_ptr(), "tiles216", 1, bs, n, stream)
        raw_off = torch.arange(n, dtype=torch.int64, device="cuda") * bs
        raw_len = torch.full((n,), bs, dtype=torch.int32, device="cuda")
        bound = (lz4mi.compress_bound(bs) + 15) & ~15
        comp = torch.empty(n * bound, dtype=torch.uint8, device="cuda")
        comp_off = torch.arange(n, dtype=torch.int64, device="cuda") * bound
        comp_len = torch.zeros(n, dtype=torch.int32, device="cuda")
        lz4mi.compress_blocks_dev(raw.data_ptr(), raw_off.data_ptr(), raw_len.data_ptr(), comp.data_ptr(),
                                  comp_off.data_ptr(), comp_len.data_ptr(), n, stream)
        cl = comp_len.cpu().numpy().astype(np.int64)
        rec = 4 + np.where((cl > 0) & (cl < bs), cl, bs)
        head = np.frombuffer(F.header(bs, True, csum, nb * bs if sized else None), dtype=np.uint8)
        flen = head.size + rec.reshape(nf, nb).sum(axis=1) + 4 + (4 if csum else 0)
        foff = np.concatenate([[0], np.cumsum(flen)[:-1]])
        within = np.cumsum(rec.reshape(nf, nb), axis=1) - rec.reshape(nf, nb)
        rec_off = (foff[:, None] + head.size + within).reshape(-1)
        arena = torch.zeros(int(flen.sum()), dtype=torch.uint8, device="cuda")      # (the EndMarks are these zeros)
        d_rec_off = i64(rec_off)
        lz4mi.frame_pack_dev(raw.data_ptr(), raw_off.data_ptr(), raw_len.data_ptr(), comp.data_ptr(),
                             comp_off.data_ptr(), comp_len.data_ptr(), arena.data_ptr(), d_rec_off.data_ptr(), n, stream)
        pos = i64((foff[:, None] + np.arange(head.size)[None, :]).reshape(-1))
        arena[pos] = torch.from_numpy(np.tile(head, nf)).cuda()
        if csum:
            c_off = torch.arange(nf, dtype=torch.int64, device="cuda") * (nb * bs)
            c_len = torch.full((nf,), nb * bs, dtype=torch.int32, device="cuda")
            dig = torch.zeros(nf, dtype=torch.int32, device="cuda")
            lz4mi.xxh32_blocks_dev(raw.data_ptr(), c_off.data_ptr(), c_len.data_ptr(), dig.data_ptr(), nf, 0, stream)
            pos = i64(((foff + flen - 4)[:, None] + np.arange(4)[None, :]).reshape(-1))
            arena[pos] = dig.view(torch.uint8)
        torch.cuda.synchronize()
        del comp
        return raw, arena, foff, flen

    res = {"device": torch.cuda.get_device_name(0), "build_id": lz4mi.build_id(), "content": "tiles216",
           "timing": f"batch and floor: HIP events on the launch stream; loop, wrapper and host chain: wall clock "
                     f"around calls that synchronise; {args.warmup} warm-ups, median of {args.reps}",
           "shapes": {}}
    for name, nf, nb, bs, sized, csum in SHAPES:
        if args.small:
            nf = max(4, nf // 16)
        raw, arena, foff, flen = build(nf, nb, bs, sized, csum)
        n, content = nf * nb, nb * bs
        slot = (content + 15) & ~15
        d_foff, d_flen = i64(foff), i64(flen)
        blk_in_off = torch.zeros(n, dtype=torch.int64, device="cuda")
        blk32 = torch.zeros((3, n), dtype=torch.int32, device="cuda")
        fin = torch.zeros(8 * nf + 4, dtype=torch.int64, device="cuda")
        out = torch.zeros(nf * slot, dtype=torch.uint8, device="cuda")
        out_off = torch.arange(nf, dtype=torch.int64, device="cuda") * slot
        out_cap = torch.full((nf,), content, dtype=torch.int64, device="cuda")

        def batch(verify=False):
            lz4mi.frames_index_dev(arena.data_ptr(), d_foff.data_ptr(), d_flen.data_ptr(), nf, blk_in_off.data_ptr(),
                                   blk32[0].data_ptr(), blk32[1].data_ptr(), blk32[2].data_ptr(), n, fin.data_ptr(),
                                   fin.data_ptr() + 64 * nf, stream)
            lz4mi.frames_decompress_dev(arena.data_ptr(), blk_in_off.data_ptr(), blk32[0].data_ptr(),
                                        blk32[1].data_ptr(), blk32[2].data_ptr(), n, fin.data_ptr(), nf, out.data_ptr(),
                                        out_off.data_ptr(), out_cap.data_ptr(), stream, verify_content=verify)

        def index_only():
            lz4mi.frames_index_dev(arena.data_ptr(), d_foff.data_ptr(), d_flen.data_ptr(), nf, blk_in_off.data_ptr(),
                                   blk32[0].data_ptr(), blk32[1].data_ptr(), blk32[2].data_ptr(), n, fin.data_ptr(),
                                   fin.data_ptr() + 64 * nf, stream)

        def same():
            return all(bool(torch.equal(out[f * slot:f * slot + content], raw[f * content:(f + 1) * content]))
                       for f in range(nf))

        r = {"frames": nf, "blocks_per_frame": nb, "block_bytes": bs, "content_size": sized, "content_checksum": csum,
             "raw_bytes": n * bs, "frame_bytes": int(flen.sum())}
        r["batch"] = event_ms(batch)
        h = fin.cpu().numpy()
        info = h[:8 * nf].reshape(nf, 8)
        r["batch_verified"] = bool((info[:, 0] == 0).all() and (info[:, 7] == 0).all() and h[8 * nf + 1] == n) and same()
        r["index_only"] = event_ms(index_only)
        if csum:
            out.zero_()
            r["batch_verify_content"] = event_ms(lambda: batch(True))
            info = fin[:8 * nf].cpu().numpy().reshape(nf, 8)
            r["batch_verify_content_verified"] = bool((info[:, 0] == 0).all() and (info[:, 7] == 0).all()) and same()
            ends = info[:, 5].tolist()

            def host_chain():
                for f in range(nf):
                    F._verify_content_checksum(arena[int(foff[f]):int(foff[f] + flen[f])], int(ends[f]),
                                               out[f * slot:f * slot + content])
            r["host_chain"] = wall_ms(host_chain)

        # the floor: the same blocks, lists precomputed
        b_out_off = (torch.arange(nf, dtype=torch.int64, device="cuda")[:, None] * slot +
                     torch.arange(nb, dtype=torch.int64, device="cuda")[None, :] * bs).reshape(-1).contiguous()
        b_cap = torch.full((n,), bs, dtype=torch.int32, device="cuda")
        b_len = torch.zeros(n, dtype=torch.int32, device="cuda")
        b_st = torch.zeros(n, dtype=torch.int32, device="cuda")
        out.zero_()
        r["floor_decompress_blocks"] = event_ms(lambda: lz4mi.decompress_blocks_dev(
            arena.data_ptr(), blk_in_off.data_ptr(), blk32[0].data_ptr(), out.data_ptr(), b_out_off.data_ptr(),
            b_cap.data_ptr(), b_len.data_ptr(), b_st.data_ptr(), n, stream, frame_words=True))
        r["floor_verified"] = bool((b_st == 0).all().item()) and same()

        # the loop: one synchronous call per frame
        out.zero_()
        if sized:
            def loop():
                for f in range(nf):
                    lz4mi.frame_decompress_dev(arena.data_ptr() + int(foff[f]), int(flen[f]), out.data_ptr() + f * slot,
                                               content, stream)
            r["loop"] = wall_ms(loop)
            r["loop_call"] = "frame_decompress_dev"
            r["loop_verified"] = same()
        else:
            def loop():
                for f in range(nf):
                    F.decompress_frame_device(arena[int(foff[f]):int(foff[f] + flen[f])], verify_checksum=False)
            r["loop"] = wall_ms(loop)
            r["loop_call"] = "decompress_frame_device (measured route)"

        rep = {}
        r["wrapper"] = wall_ms(lambda: F.decompress_frames_device(arena, offsets=foff.tolist(), lengths=flen.tolist(),
                                                                  verify_checksum=csum, report=rep))
        r["wrapper_routes_batch"] = rep["routes"].count("batch")
        r["wrapper_index_calls"] = rep["index_calls"]
        r["loop_over_batch"] = round(r["loop"]["median_ms"] / r["batch"]["median_ms"], 2)
        r["batch_over_floor"] = round(r["batch"]["median_ms"] / r["floor_decompress_blocks"]["median_ms"], 3)
        r["batch_GBps_raw"] = round(r["raw_bytes"] / r["batch"]["median_ms"] / 1e6, 1)
        res["shapes"][name] = r
        print(name, json.dumps(r), flush=True)
        del raw, arena, out, blk_in_off, blk32, b_out_off
        torch.cuda.empty_cache()

    text = json.dumps(res, indent=1)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
