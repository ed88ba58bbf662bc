"""Device-resident LZ4 frames over one or many GPUs (SURVEY.md §8e/§8f rank 1;
BASELINE config 4: an independent-block frame with content checksum, sharded).

The frame layout is the reference writer's (src/buffer/bufferCompress.js:100-259):

    header (:147-178)  magic, FLG, BD, [content size u64], [dictId], HC
    records (:209-239) per block: LE32 size + payload (compressed when 0 < c < n,
                       else n | 0x80000000 + the raw bytes)  [+ LE32 block checksum]
    EndMark (:244), [content checksum (:248-252): xxHash32 of the whole input]

Each rank holds a contiguous shard of the input (every shard but the last a whole
number of blocks), compresses it with the batch encoder and packs its records on
its GPU (`lz4mi_frame_pack`). The records are concatenated on the root in rank
order: an all-gather of the record byte counts, then point-to-point sends of
exactly those bytes (RCCL over xGMI with the nccl backend; any torch.distributed
backend works). The content checksum is one serial XXH32 chain over the whole
input: it runs on root's host over host-staged shards (the ranks share
the host: each copies its shard into /dev/shm, nothing crosses xGMI for it), the
chain on a worker thread while the next piece is copied.

`codec` is the per-rank block compressor: the GPU kernels by default
(DeviceCodec). Tests on CPU pass a stand-in with the same two methods so the
collectives, layout and checksum path (this module) run under gloo.
"""
import os
import tempfile
import threading

import numpy as np

from . import shard

MAGIC = b"\x04\x22\x4d\x18"
CHECKSUM_PIECE = 64 << 20        # content-checksum streaming granularity


def block_id(nbytes):
    """getBlockId (bufferCompress.js:77-82)."""
    if not nbytes or nbytes <= 65536:
        return 4
    if nbytes <= 262144:
        return 5
    if nbytes <= 1048576:
        return 6
    return 7


def header(block_size, independent=True, content_checksum=False, content_size=None, dict_id=None,
           block_checksum=False):
    """Frame header bytes exactly as bufferCompress.js:147-178 writes them (FLG bit 0x10 when
    block_checksum, which the reference never sets)."""
    import lz4mi
    bd = block_id(block_size)
    flg = 0x40
    if independent:
        flg |= 0x20
    if block_checksum:
        flg |= 0x10
    if content_checksum:
        flg |= 0x04
    if dict_id is not None:
        flg |= 0x01
    if content_size is not None:
        flg |= 0x08
    h = bytearray(MAGIC) + bytes([flg, (bd & 7) << 4])
    if content_size is not None:
        h += int(content_size).to_bytes(8, "little")
    if dict_id is not None:
        h += int(dict_id & 0xFFFFFFFF).to_bytes(4, "little")
    h.append((lz4mi.xxh32(bytes(h[4:])) >> 8) & 0xFF)
    return bytes(h)


class DeviceCodec:
    """The GPU path: batch encoder + device frame records (one stream). Its buffers are kept
    for the next call of the same shape (allocation is not part of a frame's kernel time);
    `last_kernel_s` is the encoder + record packing time from HIP events on the stream. The
    returned records are a view of that workspace, valid until the next call."""

    def __init__(self, stream=None):
        import torch
        self.torch = torch
        self.stream = stream if stream is not None else torch.cuda.current_stream()
        self.ws = None
        self.last_kernel_s = None

    def _workspace(self, nb, n, block_size, block_checksum, dev):
        import lz4mi
        torch = self.torch
        key = (nb, n, block_size, block_checksum, str(dev))
        if self.ws is None or self.ws["key"] != key:
            self.ws = None
            raw_off = torch.arange(nb, dtype=torch.int64, device=dev) * block_size
            raw_len = torch.clamp(n - raw_off, max=block_size).to(torch.int32)
            slot = (lz4mi.compress_bound(block_size) + 255) & ~255
            rec_max = int((4 + raw_len.to(torch.int64) + (4 if block_checksum else 0)).sum().item())
            self.ws = {"key": key, "raw_off": raw_off, "raw_len": raw_len,
                       "comp": torch.empty(nb * slot, dtype=torch.uint8, device=dev),
                       "comp_off": torch.arange(nb, dtype=torch.int64, device=dev) * slot,
                       "comp_len": torch.zeros(nb, dtype=torch.int32, device=dev),
                       "out": torch.empty(max(1, rec_max), dtype=torch.uint8, device=dev)}
        return self.ws

    def records(self, raw, block_size, block_checksum):
        """This rank's frame records (uint8 device tensor) for raw (uint8 device tensor)."""
        import lz4mi
        torch = self.torch
        s = self.stream.cuda_stream
        n = raw.numel()
        nb = -(-n // block_size)
        self.last_kernel_s = None
        if nb == 0:
            return torch.empty(0, dtype=torch.uint8, device=raw.device)
        w = self._workspace(nb, n, block_size, block_checksum, raw.device)
        e0 = torch.cuda.Event(enable_timing=True)
        e1 = torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(self.stream):
            e0.record(self.stream)
            lz4mi.compress_blocks_dev(raw.data_ptr(), w["raw_off"].data_ptr(), w["raw_len"].data_ptr(),
                                      w["comp"].data_ptr(), w["comp_off"].data_ptr(), w["comp_len"].data_ptr(), nb, s)
            rec = shard.record_sizes(w["comp_len"], w["raw_len"]) + (4 if block_checksum else 0)
            rec_off = torch.cumsum(rec, 0) - rec
            lz4mi.frame_pack_dev(raw.data_ptr(), w["raw_off"].data_ptr(), w["raw_len"].data_ptr(), w["comp"].data_ptr(),
                                 w["comp_off"].data_ptr(), w["comp_len"].data_ptr(), w["out"].data_ptr(),
                                 rec_off.data_ptr(), nb, s, block_checksum=block_checksum)
            e1.record(self.stream)
        self.stream.synchronize()
        self.last_kernel_s = e0.elapsed_time(e1) / 1e3
        total = int((rec_off[-1] + rec[-1]).item())
        return w["out"][:total]


class _ChecksumWorker:
    """Host streaming XXH32 on a worker thread (ctypes calls drop the GIL), fed in order."""

    def __init__(self, seed=0):
        import queue
        import lz4mi
        self.h = lz4mi.XXHash32(seed, len64=True)
        self.q = queue.Queue(maxsize=2)
        self.t = threading.Thread(target=self._run, daemon=True)
        self.t.start()

    def _run(self):
        while True:
            a = self.q.get()
            if a is None:
                return
            self.h.update(a)

    def feed(self, host_bytes):
        self.q.put(host_bytes)

    def digest(self):
        self.q.put(None)
        self.t.join()
        return self.h.digest()


_STAGE_PIECE = 256 << 20
_stage_calls = [0]


def _dist_ctx(group):
    import torch.distributed as dist
    multi = dist.is_available() and dist.is_initialized()
    world = dist.get_world_size(group) if multi else 1
    rank = dist.get_rank(group) if multi else 0
    return dist, multi, world, rank


def _shm_dir():
    return "/dev/shm" if os.path.isdir("/dev/shm") else tempfile.gettempdir()


def _shm_free():
    try:
        st = os.statvfs(_shm_dir())
        return st.f_bavail * st.f_frsize
    except OSError:
        return 0


def _sent_checksum(shard, sizes, dist, group, world, rank, root, seed):
    """staged_checksum's route when the shared memory filesystem cannot hold the shards:
    every other rank sends its shard to root in _STAGE_PIECE pieces over the group (device
    tensors over RCCL with the nccl backend), root hashes them in rank order as they come."""
    import torch
    g = (lambda r: dist.get_global_rank(group, r)) if group is not None else (lambda r: r)
    if rank != root:
        n = shard.numel()
        for p in range(0, n, _STAGE_PIECE):
            dist.send(shard[p:p + _STAGE_PIECE].contiguous(), dst=g(root), group=group)
        return None
    w = _ChecksumWorker(seed)
    for r in range(world):
        if r == root:
            for a in _host_pieces(shard):
                w.feed(a)
            continue
        if not sizes[r]:
            continue
        buf = torch.empty(min(_STAGE_PIECE, sizes[r]), dtype=torch.uint8, device=shard.device)
        for p in range(0, sizes[r], _STAGE_PIECE):
            m = min(_STAGE_PIECE, sizes[r] - p)
            dist.recv(buf[:m], src=g(r), group=group)
            for a in _host_pieces(buf[:m]):
                w.feed(a.copy())     # the pinned piece is reused by the next recv
    return w.digest()


def _host_pieces(t, piece=_STAGE_PIECE, nbuf=4):
    """Numpy views of consecutive pieces of a 1-D uint8 tensor. A device tensor goes through
    `nbuf` rotating pinned buffers (full-rate device-to-host copies); a piece's buffer is
    reused `nbuf` pieces later, after _ChecksumWorker (at most 3 pieces queued or in
    hand) has finished with it."""
    import torch
    n = t.numel()
    if t.device.type != "cuda":
        for p in range(0, n, piece):
            yield t[p:p + piece].numpy()
        return
    bufs = [torch.empty(min(piece, n), dtype=torch.uint8, pin_memory=True) for _ in range(min(nbuf, -(-n // piece)))]
    for k, p in enumerate(range(0, n, piece)):
        m = min(piece, n - p)
        b = bufs[k % len(bufs)][:m]
        b.copy_(t[p:p + m])
        yield b.numpy()


def _host_id():
    """This host's identity as an int64 (host name + boot id): ranks whose ids match share a
    /dev/shm, the precondition of the host-staged checksum route."""
    import hashlib
    import socket
    boot = ""
    try:
        with open("/proc/sys/kernel/random/boot_id") as f:
            boot = f.read().strip()
    except OSError:
        pass
    h = hashlib.sha256((socket.gethostname() + "|" + boot).encode()).digest()
    return int.from_bytes(h[:8], "little") & 0x7FFFFFFFFFFFFFFF


class ContentChecksum:
    """The frame's content checksum: XXH32 (the reference's variant, 64-bit length) of every
    rank's shard concatenated in rank order, on root's host (one serial chain, so one
    core). Three steps, so the chain can run beside other work:

      ContentChecksum(n, dev, group, root)   collectives, main thread: shard sizes, whether
                                             all ranks share root's host and /dev/shm has room
      .start(shard)                          no collectives: a background thread; on root it
                                             hashes root's shard (device-to-host through pinned
                                             buffers on a side stream, the chain on a worker
                                             thread), then each other rank's /dev/shm segment
                                             as soon as that rank's done-marker appears; on the
                                             other ranks it writes the shard into its segment
      .finish()                              joins, then one all-reduce of a success flag, so a
                                             failure on any rank raises on every rank

    When the ranks do not share a host (or tmpfs lacks room: a memmap written past a full tmpfs
    is a SIGBUS, not an exception), the shards go to root over the group in finish() instead
    (_sent_checksum), which is not overlapped. Returns the digest on root, None elsewhere."""

    POLL_S = 0.0005
    DEADLINE_S = 900.0

    def __init__(self, n, dev, group=None, root=0, seed=0):
        import torch
        self.dist, self.multi, self.world, self.rank = _dist_ctx(group)
        self.group, self.root, self.seed, self.dev = group, root, seed, dev
        self.n = n
        self.error = None
        self.digest = None
        self.thread = None
        self.elapsed = 0.0
        self.route = "single"
        if not self.multi:
            self.sizes = [n]
            return
        dist = self.dist
        mine = torch.tensor([n, _host_id()], dtype=torch.int64, device=dev)
        allv = [torch.zeros(2, dtype=torch.int64, device=dev) for _ in range(self.world)]
        dist.all_gather(allv, mine, group=group)
        allv = [[int(x) for x in v.tolist()] for v in allv]
        self.sizes = [v[0] for v in allv]
        same_host = all(v[1] == allv[0][1] for v in allv)
        need = sum(self.sizes[r] for r in range(self.world) if r != root)
        ok = torch.tensor([1 if same_host and _shm_free() >= need + (1 << 30) else 0], dtype=torch.int32, device=dev)
        dist.all_reduce(ok, op=dist.ReduceOp.MIN, group=group)
        if not int(ok.item()):
            self.route = "send"
            return
        self.route = "shm"
        if self.rank == root:    # abort markers of this process's earlier calls
            import glob
            for f in glob.glob(os.path.join(_shm_dir(), f"lz4mi_stage_{os.getpid()}_*.abort")):
                try:
                    os.unlink(f)
                except OSError:
                    pass
        _stage_calls[0] += 1
        tag = torch.tensor([os.getpid(), _stage_calls[0]], dtype=torch.int64, device=dev)
        dist.broadcast(tag, src=self._g(root), group=group)
        self.tag = [int(x) for x in tag.tolist()]

    def _g(self, r):
        return self.dist.get_global_rank(self.group, r) if self.group is not None else r

    def _path(self, r, suffix=""):
        return os.path.join(_shm_dir(), f"lz4mi_stage_{self.tag[0]}_{self.tag[1]}_{r}.bin{suffix}")

    def start(self, shard):
        """Start the chain on `shard`. Work already queued on the caller's current stream that
        writes `shard` is waited for (an event recorded here, waited on by the side stream), so
        the caller need not synchronise first."""
        self.shard = shard
        self.ready = None
        self.cancel = False
        if self.route == "send":
            return self
        if shard.device.type == "cuda":
            import torch
            self.ready = torch.cuda.Event()
            self.ready.record(torch.cuda.current_stream(shard.device))
        self.thread = threading.Thread(target=self._run, daemon=True)
        self.thread.start()
        return self

    def abort(self):
        """Stop the chain after an error between start() and finish() (no collectives): the
        thread ends at its next poll or staging piece (a writer stops between pieces and writes
        no marker), and this call's staging files of this rank (all ranks' on root) are removed."""
        self.cancel = True
        if self.route == "shm" and self.rank == self.root:
            # the other ranks' writers may still be copying: a marker tells them to stop between
            # pieces and remove their own file; the files of ranks already done are removed here
            # (zero bytes, removed by root's next ContentChecksum)
            with open(self._path(self.root, ".abort"), "w"):
                pass
        if getattr(self, "thread", None) is not None:
            self.thread.join()
        if self.route == "shm":
            for r in (range(self.world) if self.rank == self.root else [self.rank]):
                for suf in ("", ".done", ".err", ".done.tmp", ".err.tmp"):
                    if r != self.rank and suf == "" and not (os.path.exists(self._path(r, ".done")) or
                                                             os.path.exists(self._path(r, ".err"))):
                        continue   # still being written: its writer removes it on seeing the marker
                    try:
                        os.unlink(self._path(r, suf))
                    except OSError:
                        pass

    def _run(self):
        import time
        import torch
        t0 = time.perf_counter()
        try:
            ctx = torch.cuda.device(self.shard.device) if self.shard.device.type == "cuda" else None
            side = torch.cuda.Stream(self.shard.device) if ctx is not None else None
            if side is not None and self.ready is not None:
                side.wait_event(self.ready)      # the shard's producers on the caller's stream
            if ctx is not None:
                ctx.__enter__()
            try:
                if ctx is not None:
                    with torch.cuda.stream(side):
                        self._work()
                else:
                    self._work()
            finally:
                if ctx is not None:
                    ctx.__exit__(None, None, None)
        except BaseException as e:     # reported by finish() on every rank
            self.error = e
        self.elapsed = time.perf_counter() - t0

    def _work(self):
        import time
        import torch
        shard = self.shard
        if self.route == "single" or self.rank == self.root:
            w = _ChecksumWorker(self.seed)
            try:
                for r in range(self.world):
                    if r == self.root or self.route == "single":
                        for a in _host_pieces(shard):
                            w.feed(a)
                        continue
                    deadline = time.perf_counter() + self.DEADLINE_S
                    while not os.path.exists(self._path(r, ".done")):
                        if self.cancel:
                            raise RuntimeError("lz4mi: content checksum aborted")
                        if os.path.exists(self._path(r, ".err")):
                            raise RuntimeError(f"lz4mi: rank {r} failed to stage its shard for the content checksum")
                        if time.perf_counter() > deadline:
                            raise TimeoutError(f"lz4mi: rank {r} did not stage its shard for the content checksum")
                        time.sleep(self.POLL_S)
                    if self.sizes[r]:
                        mm = np.memmap(self._path(r), dtype=np.uint8, mode="r", shape=(self.sizes[r],))
                        for p in range(0, self.sizes[r], _STAGE_PIECE):
                            w.feed(mm[p:p + _STAGE_PIECE])
                        del mm
            finally:
                self.digest = w.digest()
            return
        n = shard.numel()
        marker = ".err"
        try:
            if n:
                mm = np.memmap(self._path(self.rank), dtype=np.uint8, mode="w+", shape=(n,))
                for p in range(0, n, _STAGE_PIECE):
                    # abort() on this rank, or on root (its marker): stop between pieces, leave no files
                    if self.cancel or os.path.exists(self._path(self.root, ".abort")):
                        del mm
                        marker = None
                        raise RuntimeError("lz4mi: content checksum aborted")
                    m = min(_STAGE_PIECE, n - p)
                    torch.from_numpy(mm[p:p + m]).copy_(shard[p:p + m])
                mm.flush()
                del mm
            marker = ".done"
        except BaseException:
            if os.path.exists(self._path(self.rank)):
                os.unlink(self._path(self.rank))
            raise
        finally:
            if marker is not None and not self.cancel and not os.path.exists(self._path(self.root, ".abort")):
                tmp = self._path(self.rank, marker + ".tmp")
                with open(tmp, "w") as f:
                    f.write(marker)
                os.rename(tmp, self._path(self.rank, marker))

    def finish(self):
        """Join the background chain; raises on every rank if any rank failed. Returns the
        digest on root (None elsewhere)."""
        import torch
        if self.route == "send":
            return _sent_checksum(self.shard, self.sizes, self.dist, self.group, self.world, self.rank, self.root,
                                  self.seed)
        if self.thread is not None:
            self.thread.join()
        if self.multi:
            ok = torch.tensor([0 if self.error is not None else 1], dtype=torch.int32, device=self.dev)
            self.dist.all_reduce(ok, op=self.dist.ReduceOp.MIN, group=self.group)
            if self.rank == self.root:          # every rank is past its writes: remove what is left
                for r in range(self.world):
                    for suf in ("", ".done", ".err"):
                        if os.path.exists(self._path(r, suf)):
                            os.unlink(self._path(r, suf))
            if not int(ok.item()):
                raise self.error if self.error is not None else RuntimeError(
                    "lz4mi: the content checksum failed on another rank")
        elif self.error is not None:
            raise self.error
        return self.digest if (self.rank == self.root or not self.multi) else None


def staged_checksum(shard, group=None, root=0, seed=0):
    """XXH32 (the reference's variant, 64-bit length) of every rank's shard concatenated in
    rank order, on root's host (ContentChecksum, run to completion). Returns the digest on
    root, None elsewhere."""
    return ContentChecksum(shard.numel(), shard.device, group, root, seed).start(shard).finish()


def _phase(timings, key, t0, dev, group=None):
    """Close a timed phase: device work done, all ranks of `group` through it (barrier). Without
    `timings` nothing is synchronised."""
    import time
    import torch
    import torch.distributed as dist
    if timings is None:
        return t0
    if dev.type == "cuda":
        torch.cuda.synchronize(dev)
    if dist.is_available() and dist.is_initialized():
        dist.barrier(group=group)
    t = time.perf_counter()
    timings[key] = timings.get(key, 0.0) + (t - t0)
    return t


def compress_frame_sharded(raw, block_size=4194304, content_checksum=True, add_content_size=True,
                           block_checksum=False, codec=None, group=None, root=0, timings=None):
    """One LZ4 frame of every rank's shard, concatenated in rank order, on `root`.

    raw: this rank's shard, a 1-D uint8 tensor (device tensor for the GPU codec). Every
    shard but the last rank's must be a whole number of blocks. Returns the frame as a
    uint8 tensor on root's device (None on the other ranks). Without torch.distributed
    initialised this is the single-GPU frame. Every collective moves tensors of raw's
    device (RCCL over xGMI for CUDA tensors, gloo for CPU ones). `timings` (dict) gets the
    phases, each closed by a barrier: kernel (compress + records), collective (records to
    root), checksum (host-staged content checksum), assemble (header + EndMark on root)."""
    import time
    import torch
    block_size = shard.BLOCK_MAX_SIZES[block_id(block_size)]
    codec = codec or DeviceCodec()
    dist, multi, world, rank = _dist_ctx(group)
    n = raw.numel()
    dev = raw.device
    t0 = time.perf_counter()
    if multi:
        t = torch.tensor([n], dtype=torch.int64, device=dev)
        all_n = [torch.zeros(1, dtype=torch.int64, device=dev) for _ in range(world)]
        dist.all_gather(all_n, t, group=group)
        sizes = [int(x.item()) for x in all_n]
    else:
        sizes = [n]
    for r in range(world - 1):
        if sizes[r] % block_size:
            raise ValueError("lz4mi: every shard but the last must hold whole blocks")
    # the content checksum reads only the raw input: its chain starts now, beside the
    # kernel and the collective (bufferCompress.js:244-252 hashes the same bytes at the end)
    ck = ContentChecksum(n, dev, group, root).start(raw) if content_checksum else None
    try:
        t0 = _phase(timings, "setup", t0, dev, group)
        records = codec.records(raw, block_size, block_checksum)
        if timings is not None and getattr(codec, "last_kernel_s", None) is not None:
            timings["kernel_device"] = timings.get("kernel_device", 0.0) + codec.last_kernel_s
        t0 = _phase(timings, "kernel", t0, dev, group)
        body = shard.gather_records_to_root(records, root=root, group=group) if multi else records
        t0 = _phase(timings, "collective", t0, dev, group)
    except BaseException:
        if ck is not None:
            ck.abort()
        raise
    csum = ck.finish() if ck is not None else None
    if timings is not None and ck is not None:
        timings["checksum_chain"] = timings.get("checksum_chain", 0.0) + ck.elapsed
    t0 = _phase(timings, "checksum_wait", t0, dev, group)
    if rank != root:
        _phase(timings, "assemble", t0, dev, group)
        return None
    total = sum(sizes)
    hdr = header(block_size, True, content_checksum, total if add_content_size else None, None, block_checksum)
    tail = b"\x00\x00\x00\x00" + (int(csum).to_bytes(4, "little") if content_checksum else b"")
    out = torch.empty(len(hdr) + body.numel() + len(tail), dtype=torch.uint8, device=dev)
    out[:len(hdr)] = torch.frombuffer(bytearray(hdr), dtype=torch.uint8).to(dev)
    out[len(hdr):len(hdr) + body.numel()] = body
    out[len(hdr) + body.numel():] = torch.frombuffer(bytearray(tail), dtype=torch.uint8).to(dev)
    _phase(timings, "assemble", t0, dev, group)
    return out


def frame_index(frame):
    """(info, pay_off, size_word) of a frame: the payload position and raw size word of every
    block in order (bufferDecompress.js:133-192). A CUDA frame is walked on its device
    (lz4mi_frame_index), a host one on the host. info: flg, content_size, block_max, end."""
    import torch
    if frame.device.type == "cuda":
        import lz4mi
        dev = frame.device
        n = frame.numel()
        cap = n // 4 + 2
        pay = torch.empty(cap, dtype=torch.int64, device=dev)
        word = torch.empty(cap, dtype=torch.int32, device=dev)
        info = torch.zeros(8, dtype=torch.int64, device=dev)
        s = torch.cuda.current_stream(dev)
        lz4mi.frame_index_dev(frame.data_ptr(), n, pay.data_ptr(), word.data_ptr(), cap, info.data_ptr(),
                              s.cuda_stream)
        h = info.cpu().tolist()
        if h[0]:
            raise lz4mi.Lz4miError(int(h[0]))
        nb = int(h[3])
        meta = {"flg": int(h[1]), "content_size": int(h[2]), "block_max": int(h[6]), "end": int(h[5]),
                "overflow": int(h[7])}
        return meta, pay[:nb], word[:nb].to(torch.int64) & 0xFFFFFFFF
    import lz4mi
    f = frame.numpy()
    try:
        info, blocks = shard.frame_blocks(f)
    except ValueError:
        raise lz4mi.Lz4miError(lz4mi.ERR_MAGIC)
    if ((info["flg"] & 0xC0) >> 6) != 1:
        raise lz4mi.Lz4miError(lz4mi.ERR_VERSION)
    pay = torch.tensor([p for p, _, _ in blocks], dtype=torch.int64)
    word = torch.tensor([(nb | (0x80000000 if st else 0)) for _, nb, st in blocks], dtype=torch.int64)
    # as lz4mi_frame_index_kernel: the walk ran past the frame's end (a payload, its block
    # checksum or the EndMark missing): the blocks cannot be cut out of it
    meta = {"flg": info["flg"], "content_size": info["content_size"], "block_max": info["block_max"],
            "end": info["end"], "overflow": int(info["end"] > f.size)}
    return meta, pay, word


class DeviceDecoder:
    """The GPU path of a rank's share of a frame: one batched decode of its compressed
    blocks (lz4mi_decompress_blocks, device pointers), stored blocks copied. The output
    buffer is kept for the next call of the same shape; `last_kernel_s` is the decode
    launch's time from HIP events on the stream."""

    def __init__(self, stream=None):
        self.stream = stream
        self.ws = None
        self.last_kernel_s = None

    def decode(self, rng, pay_rel, word, block_max, last_cap):
        """rng: this rank's frame bytes (device); pay_rel/word: its blocks' payload positions in
        rng and size words (int64 tensors). Returns (output, statuses): output = the blocks'
        decoded bytes concatenated in order; status 0 or the reference's error code. The output
        is a view of the decoder's workspace, valid until the next call."""
        import torch
        import lz4mi
        if rng.device.type != "cuda":          # a host frame: its bytes go to the current GPU once
            rng = rng.to("cuda")
            pay_rel, word = pay_rel.to("cuda"), word.to("cuda")
        dev = rng.device
        nb = pay_rel.numel()
        s = self.stream if self.stream is not None else torch.cuda.current_stream(dev)
        self.last_kernel_s = None
        cap = torch.full((nb,), block_max, dtype=torch.int64, device=dev)
        if nb:
            cap[-1] = last_cap
        slot_off = torch.arange(nb, dtype=torch.int64, device=dev) * block_max
        key = (nb, block_max, str(dev))
        if self.ws is None or self.ws[0] != key:
            self.ws = None
            self.ws = (key, torch.empty(max(1, nb * block_max), dtype=torch.uint8, device=dev))
        out = self.ws[1]
        status = torch.zeros(nb, dtype=torch.int32, device=dev)
        out_len = torch.zeros(nb, dtype=torch.int32, device=dev)
        # every block in one launch: the size words go in as they are (LZ4MI_FRAME_WORDS), so a stored
        # block (bit 31) is copied by its own wave beside the compressed ones (bufferDecompress.js:173-180;
        # larger than its slot: the reference's RangeError, status -8)
        if nb:
            w32 = torch.where(word >= 2 ** 31, word - 2 ** 32, word).to(torch.int32).contiguous()
            in_off = pay_rel.contiguous()
            c_cap = cap.to(torch.int32).contiguous()
            e0 = torch.cuda.Event(enable_timing=True)
            e1 = torch.cuda.Event(enable_timing=True)
            s.wait_stream(torch.cuda.current_stream(dev))   # the tensors above were made on the current stream
            with torch.cuda.stream(s):
                e0.record(s)
                lz4mi.decompress_blocks_dev(rng.data_ptr(), in_off.data_ptr(), w32.data_ptr(), out.data_ptr(),
                                            slot_off.data_ptr(), c_cap.data_ptr(), out_len.data_ptr(),
                                            status.data_ptr(), nb, s.cuda_stream, frame_words=True)
                e1.record(s)
            s.synchronize()
            self.last_kernel_s = e0.elapsed_time(e1) / 1e3
        if nb == 0:
            return torch.zeros(0, dtype=torch.uint8, device=dev), status
        # every block but the last filled its slot (the reference encoder's layout): the slots
        # are the output already; otherwise close the gaps
        lens = out_len.to(torch.int64)
        if bool((lens[:-1] == block_max).all()):
            return out[:(nb - 1) * block_max + int(lens[-1])], status
        ll = lens.tolist()
        res = torch.cat([out[b * block_max:b * block_max + ll[b]] for b in range(nb)])
        return res, status

    def verify(self, rng, pay_rel, word):
        """The block checksums (FLG 0x10) of this rank's run, in one launch (lz4mi_verify_blocks,
        LZ4MI_FRAME_WORDS): rng ends behind the last block's checksum. Returns the int32 status tensor,
        0 or ERR_BLOCK_CHECKSUM per block."""
        import torch
        import lz4mi
        if rng.device.type != "cuda":
            rng = rng.to("cuda")
            pay_rel, word = pay_rel.to("cuda"), word.to("cuda")
        dev = rng.device
        nb = pay_rel.numel()
        s = self.stream if self.stream is not None else torch.cuda.current_stream(dev)
        status = torch.zeros(nb, dtype=torch.int32, device=dev)
        if nb:
            w32 = torch.where(word >= 2 ** 31, word - 2 ** 32, word).to(torch.int32).contiguous()
            in_off = pay_rel.contiguous()
            s.wait_stream(torch.cuda.current_stream(dev))
            with torch.cuda.stream(s):
                lz4mi.verify_blocks_dev(rng.data_ptr(), rng.numel(), in_off.data_ptr(), w32.data_ptr(),
                                        status.data_ptr(), nb, s.cuda_stream, frame_words=True)
            s.synchronize()
        return status


def decompress_frame_sharded(frame, verify_checksum=True, group=None, root=0, decoder=None, gather=True,
                             timings=None, device=None, zero_copy=False, verify_blocks=False):
    """Decode an independent-block frame with its blocks shared out over the ranks.

    frame: the whole frame on root (1-D uint8 tensor; a CUDA tensor is indexed and scattered
    on the device), ignored on the other ranks. Root indexes the size words, every rank gets
    the index (broadcast) and a contiguous run of blocks of about equal decode cost
    (shard.balanced_runs) — the frame bytes of its run, sent
    point to point (RCCL over xGMI for CUDA tensors) — decodes them in one batch on its
    device, and the outputs are gathered to root in block order (`gather`), else each rank
    returns its own part. The content checksum (FLG 0x04) is verified on root's host from
    host-staged shards. Returns root's output (uint8 tensor), None on the other ranks (their
    part with gather=False). The frame's first error in block order is raised on every rank
    with the reference's message. `decoder` replaces DeviceDecoder (CPU tests); `timings`
    gets index / scatter / kernel / gather / checksum_wait phases, each closed by a barrier,
    plus kernel_device (the decoder's HIP-event time) and checksum_chain (the chain's own
    duration: it runs beside the gather, so checksum_wait is what it adds).
    `device`: where this rank's tensors live (default: frame's device on root, else the
    backend's: CUDA for nccl, host for gloo). With a caller's `decoder` the un-gathered result
    is a copy unless `zero_copy`: then it is a view of that decoder's workspace, overwritten
    by the decoder's next call of the same shape (bench.py keeps one decoder and opts in).
    verify_blocks: on a frame with block checksums (FLG 0x10) each rank checks its own run's
    (decoder.verify; a `decoder` without that method: ValueError) before it decodes; a mismatch on
    any rank raises ERR_BLOCK_CHECKSUM on every rank, before any block's own error is looked at."""
    import time
    import torch
    import lz4mi
    dist, multi, world, rank = _dist_ctx(group)
    if isinstance(frame, np.ndarray):
        frame = torch.from_numpy(np.ascontiguousarray(frame, dtype=np.uint8))
        if device is None and not multi:
            device = frame.device
    if device is not None:
        dev = torch.device(device)
    elif frame is not None:
        dev = frame.device
    else:   # the backend's device: RCCL moves CUDA tensors, gloo host ones
        nccl = multi and dist.get_backend(group) == "nccl"
        dev = torch.device("cuda", torch.cuda.current_device()) if nccl else torch.device("cpu")
    own_decoder = decoder is None
    decoder = decoder or DeviceDecoder()
    if verify_blocks and not hasattr(decoder, "verify"):
        raise ValueError("lz4mi: verify_blocks needs a decoder with a verify(rng, pay_rel, word) method")
    src = dist.get_global_rank(group, root) if (multi and group is not None) else root
    t0 = time.perf_counter()
    # ---- index on root, broadcast (a malformed frame raises on every rank, not only on root)
    status = 0
    meta = None
    if rank == root:
        try:
            meta, pay, word = frame_index(frame)
        except lz4mi.Lz4miError as e:
            status = e.status
    if meta is not None:
        hdr = torch.tensor([0, pay.numel(), meta["flg"], meta["content_size"], meta["block_max"], meta["end"],
                            meta["overflow"]], dtype=torch.int64, device=dev)
    else:
        hdr = torch.zeros(7, dtype=torch.int64, device=dev)
        hdr[0] = status
    if multi:
        dist.broadcast(hdr, src=src, group=group)
    status, nb, flg, csize, bmax, end, overflow = [int(x) for x in hdr.tolist()]
    if status:
        raise lz4mi.Lz4miError(status)
    if overflow:
        raise lz4mi.Lz4miError(lz4mi.ERR_MALFORMED)
    if not flg & 0x20:
        raise ValueError("lz4mi: dependent-block frames decode serially (LZ4.decompress)")
    if rank != root:
        pay = torch.zeros(nb, dtype=torch.int64, device=dev)
        word = torch.zeros(nb, dtype=torch.int64, device=dev)
    else:
        pay, word = pay.to(dev), word.to(dev)
    if multi and nb:
        dist.broadcast(pay, src=src, group=group)
        dist.broadcast(word, src=src, group=group)
    t0 = _phase(timings, "index", t0, dev, group)
    # ---- contiguous runs of blocks of about equal decode cost (shard.balanced_runs): rank r's
    # frame bytes [a_r, b_r)
    bsum = 4 if flg & 0x10 else 0
    size = word & 0x7FFFFFFF
    word_h = word.tolist()
    runs = shard.balanced_runs(word_h, bmax, world)
    pay_h, size_h = pay.tolist(), size.tolist()

    def span(lo, hi):
        if hi <= lo:
            return 0, 0
        return int(pay_h[lo]), int(pay_h[hi - 1] + size_h[hi - 1]) + bsum

    lo, hi = runs[rank]
    a, b = span(lo, hi)
    if multi:
        if rank == root:
            reqs = []
            for r in range(world):
                ra, rb = span(*runs[r])
                if r != root and rb > ra:
                    reqs.append(dist.isend(frame[ra:rb].contiguous(), dst=dist.get_global_rank(group, r)
                                           if group is not None else r, group=group))
            rng = frame[a:b]
            for q in reqs:
                q.wait()
        else:
            rng = torch.empty(max(1, b - a), dtype=torch.uint8, device=dev)[:b - a]
            if b > a:
                dist.recv(rng, src=src, group=group)
    else:
        rng = frame[a:b]
    t0 = _phase(timings, "scatter", t0, dev, group)
    # ---- decode this rank's run
    # each block decodes into block_max bytes (a block's output position depends on the sizes
    # before it, which only the decode gives); the content size is checked on the sum below
    last_cap = bmax
    if verify_blocks and flg & 0x10:
        vst = decoder.verify(rng, pay[lo:hi] - a, word[lo:hi])
        vbad = torch.tensor([int(bool((vst != 0).any()))], dtype=torch.int64, device=dev)
        if multi:
            dist.all_reduce(vbad, op=dist.ReduceOp.MAX, group=group)
        if int(vbad.item()):
            raise lz4mi.Lz4miError(lz4mi.ERR_BLOCK_CHECKSUM)
    out, status = decoder.decode(rng, pay[lo:hi] - a, word[lo:hi], bmax, last_cap)
    if timings is not None and getattr(decoder, "last_kernel_s", None) is not None:
        timings["kernel_device"] = timings.get("kernel_device", 0.0) + decoder.last_kernel_s
    bad = torch.nonzero(status != 0).flatten()
    first = torch.tensor([lo + int(bad[0]) if bad.numel() else nb, int(status[bad[0]]) if bad.numel() else 0],
                         dtype=torch.int64, device=dev)
    if multi:
        allf = [torch.zeros(2, dtype=torch.int64, device=dev) for _ in range(world)]
        dist.all_gather(allf, first, group=group)
        first = min(allf, key=lambda x: int(x[0]))
    total = torch.tensor([out.numel()], dtype=torch.int64, device=dev)
    if multi:
        dist.all_reduce(total, group=group)
    t0 = _phase(timings, "kernel", t0, dev, group)
    if int(first[0]) < nb:
        raise lz4mi.Lz4miError(int(first[1]))
    if csize > 0 and int(total.item()) != csize:
        raise lz4mi.Lz4miError(lz4mi.ERR_MALFORMED, "lz4mi: decoded size differs from the frame's content size")
    # ---- content checksum (bufferDecompress.js:213-217) from the decoded shards, its chain on
    # root's host beside the gather of the outputs to root (the chain reads each rank's shard
    # where it was decoded: host-staged, nothing crosses xGMI for it)
    ck = None
    if verify_checksum and flg & 0x04:
        ck = ContentChecksum(out.numel(), dev, group, root).start(out)
    got = None
    if gather and multi:
        try:
            got = shard.gather_records_to_root(out, root=root, group=group)
        except BaseException:
            if ck is not None:
                ck.abort()
            raise
        t0 = _phase(timings, "gather", t0, dev, group)
    if ck is not None:
        d = ck.finish()
        if timings is not None:
            timings["checksum_chain"] = timings.get("checksum_chain", 0.0) + ck.elapsed
        ok = torch.tensor([1], dtype=torch.int64, device=dev)
        if rank == root:
            want = int.from_bytes(frame[end:end + 4].cpu().numpy().tobytes(), "little")
            ok[0] = int(d == want)
        if multi:
            dist.broadcast(ok, src=src, group=group)
        t0 = _phase(timings, "checksum_wait", t0, dev, group)
        if not int(ok[0]):
            raise lz4mi.Lz4miError(lz4mi.ERR_CHECKSUM)
    if not gather or not multi:
        if rank != root and gather:
            return None
        caller_ws = decoder is not None and getattr(decoder, "ws", None) is not None and \
            out.numel() and out.data_ptr() >= decoder.ws[1].data_ptr() and \
            out.data_ptr() < decoder.ws[1].data_ptr() + decoder.ws[1].numel()
        return out.clone() if (caller_ws and not zero_copy and not own_decoder) else out
    return got


def _verify_content_checksum(frame, pos, out):
    """The frame's content checksum (at frame[pos:pos + 4]) against out (device), streamed to
    the host piece by piece (one serial XXH32 chain)."""
    import lz4mi
    want = int.from_bytes(frame[pos:pos + 4].cpu().numpy().tobytes(), "little")
    w = _ChecksumWorker()
    for p in range(0, out.numel(), CHECKSUM_PIECE):
        w.feed(out[p:p + CHECKSUM_PIECE].cpu().numpy())
    if w.digest() != want:
        raise lz4mi.Lz4miError(lz4mi.ERR_CHECKSUM)


def content_size_bound(frame_len):
    """The largest content size a frame of frame_len bytes is decoded for. A content size sizes the
    result before a block is looked at, and a damaged header can claim anything (the reference
    then fails in new Uint8Array, or allocates it). A compressed block of n bytes decodes to fewer
    than 255 * n bytes (a length byte adds at most 255, and costs a byte), a stored one to n, so
    255 * frame_len bounds what the frame's bytes can decode to; the reference's
    largest block (4 MiB) of slack on top, so that a frame cut inside its first record still gives
    the reference's result, content-size zeros. Above the bound both decompress_frame_host and
    decompress_frame_device raise ERR_RANGE and allocate nothing."""
    return 255 * int(frame_len) + 4194304


def _decode_measured(frame, head, js_exact, s, linked=False, verify_blocks=False):
    """The measured route of decompress_frame_device: index the frame's blocks on the device,
    measure every block's decoded size in one launch (lz4mi_decoded_sizes), lay the output out
    at the exact positions (exclusive prefix sum on the device) and decode all blocks in one
    batch. Returns (output, position of the content checksum), or None when the frame has to
    go to the host path so that its first error and message stay what they were.
    linked (the "linked" route, spec mode): the batch is one LZ4MI_LINKED call, so the blocks may
    depend on each other (a block's size does not depend on the bytes before it).
    verify_blocks: on a frame with block checksums (FLG 0x10) they are checked in one launch over the
    same index (lz4mi_verify_blocks), read with the size pass's statuses; a mismatch raises
    ERR_BLOCK_CHECKSUM here (the host route would only hash the frame again)."""
    import torch
    import lz4mi
    dev = frame.device
    n = frame.numel()
    bid = (int(head[5]) >> 4) & 7 if head.size > 5 else 7
    bmax = shard.BLOCK_MAX_SIZES.get(bid, 4194304)
    # the block lists are sized by walking the frame: first for the blocks it would have at a
    # compression ratio of 4, then, while the walk reports more blocks than listed, 16x as many
    # (never n / 4 entries up front: every record takes at least its 4-byte size word)
    most = n // 4 + 2
    cap = min(most, 4 * (n // bmax) + 64)
    with torch.cuda.stream(s):
        while True:
            pay = torch.empty(cap, dtype=torch.int64, device=dev)
            word = torch.empty(cap, dtype=torch.int32, device=dev)
            info = torch.zeros(8, dtype=torch.int64, device=dev)
            lz4mi.frame_index_dev(frame.data_ptr(), n, pay.data_ptr(), word.data_ptr(), cap, info.data_ptr(),
                                  s.cuda_stream)
            h = info.cpu().tolist()
            if h[0] == 0 and h[7] and h[3] >= cap and cap < most:
                cap = min(most, cap * 16)
                continue
            break
        nb = int(h[3])
        if h[0] or h[7] or nb == 0:
            return None
        size = int(h[2])
        if (int(h[1]) & 0x08) and size <= 0:
            return None
        pay, word = pay[:nb], word[:nb]
        sizes = torch.empty(nb, dtype=torch.int32, device=dev)
        mst = torch.empty(nb, dtype=torch.int32, device=dev)
        lz4mi.decoded_sizes_dev(frame.data_ptr(), pay.data_ptr(), word.data_ptr(), sizes.data_ptr(), mst.data_ptr(),
                                nb, s.cuda_stream, frame_words=True)
        sums = verify_blocks and int(h[1]) & 0x10
        if sums:
            vst = torch.empty(nb, dtype=torch.int32, device=dev)
            lz4mi.verify_blocks_dev(frame.data_ptr(), n, pay.data_ptr(), word.data_ptr(), vst.data_ptr(), nb,
                                    s.cuda_stream, frame_words=True)
        sz64 = sizes.to(torch.int64)
        ends = torch.cumsum(sz64, 0)
        comp_max = torch.where(word >= 0, sz64, torch.zeros_like(sz64)).max()   # stored blocks: bit 31 (negative)
        facts = [(mst != 0).any().to(torch.int64), comp_max, ends[-1]] + ([(vst != 0).any().to(torch.int64)] if sums else [])
        bad, comp_max, total, *vbad = torch.stack(facts).cpu().tolist()
        if vbad and vbad[0]:
            raise lz4mi.Lz4miError(lz4mi.ERR_BLOCK_CHECKSUM)
        # the host path reports these frames' errors: a block the walk fails, a compressed block that
        # decodes to more than the window path's block_max slot, a total other than the content size
        if bad or (size <= 0 and comp_max > bmax) or (size > 0 and total != size):
            return None
        out = torch.empty(max(1, total), dtype=torch.uint8, device=dev)
        out_off = (ends - sz64).contiguous()
        out_len = torch.zeros(nb, dtype=torch.int32, device=dev)
        status = torch.zeros(nb, dtype=torch.int32, device=dev)
        lz4mi.decompress_blocks_dev(frame.data_ptr(), pay.data_ptr(), word.data_ptr(), out.data_ptr(),
                                    out_off.data_ptr(), sizes.data_ptr(), out_len.data_ptr(), status.data_ptr(), nb,
                                    s.cuda_stream, frame_words=True, js_exact=js_exact, linked=linked)
        st = status.cpu().numpy()
        if ((st != 0) & (st != lz4mi.ERR_CROSS_BLOCK)).any() or (linked and (st != 0).any()):
            return None
        # blocks that read earlier blocks' output: every block before them is final now; each alone, in order
        # (the same bytes as the host path's 64 KiB window: a match offset has 16 bits, so it never reaches
        # further back than the window keeps, and before the frame's first byte both report DICT_OOB)
        for k in np.nonzero(st == lz4mi.ERR_CROSS_BLOCK)[0].tolist():
            lz4mi.decompress_blocks_dev(frame.data_ptr(), pay.data_ptr() + 8 * k, word.data_ptr() + 4 * k,
                                        out.data_ptr(), out_off.data_ptr() + 8 * k, sizes.data_ptr() + 4 * k,
                                        out_len.data_ptr() + 4 * k, status.data_ptr() + 4 * k, 1, s.cuda_stream,
                                        frame_words=True, js_exact=js_exact)
            if int(status[k].cpu()):
                return None
        if not bool((out_len == sizes).all()):
            return None
    return out[:total], int(h[5])


def decompress_frame_device(frame, js_exact=False, verify_checksum=True, stream=None, report=None, linked=False,
                            verify_blocks=False):
    """Decode a device-resident frame (1-D uint8 CUDA tensor) on its GPU. Three routes, in this
    order; `report` (a dict, optional) receives {"route": "layout" | "measured" | "host"}
    (with `linked`: "layout" | "linked" | "host"):
     - layout: the header and the block walk run on the device (lz4mi_frame_decompress), stored
       blocks are copied and the compressed ones decoded in one batch at the positions of the
       reference encoder's layout (content size present, every block but the last fills block_max);
     - measured: a frame of independent blocks (FLG 0x20) the layout walk declines (no content
       size, partial blocks): the blocks are indexed on the device, their decoded sizes measured
       in one launch (lz4mi_decoded_sizes), the output laid out at the exact positions and all
       blocks decoded in one batch; not taken for js_exact without a content size (the reference
       decodes such a frame behind a window, where a double-copy-tail rewrite at a block start
       lands elsewhere than in a contiguous result);
     - host: everything else (dependent blocks, the empty frame, frames with an error in a
       block), block by block through the host-buffer path, as bufferDecompress.js does.
    linked=True (ignored with js_exact): dependent blocks are decoded in one call too
    (LZ4MI_LINKED): the layout route passes the flag, and a frame the layout walk declines takes
    the route "linked" whatever FLG 0x20 says -- the measured route with one linked batch; the
    host route stays the last resort (the empty frame, frames with an error in a block).
    linked="exact" (with or without js_exact): the reference decoder's bytes with the layout route
    passing LZ4MI_LINKED_EXACT, one linked call for a dependent frame with a content size; a frame
    the layout walk declines takes the routes js_exact=True has without `linked`.
    verify_blocks: on a frame with block checksums (FLG 0x10) every route checks them before a block's
    own error is looked at -- layout: LZ4MI_VERIFY_BLOCKS; measured / linked: one lz4mi_verify_blocks
    launch over the block index; host: on the host -- and a mismatch raises ERR_BLOCK_CHECKSUM.
    The content checksum (FLG 0x04) is verified on the host, streamed piece by piece. Returns
    the content as a uint8 CUDA tensor: with a content size that many bytes, zeros behind what
    the blocks wrote (the reference's zero-initialised result). Raises lz4mi.Lz4miError with the
    reference's message for the frame's first error; a content size above content_size_bound
    is ERR_RANGE before anything is allocated for it."""
    import torch
    import lz4mi
    lx = isinstance(linked, str) and linked == "exact"
    if isinstance(linked, str) and not lx:
        raise ValueError("linked: True, False or 'exact'")
    if lx:
        js_exact = True                            # (every other route: the ones js_exact=True has)
    # the library binds one device per process: a frame on another device raises ERR_ARG here
    lz4mi.init(frame.device.index if frame.device.index is not None else torch.cuda.current_device())
    s = stream if stream is not None else torch.cuda.current_stream(frame.device)
    head = frame[:19].cpu().numpy()
    if head.size < 4 or int.from_bytes(head[:4].tobytes(), "little") != 0x184D2204:
        raise lz4mi.Lz4miError(lz4mi.ERR_MAGIC)
    # the content size as the reference reads it: the bytes the frame's end cuts off are 0
    h14 = np.zeros(14, dtype=np.uint8)
    h14[:min(14, head.size)] = head[:14]
    size = int.from_bytes(h14[6:14].tobytes(), "little") if head.size > 4 and head[4] & 0x08 else 0
    if report is None:
        report = {}
    if ((int(h14[4]) & 0xC0) >> 6) != 1:         # before the content size is looked at, as in the reference
        raise lz4mi.Lz4miError(lz4mi.ERR_VERSION)
    if size > content_size_bound(frame.numel()):
        # checked before the header's claim sizes any allocation: the host route refuses the frame
        # (ERR_RANGE; the reference's own failure there is the RangeError of new Uint8Array)
        report["route"] = "host"
        decompress_frame_host(frame.cpu().numpy(), js_exact=js_exact, verify_checksum=verify_checksum,
                              verify_blocks=verify_blocks)
        raise lz4mi.Lz4miError(lz4mi.ERR_RANGE)
    lk = bool(linked) and not js_exact
    try:
        if head.size < 14 and size:
            raise lz4mi.Lz4miError(lz4mi.ERR_ARG)   # the size field itself is cut: the host route's frame
        out = torch.empty(max(1, size), dtype=torch.uint8, device=frame.device)
        info = lz4mi.frame_decompress_dev(frame.data_ptr(), frame.numel(), out.data_ptr(), size, s.cuda_stream,
                                          js_exact=js_exact and not lx, linked="exact" if lx else lk,
                                          verify_blocks=verify_blocks)
    except lz4mi.Lz4miError as e:
        if e.status != lz4mi.ERR_ARG:
            raise
        out = None
        got = None
        report["route"] = "linked" if lk else "measured"   # (also what a block-checksum error there reports)
        if lk:
            got = _decode_measured(frame, head, False, s, linked=True, verify_blocks=verify_blocks)
        elif head.size > 4 and head[4] & 0x20 and not (js_exact and size == 0):
            got = _decode_measured(frame, head, js_exact, s, verify_blocks=verify_blocks)
        if got is None:
            report["route"] = "host"
            host = decompress_frame_host(frame.cpu().numpy(), js_exact=js_exact, verify_checksum=verify_checksum,
                                         verify_blocks=verify_blocks)
            return torch.from_numpy(host).to(frame.device)
        report["route"] = "linked" if lk else "measured"
        res, pos = got
        if verify_checksum and head[4] & 0x04:
            s.synchronize()
            _verify_content_checksum(frame, pos, res)
        return res
    report["route"] = "layout"
    if info["status"]:
        raise lz4mi.Lz4miError(info["status"])
    # the reference's result is its zero-initialised content-size array, whatever the blocks wrote
    # (only the frame's last block can fall short on this route): zeros behind it, all of it checksummed
    out = out[:size]
    if info["written"] < size:
        with torch.cuda.stream(s):
            out[info["written"]:].zero_()
        s.synchronize()
    if verify_checksum and info["flg"] & 0x04:
        _verify_content_checksum(frame, info["checksum_pos"], out)
    return out


def decompress_frame_host(frame, js_exact=False, verify_checksum=True, verify_blocks=False):
    """A frame in host memory decoded block by block through the host-buffer C-ABI path,
    with the reference's two layouts (bufferDecompress.js:97-186): with a content size every
    block is decoded straight into the result at its position (back-references into earlier
    blocks resolve there); without one, each block is decoded into one 4 MiB workspace kept for
    the whole frame, the last 64 KiB of output (the reference's rolling window) as its dictionary. With a
    content size the result is the reference's: content-size bytes, zeros behind what the blocks
    wrote, and the content checksum is taken over all of them. Returns the content (numpy uint8).

    A block whose declared size runs past the frame's end is decoded with that size, as the
    reference does (decompressBlock gets the size word, bytes past the array read as 0): on the
    host decoder (lz4mi_host_decompress_block over the whole frame), so nothing of the declared
    size is allocated. So is a block whose last offset or length field reaches behind its own end
    (a size word that is off by a few bytes): the reference reads the frame's bytes there.

    verify_blocks: on a frame with block checksums (FLG 0x10) every record is checked on the host
    (lz4mi_host_verify_blocks) before the first block is decoded; a mismatch, or a record the frame's
    end cuts, raises ERR_BLOCK_CHECKSUM -- no device is touched."""
    import lz4mi
    f = np.ascontiguousarray(frame, dtype=np.uint8)
    try:
        info, blocks = shard.frame_blocks(f)
    except ValueError:
        raise lz4mi.Lz4miError(lz4mi.ERR_MAGIC)
    if ((info["flg"] & 0xC0) >> 6) != 1:
        raise lz4mi.Lz4miError(lz4mi.ERR_VERSION)
    size = info["content_size"]
    if size > content_size_bound(f.size):
        raise lz4mi.Lz4miError(lz4mi.ERR_RANGE)
    if verify_blocks and info["flg"] & 0x10 and blocks:
        if lz4mi.host_verify_blocks(f, [p for p, _, _ in blocks], [n for _, n, _ in blocks]).any():
            raise lz4mi.Lz4miError(lz4mi.ERR_BLOCK_CHECKSUM)

    def block(p, n, out, pos, window=None):
        """decompressBlock(data, p, n, out, pos, window): bytes written."""
        if p + n >= 2 ** 31:      # inEnd = (inputOffset + inputSize) | 0 is negative: nothing is decoded
            return 0
        # the batch decoder's block ends at n (zeros behind it); the reference's reads on in the frame
        if p + n <= f.size and lz4mi.host_block_read_end(f, p, n) <= p + n:
            return lz4mi.decompress_raw(f, p, n, out, pos, dictionary=window, js_exact=js_exact)
        return lz4mi.host_decompress_raw(f, p, n, out, pos, dictionary=window, spec=not js_exact)

    if size > 0:
        out = np.zeros(size, dtype=np.uint8)
        pos = 0
        for p, n, stored in blocks:
            if stored:
                seg = f[p:p + n]              # subarray() clips at the frame's end
                if pos + seg.size > size:
                    raise lz4mi.Lz4miError(lz4mi.ERR_RANGE)
                out[pos:pos + seg.size] = seg
                pos += n
            else:
                pos += block(p, n, out, pos)
    else:
        # as the reference (:157-186): every block is decoded at the start of one 4 MiB workspace (whatever
        # BD says, :41, :127), over what the block before it left there, the window passed as its dictionary
        parts, window = [], np.zeros(0, dtype=np.uint8)
        ws = np.zeros(4194304, dtype=np.uint8)
        for p, n, stored in blocks:
            if stored:
                piece = f[p:p + n].copy()
            else:
                piece = ws[:block(p, n, ws, 0, window if window.size else None)].copy()
            parts.append(piece)
            window = np.concatenate([window, piece])[-65536:]
        out = np.concatenate(parts) if parts else np.zeros(0, dtype=np.uint8)
    if verify_checksum and info["checksum"]:
        end = info["end"]
        want = int.from_bytes(f[end:end + 4].tobytes(), "little")
        if lz4mi.XXHash32(0, len64=True).update(out).digest() != want:
            raise lz4mi.Lz4miError(lz4mi.ERR_CHECKSUM)
    return out


def decompress_frames_device(frames, js_exact=False, verify_checksum=True, measure=False, stream=None, report=None,
                             return_errors=False, offsets=None, lengths=None, cap_blocks=None, chains=False,
                             verify_blocks=False):
    """Decode a batch of device-resident frames with one index call, one output allocation and one decode
    call (lz4mi_frames_index / lz4mi_frames_decompress): the frames' size words are walked in parallel, one
    lane per frame, the blocks of all frames decoded by one batch launch, and with verify_checksum the
    content checksums (FLG 0x04) hashed on the device, one chain per frame, all in one launch.

    frames: a list of 1-D uint8 CUDA tensors, or one such tensor holding frame f at
    frames[offsets[f] : offsets[f] + lengths[f]] (any alignment). The list form concatenates the frames first,
    a device copy of all input that doubles its memory for the call: frames that already lie in one tensor
    should be passed with offsets and lengths. measure: LZ4MI_FRAMES_MEASURE, every
    frame's block sizes are measured (frames with a content size and partial blocks in the middle).
    chains: LZ4MI_FRAMES_CHAINS, a frame whose blocks read the blocks before them (what the reference writes
    by default for anything longer than one block; with js_exact also an independent frame whose tail rewrite
    reads below a block) is decoded in the same call, one wave per frame in block order, instead of being
    declined: right for many frames, slow for a few long ones (one wave walks the whole frame).
    verify_blocks: the block checksums (FLG 0x10) of all frames are checked on the device, one quad of lanes per
    record (lz4mi_frames_verify_blocks), enqueued behind each index call and in front of its read-back, so no
    synchronisation is added and the statuses come back with finfo. A frame with a failing record gets no room
    in the output, is not decoded and is Lz4miError(ERR_BLOCK_CHECKSUM) with route "batch" -- before any block's
    own error and the content checksum, as decompress_frame_device(verify_blocks=True) reports it; a frame the
    batch declines goes to that call with verify_blocks. report["bad_block"][f] is then the index, within
    the frame, of the first failing record of a frame whose blocks were listed, else None.
    Two host synchronisations: finfo and totals read back after the index (a third when cap_blocks -- the
    guess of _decode_measured, or the caller's -- was too small and the index runs again with the exact
    need), and finfo after the decode. A frame the batch declines (finfo[f][7], include/lz4mi.h
    LZ4MI_FRAMES_DECLINE_*: dependent blocks, the empty frame, cut frames, unsized frames with js_exact, ...)
    or whose content size is above content_size_bound goes through decompress_frame_device alone, so the
    result is always complete and what that call gives per frame.
    report (a dict, optional) receives routes (per frame "batch" or that call's route), declined (per frame
    the decline code) and index_calls. Returns the list of result tensors: for batch frames views of the one
    allocation, at 16-byte-aligned offsets. The first failing frame raises lz4mi.Lz4miError with
    .frame_index; with return_errors the error objects stand in the list instead."""
    import torch
    import lz4mi
    if offsets is None:
        frames = list(frames)
        lens = [int(t.numel()) for t in frames]
        offs = [0] * len(lens)
        for k in range(1, len(lens)):
            offs[k] = offs[k - 1] + lens[k - 1]
        dev = frames[0].device if frames else torch.device("cuda", torch.cuda.current_device())
    else:
        offs, lens = [int(x) for x in offsets], [int(x) for x in lengths]
        dev = frames.device
    nf = len(lens)
    if report is None:
        report = {}
    report.update(routes=[None] * nf, declined=[0] * nf, index_calls=0)
    if verify_blocks:
        report["bad_block"] = [None] * nf
    if nf == 0:
        return []
    lz4mi.init(dev.index if dev.index is not None else torch.cuda.current_device())
    s = stream if stream is not None else torch.cuda.current_stream(dev)
    with torch.cuda.stream(s):
        arena = torch.cat(frames) if offsets is None else frames
        if arena.numel() == 0:
            arena = torch.zeros(1, dtype=torch.uint8, device=dev)
        span = torch.tensor([offs, lens], dtype=torch.int64, device=dev)
        # the block lists are sized as _decode_measured sizes them: for a compression ratio of 4 at the
        # smallest block size; the index reports the exact need when that was too small
        nbytes = sum(lens)
        cap = cap_blocks if cap_blocks is not None else min(nbytes // 4 + 2, 4 * (nbytes // 65536) + 2 * nf + 64)
        while True:
            cap = max(1, int(cap))
            blk_in_off = torch.empty(cap, dtype=torch.int64, device=dev)
            blk32 = torch.empty((3, cap), dtype=torch.int32, device=dev)   # word, frame, size
            # finfo, then totals; with verify_blocks the int32 statuses of the cap list entries behind them, so
            # that one copy brings everything back
            fin = torch.zeros(8 * nf + 4 + ((cap + 1) // 2 if verify_blocks else 0), dtype=torch.int64, device=dev)
            lz4mi.frames_index_dev(arena.data_ptr(), span[0].data_ptr(), span[1].data_ptr(), nf, blk_in_off.data_ptr(),
                                   blk32[0].data_ptr(), blk32[1].data_ptr(), blk32[2].data_ptr(), cap, fin.data_ptr(),
                                   fin.data_ptr() + 64 * nf, s.cuda_stream, measure=measure, js_exact=js_exact)
            report["index_calls"] += 1
            if verify_blocks:
                lz4mi.frames_verify_blocks_dev(arena.data_ptr(), span[0].data_ptr(), span[1].data_ptr(), nf,
                                               blk_in_off.data_ptr(), blk32[0].data_ptr(), blk32[1].data_ptr(), cap,
                                               fin.data_ptr(), fin.data_ptr() + 8 * (8 * nf + 4), s.cuda_stream)
            h = fin.cpu().numpy()
            need = int(h[8 * nf])
            if need <= cap or report["index_calls"] > 1:
                break
            cap = need
        info = h[:8 * nf].reshape(nf, 8)
        listed = int(h[8 * nf + 1])     # the decode launch and its scratch take the blocks listed, not the guess
        if verify_blocks:
            blk_status = h[8 * nf + 4:].view(np.int32)
            for f in range(nf):
                if info[f, 0] == lz4mi.ERR_BLOCK_CHECKSUM:
                    first = int(info[f, 4])
                    report["bad_block"][f] = int(np.flatnonzero(blk_status[first:first + int(info[f, 6])])[0])
        # one allocation, the frames the call decodes at 16-byte-aligned offsets; a content size above the
        # bound sizes nothing: that frame gets no room, which declines it
        out_off, out_cap, at = [0] * nf, [0] * nf, 0
        for f in range(nf):
            total = int(info[f, 3])
            size = int(info[f, 2]) & 0xFFFFFFFFFFFFFFFF
            if info[f, 0] or info[f, 7] or size > content_size_bound(lens[f]):
                continue
            out_off[f], out_cap[f] = at, total
            at += (total + 15) & ~15
        out = torch.empty(max(1, at), dtype=torch.uint8, device=dev)
        slots = torch.tensor([out_off, out_cap], dtype=torch.int64, device=dev)
        lz4mi.frames_decompress_dev(arena.data_ptr(), blk_in_off.data_ptr(), blk32[0].data_ptr(), blk32[1].data_ptr(),
                                    blk32[2].data_ptr(), listed, fin.data_ptr(), nf, out.data_ptr(), slots[0].data_ptr(),
                                    slots[1].data_ptr(), s.cuda_stream, js_exact=js_exact,
                                    verify_content=verify_checksum, chains=chains)
        done = fin[:8 * nf].cpu().numpy().reshape(nf, 8)
    res = [None] * nf
    for f in range(nf):
        err = None
        if done[f, 7]:
            report["declined"][f] = int(done[f, 7])
            one = arena[offs[f]:offs[f] + lens[f]]
            r = {}
            try:
                res[f] = decompress_frame_device(one, js_exact=js_exact, verify_checksum=verify_checksum, stream=stream,
                                                 report=r, verify_blocks=verify_blocks)
            except lz4mi.Lz4miError as e:
                err = e
            report["routes"][f] = r.get("route", "host")
        else:
            report["routes"][f] = "batch"
            if done[f, 0]:
                err = lz4mi.Lz4miError(int(done[f, 0]))
            else:
                res[f] = out[out_off[f]:out_off[f] + out_cap[f]]
        if err is not None:
            err.frame_index = f
            if not return_errors:
                raise err
            res[f] = err
    return res


def _frame_alone(one, block_size, independent, content_checksum, add_content_size, block_checksum, stream):
    """One frame of a device-resident buffer outside the batch (what compress_frames_device does with a frame
    the batch declines) -> (frame, route). A dependent frame of more than one block is one chain
    (lz4mi.compress_chain over the host copy, bufferCompress.js:182-236), route "chain"; anything else the
    per-frame device path (DeviceCodec), route "codec". The content checksum is hashed on the host."""
    import torch
    import lz4mi
    n = one.numel()
    dev = one.device
    hdr = header(block_size, independent, content_checksum, n if add_content_size else None, None, block_checksum)
    host = None
    if not independent and n > block_size:
        route = "chain"
        host = one.cpu().numpy()
        parts = []
        for k, comp in enumerate(lz4mi.compress_chain(host, 0, n, block_size, np.zeros(16384, dtype=np.int32))):
            raw = host[k * block_size:(k + 1) * block_size]
            pay, word = (comp, comp.size) if 0 < comp.size < raw.size else (raw, raw.size | 0x80000000)
            parts += [np.array([word], dtype="<u4").view(np.uint8), pay]
            if block_checksum:
                parts.append(np.array([lz4mi.xxh32(pay, standard=True)], dtype="<u4").view(np.uint8))
        body = torch.from_numpy(np.concatenate(parts)).to(dev)
    else:
        route = "codec"
        body = DeviceCodec(stream).records(one, block_size, block_checksum)
    tail = b"\x00\x00\x00\x00"
    if content_checksum:
        h = lz4mi.XXHash32(0, len64=True)
        if host is not None:
            h.update(host)
        else:
            for p in range(0, n, CHECKSUM_PIECE):
                h.update(one[p:p + CHECKSUM_PIECE].cpu().numpy())
        tail += int(h.digest()).to_bytes(4, "little")
    out = torch.empty(len(hdr) + body.numel() + len(tail), dtype=torch.uint8, device=dev)
    out[:len(hdr)] = torch.frombuffer(bytearray(hdr), dtype=torch.uint8).to(dev)
    out[len(hdr):len(hdr) + body.numel()] = body
    out[len(hdr) + body.numel():] = torch.frombuffer(bytearray(tail), dtype=torch.uint8).to(dev)
    return out, route


def compress_frames_device(buffers, block_size=4194304, independent=True, content_checksum=False,
                           add_content_size=True, block_checksum=False, stream=None, report=None, offsets=None,
                           lengths=None, chains=False):
    """Compress a batch of device-resident buffers into one LZ4 frame each with one plan call, one scratch and one
    output allocation and one compress call (lz4mi_frames_plan / lz4mi_frames_compress, packed): frame f is
    LZ4.compress(buffer f, null, block_size, independent, content_checksum, add_content_size) byte for byte
    (block_checksum adds FLG 0x10 and the records' checksums, which the reference never writes). The blocks of all
    buffers go into the batch encoder, the frames are laid out and written on the device, and the checksums are
    hashed there, one chain per block or frame, all in one launch each.

    buffers: a list of 1-D uint8 CUDA tensors, or one such tensor holding buffer f at
    buffers[offsets[f] : offsets[f] + lengths[f]] (any alignment). The list form concatenates the buffers first,
    a device copy of all input: buffers that already lie in one tensor should be passed with offsets and lengths.
    Two host synchronisations: finfo and totals read back after the plan, finfo after the compress call.
    A frame the batch declines (finfo[f][7]) is completed alone, so the result is always complete: a dependent
    frame of more than one block by one chain (lz4mi.compress_chain), anything else by DeviceCodec, each with
    header(). chains=True (with independent=False; LZ4MI_FRAMES_CHAINS) keeps those dependent frames in the batch
    instead: one chain per frame, all of them in the one compress call, route "batch". report (a dict, optional) receives routes (per frame "batch", "chain" or "codec") and declined (per
    frame the decline code). Returns the list of frames (uint8 CUDA tensors): batch frames are views of the one
    allocation, back to back."""
    import torch
    import lz4mi
    if offsets is None:
        buffers = list(buffers)
        lens = [int(t.numel()) for t in buffers]
        offs = [0] * len(lens)
        for k in range(1, len(lens)):
            offs[k] = offs[k - 1] + lens[k - 1]
        dev = buffers[0].device if buffers else torch.device("cuda", torch.cuda.current_device())
    else:
        offs, lens = [int(x) for x in offsets], [int(x) for x in lengths]
        dev = buffers.device
    nf = len(lens)
    if report is None:
        report = {}
    report.update(routes=[None] * nf, declined=[0] * nf)
    if nf == 0:
        return []
    bs = shard.BLOCK_MAX_SIZES[block_id(block_size)]
    flags = lz4mi.frames_enc_flags(independent, content_checksum, add_content_size, block_checksum, packed=True,
                                   chains=chains)
    lz4mi.init(dev.index if dev.index is not None else torch.cuda.current_device())
    s = stream if stream is not None else torch.cuda.current_stream(dev)
    with torch.cuda.stream(s):
        arena = torch.cat(buffers) if offsets is None else buffers
        if arena.numel() == 0:
            arena = torch.zeros(1, dtype=torch.uint8, device=dev)
        span = torch.tensor([offs, lens], dtype=torch.int64, device=dev)
        cap = max(1, sum(-(-n // bs) for n in lens))     # the lengths are the host's: the exact block count
        blk64 = torch.empty((2, cap), dtype=torch.int64, device=dev)   # in_off, work_off
        blk32 = torch.empty((2, cap), dtype=torch.int32, device=dev)   # len, frame
        fin = torch.zeros(8 * nf + 4, dtype=torch.int64, device=dev)   # finfo, then totals
        lz4mi.frames_plan_dev(span[0].data_ptr(), span[1].data_ptr(), nf, bs, blk64[0].data_ptr(), blk32[0].data_ptr(),
                              blk32[1].data_ptr(), blk64[1].data_ptr(), cap, fin.data_ptr(), fin.data_ptr() + 64 * nf,
                              s.cuda_stream, flags=flags)
        totals = fin[8 * nf:].cpu().tolist()
        listed, out_total, work_bytes = int(totals[1]), int(totals[2]), int(totals[3])
        work = torch.empty(max(16, work_bytes), dtype=torch.uint8, device=dev)
        out = torch.empty(max(1, out_total), dtype=torch.uint8, device=dev)
        lz4mi.frames_compress_dev(arena.data_ptr(), blk64[0].data_ptr(), blk32[0].data_ptr(), blk32[1].data_ptr(),
                                  blk64[1].data_ptr(), listed, fin.data_ptr(), nf, work.data_ptr(), work.numel(),
                                  out.data_ptr(), out_total, None, None, s.cuda_stream, flags=flags)
        done = fin[:8 * nf].cpu().numpy().reshape(nf, 8)
    res = [None] * nf
    for f in range(nf):
        if done[f, 7]:
            report["declined"][f] = int(done[f, 7])
            res[f], report["routes"][f] = _frame_alone(arena[offs[f]:offs[f] + lens[f]], bs, independent,
                                                       content_checksum, add_content_size, block_checksum, stream)
        else:
            report["routes"][f] = "batch"
            res[f] = out[int(done[f, 5]):int(done[f, 5] + done[f, 3])]
    return res
