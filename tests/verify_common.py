"""Shared by tests/test_verify_cpu.py and tests/test_gpu_verify.py: frame block checksums
(FLG 0x10) checked by lz4mi_verify_blocks / lz4mi_host_verify_blocks and by the frame routes.

Two inputs, both checked against the CPU oracle only:
  - a sweep of records (payload + LE32 of oracle.xxh32_std(payload)) at the lengths around the
    XXH32 kernel's load pipeline and at every start residue mod 4, inside one array whose other
    bytes are all 0x00 or all 0xFF;
  - one five-block frame (four compressed blocks, one stored) in every combination of block
    independence and content size, and the ways it is damaged.
"""
import functools

import numpy as np

import oracle as O
from lz4mi import shard

ERR_BLOCK_CHECKSUM = -10
BS = 65536
# tests/test_gpu_parity.py test_xxh32_batch_pipeline_edges' lengths, and the short tails
PIPELINE_LENS = (0, 15, 16, 4095, 4096, 4097, 4111, 4112, 4128, 6144 + 7, 8191, 8192, 8193, 12288 + 200,
                 (1 << 16) - 1, 1 << 16, (1 << 16) + 17)
LENS = PIPELINE_LENS + (1, 3, 4, 17, 31, 32, 33)
FILLS = (0x00, 0xFF)


def le32(x):
    return np.array([x & 0xFFFFFFFF], dtype="<u4").view(np.uint8)


def record(payload):
    return np.concatenate([np.asarray(payload, dtype=np.uint8), le32(O.xxh32_std(payload))])


@functools.lru_cache(maxsize=None)
def _sweep_layout():
    """(payloads, offsets): every length at the start residues 0, 1, 2, 3 (mod 4), 5 to 8 bytes of
    the surroundings between two records and 64 bytes of them at either end."""
    src = O.generate("random", 11, (1 << 16) + 64)
    pays, offs, at = [], [], 64
    for k, n in enumerate(LENS):
        for r in range(4):
            at += 5
            at += (r - at) % 4
            pays.append(src[(k + r) % 5:(k + r) % 5 + n])
            offs.append(at)
            at += n + 4
    return tuple(pays), tuple(offs), at + 64


def sweep(fill):
    """-> (arena, offsets uint64, lengths uint32): the records of _sweep_layout in `fill`."""
    pays, offs, size = _sweep_layout()
    arena = np.full(size, fill, dtype=np.uint8)
    for p, o in zip(pays, offs):
        arena[o:o + p.size + 4] = record(p)
    return arena, np.array(offs, dtype=np.uint64), np.array([p.size for p in pays], dtype=np.uint32)


def damage_sites(off, n):
    """The positions whose bit is flipped in turn: the payload's first, middle and last byte (an
    empty payload has none) and each of the four checksum bytes."""
    pay = sorted({off, off + n // 2, off + n - 1}) if n else []
    return [int(p) for p in pay] + [int(off + n + k) for k in range(4)]


def expected(arena, offs, lens, total=None):
    """The statuses from the oracle hash alone."""
    total = arena.size if total is None else total
    out = []
    for o, n in zip(offs, lens):
        o, n = int(o), int(n) & 0x7FFFFFFF
        ok = o + n + 4 <= total and int(arena[o + n:o + n + 4].view("<u4")[0]) == O.xxh32_std(arena[o:o + n])
        out.append(0 if ok else ERR_BLOCK_CHECKSUM)
    return np.array(out, dtype=np.int32)


# ------------------------------------------------------------------------------------- the frame
@functools.lru_cache(maxsize=None)
def data():
    return np.concatenate([O.generate("tiles216", 3, 2 * BS), O.generate("random", 4, BS),
                           O.generate("text", 5, BS + 1000)])


PAYLOADS = {True: (17677, 17679, 65536, 40661, 713), False: (17677, 5948, 65536, 40661, 603)}
RESIDUES = {True: (3, 0, 3, 3, 0), False: (3, 0, 0, 0, 1)}


@functools.lru_cache(maxsize=None)
def frame(indep, sized, content_checksum=True, block_checksum=True):
    """The frame (read-only) of data(): five blocks, block 2 stored. With block checksums its shape
    is asserted, so that a change in the oracle cannot hollow the tests out."""
    f = O.compress_frame(data(), None, BS, indep, content_checksum, sized, block_checksum=block_checksum)
    info, blocks = shard.frame_blocks(f)
    assert [st for _, _, st in blocks] == [False, False, True, False, False]
    assert bool(info["flg"] & 0x10) == block_checksum and bool(info["flg"] & 0x20) == indep
    assert (info["content_size"] == data().size) if sized else info["content_size"] == 0
    if block_checksum:
        assert tuple(n for _, n, _ in blocks) == PAYLOADS[indep]
        assert tuple(p % 4 for p, _, _ in blocks) == RESIDUES[indep]
        for p, n, _ in blocks:
            assert int(f[p + n:p + n + 4].view("<u4")[0]) == O.xxh32_std(f[p:p + n])
    f.setflags(write=False)
    return f


@functools.lru_cache(maxsize=None)
def decoded(indep, reference):
    """What the sized frame decodes to: data(), or (`reference`) the reference decoder's bytes from the
    oracle -- its double-copy-tail rewrite changes bytes of the text blocks."""
    st, out = O.decompress_frame(frame(indep, True), verify_checksum=False, js_compat=reference)
    assert st == 0 and out.size == data().size and (reference or np.array_equal(out, data()))
    return out


def blocks_of(f):
    return shard.frame_blocks(f)[1]


DAMAGES = ("payload0", "stored", "last_sum", "cut")


def damaged(f, how):
    """A damaged copy of a frame with block checksums: a flipped payload byte in block 0
    (`payload0`) or in the stored block (`stored`), a flipped checksum byte of the last block
    (`last_sum`), the frame cut one byte into its last checksum (`cut`); `decode0`: block 0's
    first three bytes zeroed, so that its decode fails too (a token 0x00 with offset 0)."""
    b = blocks_of(f)
    g = f.copy()
    if how == "payload0":
        g[b[0][0] + b[0][1] // 2] ^= 0x01
    elif how == "stored":
        g[b[2][0] + 1000] ^= 0x80
    elif how == "last_sum":
        g[b[4][0] + b[4][1] + 2] ^= 0x10
    elif how == "cut":
        g = g[:b[4][0] + b[4][1] + 1].copy()
    elif how == "decode0":
        g[b[0][0]:b[0][0] + 3] = 0
        assert O.decompress_block(g[b[0][0]:b[0][0] + b[0][1]], BS)[0] != 0
    else:
        raise ValueError(how)
    return g


class HostDecoder:
    """decompress_frame_sharded's decoder on the host: the oracle decodes each block, and verify()
    is lz4mi_host_verify_blocks over the rank's run."""

    def decode(self, rng, pay_rel, word, block_max, last_cap):
        import torch
        f = rng.numpy()
        outs, status = [], []
        nb = pay_rel.numel()
        for b in range(nb):
            p, w = int(pay_rel[b]), int(word[b])
            n, cap = w & 0x7FFFFFFF, (block_max if b + 1 < nb else last_cap)
            if w & 0x80000000:
                outs.append(f[p:p + n])
                status.append(0)
            else:
                st, m, out = O.decompress_block(f[p:p + n], cap)
                outs.append(out[:m] if st == 0 else np.zeros(0, dtype=np.uint8))
                status.append(st)
        res = np.concatenate(outs) if outs else np.zeros(0, dtype=np.uint8)
        return torch.from_numpy(res), torch.tensor(status, dtype=torch.int32)

    def verify(self, rng, pay_rel, word):
        import torch
        import lz4mi
        return torch.from_numpy(lz4mi.host_verify_blocks(rng.numpy(), pay_rel.numpy(), word.numpy(), frame_words=True))


class NoVerifyDecoder:
    def decode(self, rng, pay_rel, word, block_max, last_cap):
        return HostDecoder().decode(rng, pay_rel, word, block_max, last_cap)
