"""Shared by test_damaged_frames_cpu.py and test_gpu_damaged_frames.py: the recorded outcomes of
the reference's decompressBuffer on damaged frames (tests/golden/damaged_frames.json, written by
tools/golden/gen_damaged_frames.mjs), the frames rebuilt from their recipes, and a plain byte-wise
restatement of the reference's frame walk (bufferDecompress.js:56-92 header, :133-192 block loop)."""
import functools
import json
import os

import numpy as np

import oracle as O

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# the reference's messages -> the status both the oracle and lz4mi report for them
STATUS_OF_MESSAGE = {
    "LZ4: Output Buffer Too Small": -1, "LZ4: Malformed Input": -2, "LZ4: Invalid Offset 0": -3,
    "LZ4: Dictionary Offset Out of Bounds": -4, "LZ4: Invalid Magic Number": -5, "LZ4: Content Checksum Error": -7,
    # result.set(data.subarray(...), resultPos) of a stored block past the result (bufferDecompress.js:148)
    "Source is too large": -8, "offset is out of bounds": -8,
}
ALLOC_PREFIX = "Invalid typed array length"     # new Uint8Array(expectedOutputSize), :107 (the 2^48 case only)
BMAX = {4: 65536, 5: 262144, 6: 1048576, 7: 4194304}


@functools.lru_cache(maxsize=None)
def fixture():
    with open(os.path.join(GOLDEN, "damaged_frames.json")) as f:
        return json.load(f)


def base_names():
    return [b["name"] for b in fixture()["bases"]]


@functools.lru_cache(maxsize=None)
def base(name):
    """A base frame's entry, its cases written out: {"k": kind, "p": pieces, "v" / "n": the outcome with
    verifyChecksum true / false, or "u": 1 for an unspecified case}. In the file a case is
    [kind, recipe, v, n], kind and outcomes being indices into the base's lists (-1: unspecified) and
    the recipe a length (the frame cut there), [pos, hex] (bytes written over base[pos..]) or the pieces."""
    b = dict(next(b for b in fixture()["bases"] if b["name"] == name))
    n = b["frame_len"]
    cases = []
    for kind, r, v, w in b["cases"]:
        if isinstance(r, int):
            p = [[0, r]]
        elif isinstance(r[0], int):
            p = [[0, r[0]], r[1], [r[0] + len(r[1]) // 2, n]]
        else:
            p = r
        c = {"k": b["kinds"][kind], "p": p}
        if v < 0:
            c["u"] = 1
        else:
            c["v"], c["n"] = b["outcomes"][v], b["outcomes"][w]
        cases.append(c)
    b["cases"] = cases
    return b


@functools.lru_cache(maxsize=None)
def base_content(name):
    parts = fixture()["contents"][base(name)["content"]]
    return np.concatenate([O.generate(k, s, n) for k, s, n in parts]) if parts else np.zeros(0, dtype=np.uint8)


@functools.lru_cache(maxsize=None)
def base_frame(name):
    """The undamaged frame, from the oracle's encoder; its length and digest are the generator's."""
    b = base(name)
    f = O.compress_frame(base_content(name), None, fixture()["block"], b["indep"], b["csum"], b["size"],
                         block_checksum=b["bsum"])
    assert f.size == b["frame_len"] and "%08x" % O.xxh32(f) == b["frame_xxh"], name
    f.setflags(write=False)
    return f


def build(f, pieces):
    """A case's frame: [a, b] = base[a:b], a string = hex bytes."""
    parts = [np.frombuffer(bytes.fromhex(p), dtype=np.uint8) if isinstance(p, str) else f[p[0]:p[1]] for p in pieces]
    return np.concatenate(parts) if parts else np.zeros(0, dtype=np.uint8)


def cases(name, specified=True):
    """[(index, case, frame)] of a base frame; the unspecified cases are left out unless asked for."""
    f = base_frame(name)
    return [(k, c, build(f, c["p"])) for k, c in enumerate(base(name)["cases"]) if not (specified and c.get("u"))]


def expected_status(outcome):
    """The status of a recorded outcome [1, length, xxh32] or [0, error class, message]."""
    if outcome[0]:
        return 0
    name, msg = outcome[1], outcome[2]
    if msg.startswith("LZ4: Unsupported Version"):
        return -6
    if name == "RangeError" and msg.startswith(ALLOC_PREFIX):
        return "alloc"
    assert (name == "RangeError") == (STATUS_OF_MESSAGE[msg] == -8), outcome
    return STATUS_OF_MESSAGE[msg]


def walk(f):
    """The reference's walk of a frame, byte by byte, a read past the end being 0 as `undefined | 0`
    is; no guard where the reference has none. Returns the eight info words of the frame kernels
    (status, FLG, content size, blocks, 0, position after the loop, block_max, overflow) and the
    blocks [(payload position, size word)]."""
    n = len(f)
    g = lambda p: int(f[p]) if p < n else 0
    u32 = lambda p: g(p) | g(p + 1) << 8 | g(p + 2) << 16 | g(p + 3) << 24
    if n < 4 or u32(0) != 0x184D2204:
        return [-5, 0, 0, 0, 0, 0, 4194304, 0], []
    flg = g(4)
    if (flg & 0xC0) >> 6 != 1:
        return [-6, flg, 0, 0, 0, 0, 4194304, 0], []
    bmax = BMAX.get((g(5) >> 4) & 7, 4194304)
    pos = 6
    size = 0
    if flg & 0x08:
        size = u32(pos + 4) * 4294967296 + u32(pos)
        pos += 8
    if flg & 0x01:
        pos += 4
    pos += 1
    blocks = []
    while pos < n:
        w = u32(pos)
        pos += 4
        if w == 0:
            break
        blocks.append((pos, w))
        pos += w & 0x7FFFFFFF
        if flg & 0x10:
            pos += 4
    return [0, flg, size, len(blocks), 0, pos, bmax, int(pos > n)], blocks
