"""LZ4MI_LINKED without a device: the flag in the header and the binding, and the `linked`
parameter of the three Python entry points (its GPU tests: tests/test_gpu_linked.py)."""
import inspect
import os
import re

import pytest

from conftest import ROOT

lz4mi = pytest.importorskip("lz4mi")


def test_header_defines_the_flag():
    with open(os.path.join(ROOT, "include", "lz4mi.h")) as f:
        text = f.read()
    m = re.search(r"^#define\s+LZ4MI_LINKED\s+(\S+)", text, re.M)
    assert m and m.group(1) == "0x80u"
    flags = {n: int(v.rstrip("u"), 16) for n, v in re.findall(r"^#define\s+(LZ4MI_[A-Z0-9_]+)\s+(0x[0-9A-Fa-f]+u)\b", text, re.M)
             if n != "LZ4MI_MAX_BLOCK"}
    assert flags["LZ4MI_LINKED"] == 0x80
    assert sum(v == 0x80 for v in flags.values()) == 1       # no other flag shares the bit


def test_binding_constant():
    assert lz4mi.LINKED == 0x80
    assert lz4mi.LINKED & (lz4mi.DEVICE_PTRS | lz4mi.JS_COMPAT | lz4mi.JS_EXACT | lz4mi.XXH_STANDARD |
                           lz4mi.XXH_LEN64 | lz4mi.BLOCK_CHECKSUM | lz4mi.FRAME_WORDS) == 0


def test_entry_points_accept_linked():
    from lz4mi import frame as F
    for fn in (lz4mi.decompress_blocks, lz4mi.decompress_blocks_dev, lz4mi.frame_decompress_dev,
               F.decompress_frame_device):
        p = inspect.signature(fn).parameters.get("linked")
        assert p is not None and p.default is False, fn.__name__
