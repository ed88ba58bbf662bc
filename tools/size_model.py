#!/usr/bin/env python3
"""Host model of the size kernel (tools/proto/size_kernel_model.cpp): checks it against
lz4mi_host_decoded_size on the size tests' inputs and prints the certification passes per 1 KiB
chunk for each generator at the given warm-up distances. No device needed.

  python tools/size_model.py [64 256 512]
"""
import ctypes
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "divortio-lz4_amd")):
    sys.path.insert(0, p)

import lz4mi  # noqa: E402
import oracle as O  # noqa: E402
import sizes_common as C  # noqa: E402


def main():
    warms = [int(a) for a in sys.argv[1:]] or [64, 256, 512]
    with tempfile.TemporaryDirectory() as d:
        so = os.path.join(d, "libsizemodel.so")
        subprocess.run(["g++", "-O2", "-shared", "-fPIC", "-o", so,
                        os.path.join(ROOT, "tools", "proto", "size_kernel_model.cpp")], check=True)
        E = ctypes.CDLL(so)
        E.emu_size.restype = ctypes.c_uint32
        E.emu_size.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p]
        passes = ctypes.c_uint64.in_dll(E, "g_passes")
        chunks = ctypes.c_uint64.in_dll(E, "g_chunks")

        def model(b):
            b = np.ascontiguousarray(b)
            st = ctypes.c_int32(0)
            r = E.emu_size(b.ctypes.data if b.size else None, b.size, ctypes.addressof(st))
            return st.value, r

        def check(name, blocks):
            passes.value = chunks.value = 0
            bad = sum(model(b) != lz4mi.host_decoded_size(b) for b in blocks)
            print(f"  {name:12s} blocks {len(blocks):5d}  differ from the host walker {bad}  "
                  f"passes/chunk {passes.value / max(1, chunks.value):.2f}")
            return bad

        n = 4 << 20
        sets = [("chunk edges", C.chunk_edge_blocks()), ("prefixes/7", C.prefixes()[::7]),
                ("mutations", [m for part in C.mutations() for m in part])]
        for kind in C.GENERATOR_KINDS:
            sets.append((kind, [O.compress_block_bytes(O.generate(kind, 5, k)) for k in C.SOURCE_SIZES] +
                         [O.compress_block_bytes(O.generate(kind, 9, n))]))
        sets.append(("zeros, p3", [O.compress_block_bytes(np.zeros(n, np.uint8)),
                                   O.compress_block_bytes(np.tile(np.array([1, 2, 3], np.uint8), n // 3 + 1)[:n])]))
        bad = 0
        for w in warms:
            E.emu_set_warm(w)
            print(f"warm-up {w} bytes")
            for name, blocks in sets:
                bad += check(name, blocks)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
