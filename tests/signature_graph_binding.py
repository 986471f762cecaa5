"""ctypes binding of tests/native/em2_signature_graph_restatement.cpp (createSignatureGraph, SignatureGraph::createEdges,
analyzeLshSignatures and Lsh::writeSignatureStatistics restated with the reference's containers) and the inputs the signature
graph tests share.  Compiled with g++ at first use.  Test infrastructure only."""
import ctypes
import functools
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE_DIR = os.path.join(ROOT, "tests", "native")
SOURCE = os.path.join(NATIVE_DIR, "em2_signature_graph_restatement.cpp")
FILES = ("Signatures.csv", "Histogram.csv", "LshSignatureStatistics.csv")

c = ctypes
P = c.c_void_p


def _ptr(a):
    return a.ctypes.data_as(c.c_void_p)


def word_count(lsh_count):
    return (lsh_count - 1) // 64 + 1


class SignatureGraphRestatement:
    def __init__(self, lib):
        self.lib = lib
        lib.em2r_signature_graph_create.argtypes = [P, c.c_uint32, c.c_uint32, c.c_uint64, P]
        lib.em2r_signature_graph_create.restype = P
        lib.em2r_signature_graph_sizes.argtypes = [P, P, P, P, P]
        lib.em2r_signature_graph_sizes.restype = None
        lib.em2r_signature_graph_get.argtypes = [P] * 6
        lib.em2r_signature_graph_get.restype = None
        lib.em2r_signature_graph_free.argtypes = [P]
        lib.em2r_signature_graph_free.restype = None
        lib.em2r_signature_statistics.argtypes = [P, c.c_uint32, c.c_uint32, P, P]
        lib.em2r_signature_statistics.restype = None
        lib.em2r_analyze_lsh_signatures.argtypes = [P, c.c_uint32, c.c_uint32, c.c_char_p]
        lib.em2r_analyze_lsh_signatures.restype = c.c_int

    def signature_graph(self, signatures, lsh_count, min_cell_count=0):
        """-> the dict of capi.signature_graph_take, and "seconds" (the map, the vertices and the edges on one thread)."""
        signatures = np.ascontiguousarray(signatures, dtype=np.uint64)
        assert signatures.ndim == 2 and signatures.shape[1] == word_count(lsh_count)
        seconds = c.c_double(0.)
        handle = self.lib.em2r_signature_graph_create(_ptr(signatures), signatures.shape[0], lsh_count, min_cell_count, c.byref(seconds))
        try:
            sizes = [c.c_uint64(0) for _ in range(4)]
            self.lib.em2r_signature_graph_sizes(handle, *[c.byref(s) for s in sizes])
            distinct, vertices, cells, edges = (s.value for s in sizes)
            out = {
                "vertexSignatures": np.zeros((vertices, signatures.shape[1]), dtype=np.uint64),
                "cellOffsets": np.zeros(vertices + 1, dtype=np.uint64),
                "cells": np.zeros(cells, dtype=np.uint32),
                "edgeVertex0": np.zeros(edges, dtype=np.uint32),
                "edgeVertex1": np.zeros(edges, dtype=np.uint32),
            }
            self.lib.em2r_signature_graph_get(handle, *[_ptr(out[key]) for key in (
                "vertexSignatures", "cellOffsets", "cells", "edgeVertex0", "edgeVertex1")])
            out["distinctCount"] = distinct
            out["seconds"] = seconds.value
        finally:
            self.lib.em2r_signature_graph_free(handle)
        return out

    def signature_statistics(self, signatures, lsh_count):
        """-> (setCount uint64 [lshCount], seconds)."""
        signatures = np.ascontiguousarray(signatures, dtype=np.uint64)
        set_count = np.zeros(lsh_count, dtype=np.uint64)
        seconds = c.c_double(0.)
        self.lib.em2r_signature_statistics(_ptr(signatures), signatures.shape[0], lsh_count, _ptr(set_count), c.byref(seconds))
        return set_count, seconds.value

    def analyze_lsh_signatures(self, signatures, lsh_count, directory):
        signatures = np.ascontiguousarray(signatures, dtype=np.uint64)
        assert self.lib.em2r_analyze_lsh_signatures(_ptr(signatures), signatures.shape[0], lsh_count, os.fsencode(directory)) == 0


@functools.lru_cache(maxsize=None)
def load():
    build = os.path.join(NATIVE_DIR, "build")
    os.makedirs(build, exist_ok=True)
    path = os.path.join(build, "libem2signaturegraphrestatement.so")
    if not os.path.exists(path) or os.path.getmtime(path) < os.path.getmtime(SOURCE):
        tmp = path + ".%d.tmp" % os.getpid()
        cmd = ["g++", "-std=c++17", "-O2", "-fPIC", "-shared", "-o", tmp, SOURCE]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError("signature graph restatement build failed: " + r.stderr)
        os.replace(tmp, path)
    return SignatureGraphRestatement(ctypes.CDLL(path))


def read_files(directory):
    return {name: open(os.path.join(directory, name), "rb").read() for name in FILES}


# ---- inputs ----

def pack_bits(bits):
    """bits [cells, lshCount] of 0 / 1 -> signatures uint64 [cells, words]: bit 0 is the most significant bit of word 0, the
    bits behind lshCount are zero."""
    bits = np.asarray(bits, dtype=np.uint8)
    cells, lsh_count = bits.shape
    padded = np.zeros((cells, word_count(lsh_count) * 64), dtype=np.uint8)
    padded[:, :lsh_count] = bits
    return np.ascontiguousarray(np.packbits(padded, axis=1).view(">u8").astype(np.uint64))


def of_integers(values, lsh_count):
    """Signatures of at most 64 bits from integers below 2^lshCount: bit i of the signature is bit lshCount - 1 - i of the value."""
    values = np.asarray(values, dtype=np.uint64)
    return np.ascontiguousarray((values << np.uint64(64 - lsh_count)).reshape(-1, 1))


def planted(lsh_count, cells, bases, flips, seed):
    """`bases` random signatures, the first of them once more with each bit of `flips` inverted, and random copies of all of
    those up to `cells` cells, shuffled."""
    rng = np.random.default_rng(seed)
    rows = [rng.integers(0, 2, lsh_count, dtype=np.uint8) for _ in range(bases)]
    for bit in flips:
        row = rows[0].copy()
        row[bit] ^= 1
        rows.append(row)
    rows = np.array(rows)
    assert len(rows) <= cells
    pick = np.concatenate([np.arange(len(rows)), rng.integers(0, len(rows), cells - len(rows))])
    return pack_bits(rows[rng.permutation(pick)])


def _hypercube(cells, seed):
    rng = np.random.default_rng(seed)
    values = rng.permutation(64) if cells == 64 else np.concatenate([rng.permutation(64), rng.integers(0, 64, cells - 64)])[rng.permutation(cells)]
    return of_integers(values, 6)


def _path_3_1_2():
    # 0000 x 3, 0100 x 1, 0110 x 2: a path; cells interleaved so that the ids of a group are not consecutive
    return of_integers([0b0000, 0b0110, 0b0000, 0b0100, 0b0110, 0b0000], 4)


def _sizes_1_2_3(seed=12):
    rng = np.random.default_rng(seed)
    values = rng.choice(4096, 100, replace=False)
    sizes = rng.integers(1, 4, 100)
    sizes[:3] = (1, 2, 3)
    return of_integers(rng.permutation(np.repeat(values, sizes)), 12)


@functools.lru_cache(maxsize=None)
def case(name):
    """(signatures [cells, words], lshCount) of a named input; built once, never modified (the array is read-only)."""
    if name.startswith("cells-"):                        # cells-<n>: random 8-bit signatures
        n = int(name.split("-")[1])
        out = of_integers(np.random.default_rng(n).integers(0, 256, n), 8), 8
    else:
        out = {
            "one-cell-one-bit": lambda: (of_integers([1], 1), 1),
            "one-bit-both": lambda: (of_integers([1, 0, 1], 1), 1),
            "hypercube": lambda: (_hypercube(64, 1), 6),
            "hypercube-200": lambda: (_hypercube(200, 2), 6),
            "bits-63": lambda: (planted(63, 40, 10, (0, 62), 63), 63),
            "bits-64": lambda: (planted(64, 40, 10, (0, 63), 64), 64),
            "bits-65": lambda: (planted(65, 40, 10, (0, 63, 64), 65), 65),
            "bits-128": lambda: (planted(128, 60, 20, (0, 63, 64, 127), 128), 128),
            "bits-1024": lambda: (planted(1024, 300, 40, (0, 63, 64, 511, 1023), 1024), 1024),
            "path-3-1-2": lambda: (_path_3_1_2(), 4),
            "one-group-70000": lambda: (of_integers(np.full(70000, 0x2a5), 10), 10),
            "uniform-20-bits": lambda: (of_integers(np.random.default_rng(20).integers(0, 1 << 20, 200000), 20), 20),
            "sizes-1-2-3": lambda: (_sizes_1_2_3(), 12),
        }[name]()
    out[0].setflags(write=False)
    return out


# (case, minCellCount)
GRAPH_CASES = [(name, 0) for name in (
    "one-cell-one-bit", "one-bit-both", "hypercube", "hypercube-200", "bits-63", "bits-64", "bits-65", "bits-128", "bits-1024",
    "one-group-70000", "cells-63", "cells-64", "cells-65", "cells-257", "uniform-20-bits", "sizes-1-2-3")] + [
    ("path-3-1-2", 0), ("path-3-1-2", 1), ("path-3-1-2", 2), ("path-3-1-2", 4), ("hypercube-200", 4), ("cells-257", 2)]
ANALYZE_CASES = ["hypercube-200", "uniform-20-bits", "sizes-1-2-3"]
GRAPH_KEYS = ("vertexSignatures", "cellOffsets", "cells", "edgeVertex0", "edgeVertex1")


@functools.lru_cache(maxsize=None)
def reference(name, min_cell_count):
    """The restatement's graph of a case; computed once and shared (the arrays are read-only)."""
    signatures, lsh_count = case(name)
    out = load().signature_graph(signatures, lsh_count, min_cell_count)
    for key in GRAPH_KEYS:
        out[key].setflags(write=False)
    return out


def assert_same_graph(mine, theirs, what):
    assert mine["distinctCount"] == theirs["distinctCount"], what
    for key in GRAPH_KEYS:
        assert mine[key].dtype == theirs[key].dtype and np.array_equal(mine[key], theirs[key]), "%s: %s differs" % (what, key)
