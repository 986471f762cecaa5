"""ctypes binding of tests/native/em2_dense_restatement.cpp (getDenseExpressionMatrix on a restricted CSR; deduplicate, the
std::set_* steps and the mt19937 downsampling of the cell set operations) and what the dense read-out tests share.
Compiled with g++ at first use.  Test infrastructure only."""
import ctypes
import functools
import os
import subprocess

import numpy as np

import expression_cases as ec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE_DIR = os.path.join(ROOT, "tests", "native")
SOURCE = os.path.join(NATIVE_DIR, "em2_dense_restatement.cpp")
COUNT_DTYPE = np.dtype([("gene", "<u4"), ("count", "<f4")])
UNION, INTERSECTION, DIFFERENCE = 0, 1, 2

c = ctypes
P = c.c_void_p


def _ptr(a):
    return a.ctypes.data_as(c.c_void_p)


class DenseRestatement:
    def __init__(self, lib):
        self.lib = lib
        lib.em2r_dense_expression.argtypes = [P, P, c.c_uint32, c.c_uint32, c.c_int, P, P]
        lib.em2r_dense_expression.restype = c.c_int
        lib.em2r_deduplicate.argtypes = [P, c.c_uint64, P]
        lib.em2r_deduplicate.restype = c.c_uint64
        lib.em2r_set_operation.argtypes = [c.c_int, P, c.c_uint64, P, c.c_uint64, P]
        lib.em2r_set_operation.restype = c.c_uint64
        lib.em2r_downsample.argtypes = [P, c.c_uint64, c.c_double, c.c_int, P]
        lib.em2r_downsample.restype = c.c_uint64

    def dense_expression(self, toc, data, gene_count, method, with_seconds=False):
        """float64 [cells, gene_count] of a CSR in local ids (the reference's array)."""
        toc = np.ascontiguousarray(toc, dtype=np.uint64)
        data = np.ascontiguousarray(data, dtype=COUNT_DTYPE)
        cells = len(toc) - 1
        out = np.zeros((cells, gene_count), dtype=np.float64)
        seconds = c.c_double(0.)
        rc = self.lib.em2r_dense_expression(_ptr(toc), _ptr(data), cells, gene_count, int(method), _ptr(out), c.byref(seconds))
        if rc != 0:
            raise RuntimeError("Invalid normalization method.")
        return (out, seconds.value) if with_seconds else out

    def deduplicate(self, ids):
        ids = np.ascontiguousarray(ids, dtype=np.uint32)
        out = np.zeros(len(ids), dtype=np.uint32)
        return out[:self.lib.em2r_deduplicate(_ptr(ids), len(ids), _ptr(out))]

    def set_operation(self, operation, a, b):
        a = np.ascontiguousarray(a, dtype=np.uint32)
        b = np.ascontiguousarray(b, dtype=np.uint32)
        out = np.zeros(len(a) + len(b), dtype=np.uint32)
        return out[:self.lib.em2r_set_operation(operation, _ptr(a), len(a), _ptr(b), len(b), _ptr(out))]

    def downsample(self, ids, probability, seed):
        """seed: a Python int, wrapped to the reference's 32-bit int."""
        ids = np.ascontiguousarray(ids, dtype=np.uint32)
        out = np.zeros(len(ids), dtype=np.uint32)
        wrapped = int(seed) & 0xffffffff
        wrapped -= (wrapped & 0x80000000) << 1
        return out[:self.lib.em2r_downsample(_ptr(ids), len(ids), probability, wrapped, _ptr(out))]


@functools.lru_cache(maxsize=None)
def load():
    build = os.path.join(NATIVE_DIR, "build")
    os.makedirs(build, exist_ok=True)
    path = os.path.join(build, "libem2denserestatement.so")
    if not os.path.exists(path) or os.path.getmtime(path) < os.path.getmtime(SOURCE):
        tmp = path + ".%d.tmp" % os.getpid()
        cmd = ["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-o", tmp, SOURCE]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError("dense restatement build failed: " + r.stderr)
        os.replace(tmp, path)
    return DenseRestatement(ctypes.CDLL(path))


def dense_difference(name, got, expected):
    """None, or how the device's matrix differs from the restatement's (float64).  NaNs must sit at the same places; they are
    then replaced by 0 in both -- the sign and payload of an inf * 0 NaN differ between x86 and the GPU and carry no
    information -- and everything is compared bit for bit (expression_cases.first_difference).  A float32 result is compared
    with the restatement narrowed to float32, which loses nothing: every element is a float before the reference widens it."""
    got = np.ascontiguousarray(got)
    expected = np.ascontiguousarray(expected, dtype=np.float64)
    if got.dtype == np.float32:
        narrowed = expected.astype(np.float32)
        finite = ~np.isnan(expected)
        assert np.array_equal(narrowed[finite].astype(np.float64), expected[finite]), "the restatement holds a value that is no float"
        expected = narrowed
    if got.shape != expected.shape:
        return "%s: shape %s, expected %s" % (name, got.shape, expected.shape)
    nan_got, nan_expected = np.isnan(got), np.isnan(expected)
    if not np.array_equal(nan_got, nan_expected):
        rows = np.nonzero((nan_got != nan_expected).reshape(len(got), -1).any(axis=1))[0]
        return "%s: NaNs at other places in %d rows, first %s" % (name, len(rows), rows[:12].tolist())
    return ec.first_difference([name], [np.where(nan_got, 0, got)], [np.where(nan_expected, 0, expected)])


def local_ids_of(gene_set, global_gene_count=None):
    """GeneSet-*-LocalIds of ascending global ids: sized by the largest id + 1 (GeneSet::addGene), or by global_gene_count."""
    gene_set = np.asarray(gene_set, dtype=np.uint32)
    size = (int(gene_set[-1]) + 1 if len(gene_set) else 0) if global_gene_count is None else global_gene_count
    local = np.full(size, 0xffffffff, dtype=np.uint32)
    local[gene_set] = np.arange(len(gene_set), dtype=np.uint32)
    return local


def restrict(toc, data, cell_ids, gene_set):
    """ExpressionMatrixSubset as arrays, in numpy: the rows cell_ids of a CSR in global ids, the genes of gene_set (ascending
    global ids) under their local ids, stored order kept -> (toc, data)."""
    toc = np.asarray(toc, dtype=np.uint64)
    local = local_ids_of(gene_set)
    pieces, out_toc = [], [0]
    for cell in cell_ids:
        row = data[int(toc[cell]):int(toc[cell + 1])]
        known = row["gene"] < len(local)
        row = row[known]
        mapped = local[row["gene"]]
        keep = mapped != 0xffffffff
        piece = np.zeros(int(keep.sum()), dtype=COUNT_DTYPE)
        piece["gene"] = mapped[keep]
        piece["count"] = row["count"][keep]
        pieces.append(piece)
        out_toc.append(out_toc[-1] + len(piece))
    return np.array(out_toc, dtype=np.uint64), (np.concatenate(pieces) if pieces else np.zeros(0, dtype=COUNT_DTYPE))
