"""ctypes binding of tests/native/em2_gene_pairs_restatement.cpp, the C++ restatement of findSimilarGenePairs0
(src/ExpressionMatrixFindSimilarGenePairs.cpp:16-198), and the inputs the gene pairs tests share.  Compiled with g++ at first
use, with the flags of fsp0_binding.  Test infrastructure only."""
import ctypes
import os
import subprocess

import numpy as np

import fsp0_binding

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE_DIR = os.path.join(ROOT, "tests", "native")
SOURCE = os.path.join(NATIVE_DIR, "em2_gene_pairs_restatement.cpp")

COUNT_DTYPE = fsp0_binding.COUNT_DTYPE
NONE, L1, L2 = 0, 1, 2

c = ctypes
P = c.c_void_p


def _ptr(a):
    return a.ctypes.data_as(c.c_void_p)


class GenePairsRestatement:
    def __init__(self, lib):
        self.lib = lib
        lib.em2r_find_similar_gene_pairs0.argtypes = [P, P, c.c_uint32, c.c_uint32, c.c_int, c.c_uint32, c.c_double, P, P, P, P]
        lib.em2r_find_similar_gene_pairs0.restype = c.c_int
        lib.em2r_gene_pair_band.argtypes = [P, P, c.c_uint32, c.c_uint32, c.c_int, c.c_uint32, c.c_uint32, P, P]
        lib.em2r_gene_pair_band.restype = c.c_int
        lib.em2r_keep_best_and_sort.argtypes = [P, c.c_uint32, c.c_uint32, c.c_double, P, P, P]
        lib.em2r_keep_best_and_sort.restype = c.c_int

    def find_similar_gene_pairs0(self, toc, data, gene_count, method, k, thr, all_similarities=True):
        """-> (gene [G, k], similarity [G, k] float32, usedCount [G], r [G, G] float32 or None); unused slots zero."""
        toc = np.ascontiguousarray(toc, dtype=np.uint64)
        data = np.ascontiguousarray(data, dtype=COUNT_DTYPE)
        gene = np.zeros((gene_count, k), dtype=np.uint32)
        sim = np.zeros((gene_count, k), dtype=np.float32)
        used = np.zeros(gene_count, dtype=np.uint32)
        r = np.zeros((gene_count, gene_count), dtype=np.float32) if all_similarities else None
        rc = self.lib.em2r_find_similar_gene_pairs0(_ptr(toc), _ptr(data), len(toc) - 1, gene_count, method, k, thr, _ptr(gene),
                                                    _ptr(sim), _ptr(used), _ptr(r) if all_similarities else None)
        if rc != 0:
            raise ValueError("the gene pairs restatement rejected the arguments (%d)" % rc)
        return gene, sim, used, r

    def gene_pair_band(self, toc, data, gene_count, method, gene_begin, gene_end):
        """-> (r [gene_end - gene_begin, G] float32, filled for partner < gene; seconds of the inner products)."""
        toc = np.ascontiguousarray(toc, dtype=np.uint64)
        data = np.ascontiguousarray(data, dtype=COUNT_DTYPE)
        out = np.zeros((gene_end - gene_begin, gene_count), dtype=np.float32)
        seconds = c.c_double(0.)
        rc = self.lib.em2r_gene_pair_band(_ptr(toc), _ptr(data), len(toc) - 1, gene_count, method, gene_begin, gene_end, _ptr(out),
                                          c.byref(seconds))
        if rc != 0:
            raise ValueError("the gene pairs restatement rejected the arguments (%d)" % rc)
        return out, seconds.value

    def keep_best_and_sort(self, r, k, thr):
        """The stored list of a gene whose only partners are 0 .. len(r)-1 with these r (the last gene of a problem): the
        survivors in ascending id through keepBest and std::sort -> (gene [k], similarity [k], usedCount)."""
        r = np.ascontiguousarray(r, dtype=np.float32)
        gene = np.zeros(k, dtype=np.uint32)
        sim = np.zeros(k, dtype=np.float32)
        used = c.c_uint32(0)
        self.lib.em2r_keep_best_and_sort(_ptr(r), len(r), k, thr, _ptr(gene), _ptr(sim), c.byref(used))
        return gene, sim, used.value


def load():
    build = os.path.join(NATIVE_DIR, "build")
    os.makedirs(build, exist_ok=True)
    path = os.path.join(build, "libem2genepairsrestatement.so")
    if not os.path.exists(path) or os.path.getmtime(path) < os.path.getmtime(SOURCE):
        tmp = path + ".%d.tmp" % os.getpid()
        cmd = ["g++", "-std=c++17", "-O2", "-msse4.2", "-ffp-contract=off", "-fPIC", "-shared", "-o", tmp, SOURCE]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError("gene pairs restatement build failed: " + r.stderr)
        os.replace(tmp, path)
    return GenePairsRestatement(ctypes.CDLL(path))


# ---- inputs ----

def csr_of_cells(cells):
    """cells: a list of (gene ids ascending, counts) per cell -> (toc, data)."""
    toc = np.zeros(len(cells) + 1, dtype=np.uint64)
    toc[1:] = np.cumsum([len(g) for g, _ in cells])
    data = np.zeros(int(toc[-1]), dtype=COUNT_DTYPE)
    at = 0
    for g, cnt in cells:
        data["gene"][at:at + len(g)] = g
        data["count"][at:at + len(g)] = cnt
        at += len(g)
    return toc, data


def dense_to_csr(dense):
    """dense [cells, genes] float32 -> (toc, data) of its nonzero entries."""
    return csr_of_cells([(np.nonzero(row)[0].astype(np.uint32), row[np.nonzero(row)[0]]) for row in dense])


def to_dense(toc, data, gene_count):
    cells = len(toc) - 1
    dense = np.zeros((cells, gene_count), dtype=np.float32)
    for cell in range(cells):
        b, e = int(toc[cell]), int(toc[cell + 1])
        dense[cell, data["gene"][b:e]] = data["count"][b:e]
    return dense


def tie_input(seed=7):
    """An input full of exact ties: 40 cells x 90 genes.  Genes 0..29 are clustered non-integer data; genes 30..59 repeat
    them (gene 30 + i is gene i: every r of one equals the r of the other, and r(i, 30 + i) is that of a gene with itself);
    genes 60..89 are each expressed in exactly one cell, three cells shared by ten genes each, so within such a group every
    pair has the same r and all of them the same r to every third gene."""
    toc, data = fsp0_binding.clustered(40, 30, 0.35, seed=seed, cluster_count=3, non_integer=True)
    dense = np.zeros((40, 90), dtype=np.float32)
    dense[:, :30] = to_dense(toc, data, 30)
    dense[:, 30:60] = dense[:, :30]
    for i in range(30):
        dense[(3, 17, 31)[i // 10], 60 + i] = 2.0 + (i // 10)
    toc, data = dense_to_csr(dense)
    return toc, data, 90


def best_k_by_similarity_then_id(r, k, thr):
    """What findSimilarGenePairs0 is NOT: per gene the k partners above the threshold that are best by (similarity descending,
    id ascending).  -> (gene [G, k], similarity [G, k], usedCount)."""
    n = r.shape[0]
    gene = np.zeros((n, k), dtype=np.uint32)
    sim = np.zeros((n, k), dtype=np.float32)
    used = np.zeros(n, dtype=np.uint32)
    for g0 in range(n):
        candidates = sorted((-r[g0, g1], g1) for g1 in range(n) if g1 != g0 and np.float64(r[g0, g1]) > thr)[:k]
        used[g0] = len(candidates)
        for i, (negative, g1) in enumerate(candidates):
            gene[g0, i] = g1
            sim[g0, i] = -negative
    return gene, sim, used
