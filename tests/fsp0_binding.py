"""ctypes binding of tests/native/em2_fsp0_restatement.cpp, the C++ restatement of findSimilarPairs0
(src/ExpressionMatrixFindSimilarPairs.cpp:16-99) and analyzeSimilarPairs (src/ExpressionMatrixLsh.cpp:55-150), and the
inputs the fsp0 tests share.  Compiled with g++ at first use, with the flags of fsp6_binding.  Test infrastructure only."""
import ctypes
import os
import subprocess

import numpy as np

import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE_DIR = os.path.join(ROOT, "tests", "native")
SOURCE = os.path.join(NATIVE_DIR, "em2_fsp0_restatement.cpp")

COUNT_DTYPE = np.dtype([("gene", "<u4"), ("count", "<f4")])

c = ctypes
P = c.c_void_p


def _ptr(a):
    return a.ctypes.data_as(c.c_void_p)


class Fsp0Restatement:
    def __init__(self, lib):
        self.lib = lib
        lib.em2r_pair_similarities.argtypes = [P, P, c.c_uint32, c.c_uint32, P]
        lib.em2r_pair_similarities.restype = None
        lib.em2r_cell_similarity.argtypes = [P, P, c.c_uint32, c.c_uint32, c.c_uint32, c.c_uint32]
        lib.em2r_cell_similarity.restype = c.c_double
        lib.em2r_count_similar_pairs_of_rows.argtypes = [P, P, c.c_uint32, c.c_uint32, c.c_uint32, c.c_uint32, c.c_double]
        lib.em2r_count_similar_pairs_of_rows.restype = c.c_uint64
        lib.em2r_find_similar_pairs0.argtypes = [P, P, c.c_uint32, c.c_uint32, c.c_uint32, c.c_double, P, P, P, P, P]
        lib.em2r_find_similar_pairs0.restype = c.c_int
        lib.em2r_find_similar_pairs0_rows.argtypes = [P, P, c.c_uint32, c.c_uint32, c.c_uint32, c.c_uint32, c.c_uint32, c.c_double,
                                                      P, P, P, P, P]
        lib.em2r_find_similar_pairs0_rows.restype = c.c_int
        lib.em2r_analyze_similar_pairs.argtypes = [P, P, c.c_uint32, c.c_uint32, P, P, P, c.c_uint32, P, c.c_double,
                                                   c.c_char_p, c.c_char_p]
        lib.em2r_analyze_similar_pairs.restype = c.c_int

    @staticmethod
    def _csr(toc, data):
        return np.ascontiguousarray(toc, dtype=np.uint64), np.ascontiguousarray(data, dtype=COUNT_DTYPE)

    def pair_similarities(self, toc, data, gene_count):
        """float64 per unordered pair, cell 0 ascending, cell 1 > cell 0 ascending."""
        toc, data = self._csr(toc, data)
        n = len(toc) - 1
        out = np.zeros(n * (n - 1) // 2, dtype=np.float64)
        self.lib.em2r_pair_similarities(_ptr(toc), _ptr(data), n, gene_count, _ptr(out))
        return out

    def cell_similarity(self, toc, data, gene_count, cell0, cell1):
        toc, data = self._csr(toc, data)
        return self.lib.em2r_cell_similarity(_ptr(toc), _ptr(data), len(toc) - 1, gene_count, cell0, cell1)

    def count_similar_pairs_of_rows(self, toc, data, gene_count, row_begin, row_end, thr):
        toc, data = self._csr(toc, data)
        return int(self.lib.em2r_count_similar_pairs_of_rows(_ptr(toc), _ptr(data), len(toc) - 1, gene_count, row_begin, row_end, thr))

    def find_similar_pairs0(self, toc, data, gene_count, k, thr, rows=None):
        """-> (cell [n, k], similarity [n, k] float32, usedCount, lowestSimilarityIndex, lowestSimilarity); unused slots zero.
        rows = (begin, end): those rows only, each from its own candidates in ascending id (the arrays then have end - begin
        rows); the cost is that of the rows, not of all pairs."""
        toc, data = self._csr(toc, data)
        cells = len(toc) - 1
        n = cells if rows is None else rows[1] - rows[0]
        cell = np.zeros((n, k), dtype=np.uint32)
        sim = np.zeros((n, k), dtype=np.float32)
        used = np.zeros(n, dtype=np.uint32)
        low_index = np.zeros(n, dtype=np.uint32)
        low = np.zeros(n, dtype=np.float32)
        if rows is None:
            rc = self.lib.em2r_find_similar_pairs0(_ptr(toc), _ptr(data), cells, gene_count, k, thr, _ptr(cell), _ptr(sim), _ptr(used),
                                                   _ptr(low_index), _ptr(low))
        else:
            rc = self.lib.em2r_find_similar_pairs0_rows(_ptr(toc), _ptr(data), cells, gene_count, rows[0], rows[1], k, thr, _ptr(cell),
                                                        _ptr(sim), _ptr(used), _ptr(low_index), _ptr(low))
        if rc != 0:
            raise ValueError("the fsp0 restatement rejected the arguments (%d)" % rc)
        return cell, sim, used, low_index, low

    def analyze_similar_pairs(self, toc, data, gene_count, cell, sim, used, global_cell_ids, csv_downsample, pairs_csv, stats_csv):
        toc, data = self._csr(toc, data)
        cell = np.ascontiguousarray(cell, dtype=np.uint32)
        sim = np.ascontiguousarray(sim, dtype=np.float32)
        used = np.ascontiguousarray(used, dtype=np.uint32)
        ids = np.ascontiguousarray(global_cell_ids, dtype=np.uint32)
        k = cell.shape[1] if cell.ndim == 2 else 0
        return self.lib.em2r_analyze_similar_pairs(_ptr(toc), _ptr(data), len(toc) - 1, gene_count, _ptr(cell), _ptr(sim), _ptr(used),
                                                   k, _ptr(ids), csv_downsample, os.fsencode(pairs_csv), os.fsencode(stats_csv))


def load():
    build = os.path.join(NATIVE_DIR, "build")
    os.makedirs(build, exist_ok=True)
    path = os.path.join(build, "libem2fsp0restatement.so")
    if not os.path.exists(path) or os.path.getmtime(path) < os.path.getmtime(SOURCE):
        tmp = path + ".%d.tmp" % os.getpid()
        cmd = ["g++", "-std=c++17", "-O2", "-msse4.2", "-ffp-contract=off", "-fPIC", "-shared", "-o", tmp, SOURCE]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError("fsp0 restatement build failed: " + r.stderr)
        os.replace(tmp, path)
    return Fsp0Restatement(ctypes.CDLL(path))


# ---- inputs ----

def counts_of(genes, counts):
    data = np.empty(len(genes), dtype=COUNT_DTYPE)
    data["gene"] = genes
    data["count"] = counts
    return data


def clustered(cells, genes, density, seed=12345, cluster_count=8, non_integer=False):
    """synth.expression_matrix as (toc, data); non_integer: counts scaled by a per-entry factor that is no power of two, so
    that products round and the order of the double sum shows."""
    toc, g, cnt = synth.expression_matrix(cells, genes, density=density, cluster_count=cluster_count, seed=seed)
    if non_integer:
        factor = 0.37 + synth.uniform01(seed, 77, np.arange(len(cnt), dtype=np.uint64))
        cnt = (cnt.astype(np.float64) * factor).astype(np.float32)
    return toc, counts_of(g, cnt)


def wide_matrix():
    """1100 cells x 40 000 genes, about 20 non-integer counts per cell: more genes than LDS holds, so the kernels take their
    global-memory form, and more rows than that form has blocks (1024), so 76 blocks load a second row into a scratch vector
    that still holds the first row's values: only the bitmap may decide.  -> (toc, data, genes)"""
    toc, data = clustered(1100, 40000, 0.0005, seed=1100, cluster_count=6, non_integer=True)
    return toc, data, 40000


def repeat_cells(toc, data, pattern):
    """Cell c of the input appears pattern[c] times in a row: identical cells have identical similarities to every third
    cell, which puts exact ties at the eviction boundary of SimilarPairs::add."""
    toc = np.asarray(toc, dtype=np.uint64)
    pieces, lengths = [], []
    for cell, times in enumerate(pattern):
        begin, end = int(toc[cell]), int(toc[cell + 1])
        for _ in range(int(times)):
            pieces.append(data[begin:end])
            lengths.append(end - begin)
    out_toc = np.zeros(len(lengths) + 1, dtype=np.uint64)
    out_toc[1:] = np.cumsum(lengths)
    return out_toc, (np.concatenate(pieces) if pieces else np.zeros(0, dtype=COUNT_DTYPE))


def duplicated_cells_input():
    """The tie input of the fsp0 tests: 60 clustered cells, each 2 or 3 times (151 cells), 300 genes."""
    toc, data = clustered(60, 300, 0.08, seed=4242, cluster_count=3)
    pattern = 2 + (synth.hash_u64(99, np.arange(60, dtype=np.uint64)) % np.uint64(2)).astype(np.int64)
    toc, data = repeat_cells(toc, data, pattern)
    return toc, data, 300


def best_k_by_similarity_then_id(exact, cell_count, k, thr):
    """What findSimilarPairs0 is NOT: per cell the k candidates above the threshold that are best by (float similarity
    descending, id ascending).  -> (cell [n, k], similarity [n, k], usedCount)."""
    sims = np.zeros((cell_count, cell_count), dtype=np.float64)
    iu = np.triu_indices(cell_count, 1)
    sims[iu] = exact
    sims = sims + sims.T
    cell = np.zeros((cell_count, k), dtype=np.uint32)
    sim = np.zeros((cell_count, k), dtype=np.float32)
    used = np.zeros(cell_count, dtype=np.uint32)
    for c0 in range(cell_count):
        candidates = [(-np.float32(sims[c0, c1]), c1) for c1 in range(cell_count) if c1 != c0 and sims[c0, c1] > thr]
        candidates.sort()
        candidates = candidates[:k]
        used[c0] = len(candidates)
        for i, (negative, c1) in enumerate(candidates):
            cell[c0, i] = c1
            sim[c0, i] = -negative
    return cell, sim, used
