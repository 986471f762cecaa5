"""ctypes binding of tests/native/em2_rank_genes_restatement.cpp (the rank-sum test of em2_rank_genes restated for one thread
from the definition of a mid-rank), an independent numpy statement over dense columns (np.unique), and the inputs the rank
genes tests share.  Compiled with g++ at first use.  Test infrastructure only."""
import ctypes
import functools
import math
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE_DIR = os.path.join(ROOT, "tests", "native")
SOURCE = os.path.join(NATIVE_DIR, "em2_rank_genes_restatement.cpp")
HEADER = os.path.join(ROOT, "expressionmatrix2_amd", "csrc", "em2_rank_genes_host.h")

COUNT_DTYPE = np.dtype([("gene", "<u4"), ("count", "<f4")])
NO_GROUP = 0xffffffff
INTEGERS = ("groupSize", "nonZeroCount", "rankSum2", "tieSum")
DOUBLES = ("zScore", "auc")

c = ctypes
P = c.c_void_p


def _ptr(a):
    return a.ctypes.data_as(c.c_void_p) if a is not None else None


class RankGenesRestatement:
    def __init__(self, lib):
        self.lib = lib
        lib.em2r_rank_genes.argtypes = [P, P, c.c_uint32, c.c_uint32, c.c_uint32, P, P, c.c_uint32, P, P, P, P, P, P, P]
        lib.em2r_rank_genes.restype = c.c_int

    def rank_genes(self, toc, data, gene_count, group, group_count, norm_inverse=None, gene_begin=0, gene_end=None):
        """-> dict(groupSize, nonZeroCount, rankSum2, tieSum, zScore, auc, seconds) for the genes [gene_begin, gene_end);
        ValueError where a value is NaN."""
        toc = np.ascontiguousarray(toc, dtype=np.uint64)
        data = np.ascontiguousarray(data, dtype=COUNT_DTYPE)
        group = np.ascontiguousarray(group, dtype=np.uint32)
        gene_end = gene_count if gene_end is None else gene_end
        n = gene_end - gene_begin
        if norm_inverse is not None:
            norm_inverse = np.ascontiguousarray(norm_inverse, dtype=np.float64)
        out = {"groupSize": np.zeros(group_count, np.uint32), "nonZeroCount": np.zeros((n, group_count), np.uint32),
               "rankSum2": np.zeros((n, group_count), np.uint64), "tieSum": np.zeros(n, np.uint64),
               "zScore": np.zeros((n, group_count), np.float64), "auc": np.zeros((n, group_count), np.float64)}
        seconds = c.c_double(0.)
        rc = self.lib.em2r_rank_genes(_ptr(toc), _ptr(data), len(toc) - 1, gene_begin, gene_end, _ptr(norm_inverse), _ptr(group),
                                      group_count, _ptr(out["groupSize"]), _ptr(out["nonZeroCount"]), _ptr(out["rankSum2"]),
                                      _ptr(out["tieSum"]), _ptr(out["zScore"]), _ptr(out["auc"]), c.byref(seconds))
        if rc != 0:
            raise ValueError("a value is not a number")
        out["seconds"] = seconds.value
        return out


@functools.lru_cache(maxsize=None)
def load():
    build = os.path.join(NATIVE_DIR, "build")
    os.makedirs(build, exist_ok=True)
    path = os.path.join(build, "libem2rankgenesrestatement.so")
    newest = max(os.path.getmtime(SOURCE), os.path.getmtime(HEADER))
    if not os.path.exists(path) or os.path.getmtime(path) < newest:
        tmp = path + ".%d.tmp" % os.getpid()
        cmd = ["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-o", tmp, SOURCE]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError("rank genes restatement build failed: " + r.stderr)
        os.replace(tmp, path)
    return RankGenesRestatement(ctypes.CDLL(path))


# ---- the independent numpy statement ----

def dense_values(toc, data, gene_count, norm_inverse=None):
    """float32 [cells][genes]: count * float32(normInverse) where stored (a float32 product), +0 elsewhere, -0 as +0."""
    cells = len(toc) - 1
    rows = np.repeat(np.arange(cells), np.diff(np.asarray(toc).astype(np.int64)))
    with np.errstate(all="ignore"):
        value = data["count"] if norm_inverse is None else data["count"] * np.asarray(norm_inverse, np.float64).astype(np.float32)[rows]
    dense = np.zeros((cells, gene_count), dtype=np.float32)
    dense[rows, data["gene"]] = value
    return dense + np.float32(0)                           # (-0) + (+0) = +0


def statistics(cell_count, group_size, rank_sum2, tie_sum):
    """zScore and auc [genes][groups] from the integers, in the order csrc/em2_rank_genes_host.h states (numpy's float64
    operations round once each, as the header's)."""
    N = int(cell_count)
    n = group_size.astype(np.int64)[None, :]
    m = N - n
    u2 = rank_sum2.astype(np.int64) - n * (n + 1)
    num = u2 - n * m
    s = (N * N * N - N - tie_sum.astype(np.int64))[:, None]
    with np.errstate(all="ignore"):
        var = ((n.astype(np.float64) * m.astype(np.float64)) * s.astype(np.float64)) / ((12. * np.float64(N)) * np.float64(N - 1))
        z = np.where(var > 0., (0.5 * num.astype(np.float64)) / np.sqrt(var), 0.)
        auc = np.where(n * m != 0, u2.astype(np.float64) / ((2. * n.astype(np.float64)) * m.astype(np.float64)), 0.5)
    return z, auc + np.zeros_like(z)


def numpy_statement(toc, data, gene_count, group, group_count, norm_inverse=None):
    """The same dict from dense columns: np.unique gives the tie groups of a column, the cumulative counts their mid-ranks."""
    dense = dense_values(toc, data, gene_count, norm_inverse)
    if np.isnan(dense).any():
        raise ValueError("a value is not a number")
    cells = dense.shape[0]
    group = np.asarray(group, dtype=np.uint32)
    member = group != NO_GROUP
    out = {"groupSize": np.bincount(group[member], minlength=group_count).astype(np.uint32),
           "nonZeroCount": np.zeros((gene_count, group_count), np.uint32), "rankSum2": np.zeros((gene_count, group_count), np.uint64),
           "tieSum": np.zeros(gene_count, np.uint64)}
    for g in range(gene_count):
        _, inverse, counts = np.unique(dense[:, g], return_inverse=True, return_counts=True)
        counts = counts.astype(np.int64)
        twice = (2 * np.cumsum(counts) - counts + 1)[inverse.reshape(-1)]           # 2 * (last rank - (t - 1) / 2)
        out["tieSum"][g] = int(np.sum(counts ** 3 - counts))
        sums = np.zeros(group_count, np.int64)
        np.add.at(sums, group[member], twice[member])
        out["rankSum2"][g] = sums
        out["nonZeroCount"][g] = np.bincount(group[member & (dense[:, g] != 0)], minlength=group_count)
    out["zScore"], out["auc"] = statistics(cells, out["groupSize"], out["rankSum2"], out["tieSum"])
    return out


def p_values(z):
    """The facade's two-sided p: erfc(|z| / sqrt(2)) with math.erfc."""
    return np.vectorize(lambda x: math.erfc(abs(x) / math.sqrt(2.)), otypes=[np.float64])(z)


def assert_same(mine, theirs, what, names=INTEGERS + DOUBLES):
    """Bit for bit: the integers equal, the doubles with equal bit patterns."""
    for name in names:
        a, b = np.asarray(mine[name]), np.asarray(theirs[name])
        assert a.shape == b.shape, "%s: %s has shape %s, not %s" % (what, name, a.shape, b.shape)
        if a.dtype == np.float64:
            a, b = a.view(np.uint64), b.view(np.uint64)
        assert np.array_equal(a, b), "%s: %s differs at %s" % (what, name, np.argwhere(a != b)[:5].tolist())


# ---- inputs ----

def csr_of_dense(dense, stored):
    """(toc, data) of the cells' rows: the entries where `stored`."""
    cells, genes = np.nonzero(stored)
    toc = np.zeros(dense.shape[0] + 1, dtype=np.uint64)
    toc[1:] = np.cumsum(np.bincount(cells, minlength=dense.shape[0]))
    data = np.zeros(len(cells), dtype=COUNT_DTYPE)
    data["gene"] = genes
    data["count"] = dense[cells, genes]
    return toc, data


def random_case(cells, genes, groups, seed, density=0.3, ungrouped=0.1):
    """Counts from a handful of small values (many ties) and some non-integers; groups at random, some cells in none.  From
    three cells on, cell 1 is empty (its norm inverses are inf)."""
    rng = np.random.default_rng(seed)
    stored = rng.random((cells, genes)) < density
    if cells >= 3:
        stored[1, :] = False
    dense = np.where(rng.random((cells, genes)) < 0.7, rng.integers(1, 5, (cells, genes)).astype(np.float32),
                     rng.gamma(1.5, 2.0, (cells, genes)).astype(np.float32))
    group = rng.integers(0, groups, cells).astype(np.uint32)
    group[rng.random(cells) < ungrouped] = NO_GROUP
    toc, data = csr_of_dense(dense, stored)
    return toc, data, genes, group, groups


def odd_case(seed=3):
    """120 cells x 9 genes, 4 groups of which group 3 is empty, some cells in none.  Gene 0: stored zeros among positives; gene
    1: negative counts, a stored -0 and a stored +0; gene 2: +inf and -inf; gene 3: stored nowhere; gene 4: stored zeros only;
    gene 5: one value in every cell but cell 7; gene 6: all distinct but for cell 7; genes 7, 8: random.  Cell 7 is empty."""
    rng = np.random.default_rng(seed)
    cells, genes = 120, 9
    stored = rng.random((cells, genes)) < 0.4
    dense = rng.integers(1, 4, (cells, genes)).astype(np.float32)
    dense[:, 0][rng.random(cells) < 0.3] = 0.
    dense[:, 1] = rng.integers(-3, 3, cells)
    stored[[2, 3], 1], dense[2, 1], dense[3, 1] = True, -0., 0.
    stored[[4, 5, 6], 2], dense[4, 2], dense[5, 2], dense[6, 2] = True, np.inf, -np.inf, np.inf
    stored[:, 3] = False
    dense[:, 4] = 0.
    stored[:, 5], dense[:, 5] = True, 2.5
    stored[:, 6], dense[:, 6] = True, rng.permutation(cells).astype(np.float32) - 30.5
    stored[7, :] = False
    group = rng.integers(0, 3, cells).astype(np.uint32)
    group[rng.random(cells) < 0.15] = NO_GROUP
    toc, data = csr_of_dense(dense, stored)
    return toc, data, genes, group, 4


def chunk_case(seed=4):
    """300 cells x 5 genes for a chunk of 64 entries: gene 0 stored in all 300 cells with one value (one run crosses five
    chunks), gene 1 all distinct, gene 2 stored nowhere, gene 3 stored zeros only, gene 4 random with negatives."""
    rng = np.random.default_rng(seed)
    cells, genes = 300, 5
    stored = np.zeros((cells, genes), dtype=bool)
    dense = np.zeros((cells, genes), dtype=np.float32)
    stored[:, 0], dense[:, 0] = True, 7.
    stored[:, 1], dense[:, 1] = True, rng.permutation(cells).astype(np.float32) + 1.
    stored[rng.random(cells) < 0.5, 3] = True
    stored[:, 4] = rng.random(cells) < 0.7
    dense[:, 4] = rng.integers(-2, 3, cells)
    group = rng.integers(0, 3, cells).astype(np.uint32)
    group[rng.random(cells) < 0.1] = NO_GROUP
    toc, data = csr_of_dense(dense, stored)
    return toc, data, genes, group, 3


@functools.lru_cache(maxsize=None)
def case(name):
    """(toc, data, gene_count, group, group_count) of a named input; built once, never modified (the arrays are read-only).
    random-<cells>x<genes>x<groups>."""
    if name.startswith("random"):
        cells, genes, groups = (int(x) for x in name.split("-")[1].split("x"))
        out = random_case(cells, genes, groups, seed=cells * 131 + genes * 7 + groups, density=1.0 if cells <= 2 else 0.3)
    else:
        out = {"odd": odd_case, "chunks": chunk_case}[name]()
    for a in (out[0], out[1], out[3]):
        a.setflags(write=False)
    return out


def norm_inverses(toc, data):
    """(norm1Inverse, norm2Inverse) of the cells of the CSR itself, as ExpressionMatrix::addCell defines them: double sums of
    the counts and of their float squares, in stored order (inf for an empty cell)."""
    n1 = np.zeros(len(toc) - 1, dtype=np.float64)
    n2 = np.zeros(len(toc) - 1, dtype=np.float64)
    with np.errstate(all="ignore"):
        for cell in range(len(toc) - 1):
            counts = data["count"][int(toc[cell]):int(toc[cell + 1])]
            sum1 = sum2 = 0.
            for v in counts:
                sum1 += float(v)
                sum2 += float(np.float32(v) * np.float32(v))
            n1[cell] = np.float64(1.) / np.float64(sum1)
            n2[cell] = np.float64(1.) / np.sqrt(np.float64(sum2))
    return n1, n2
