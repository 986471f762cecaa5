"""ctypes binding of tests/native/em2_gene_information_restatement.cpp (computeGeneInformationContent,
src/ExpressionMatrix.cpp:1947-2018, restated line by line), the higher-precision statement R the doubles are held against, and the
inputs the gene information tests share.  Compiled with g++ at first use.  Test infrastructure only."""
import ctypes
import functools
import math
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE_DIR = os.path.join(ROOT, "tests", "native")
SOURCE = os.path.join(NATIVE_DIR, "em2_gene_information_restatement.cpp")

COUNT_DTYPE = np.dtype([("gene", "<u4"), ("count", "<f4")])
NONE, L1, L2 = 0, 1, 2
CHUNK = 1024          # kGeneInformationChunk (csrc/em2_device.h): the entries of a gene one wave reduces

c = ctypes
P = c.c_void_p


def _ptr(a):
    return a.ctypes.data_as(c.c_void_p) if a is not None else None


class GeneInformationRestatement:
    def __init__(self, lib):
        self.lib = lib
        lib.em2r_cell_norm_inverses.argtypes = [P, P, c.c_uint32, P, P]
        lib.em2r_cell_norm_inverses.restype = c.c_int
        lib.em2r_gene_information_content.argtypes = [P, P, c.c_uint32, c.c_uint32, c.c_uint32, P, P, P, P, P, P, P]
        lib.em2r_gene_information_content.restype = c.c_int

    def cell_norm_inverses(self, toc, data):
        toc = np.ascontiguousarray(toc, dtype=np.uint64)
        data = np.ascontiguousarray(data, dtype=COUNT_DTYPE)
        n1 = np.zeros(len(toc) - 1, dtype=np.float64)
        n2 = np.zeros(len(toc) - 1, dtype=np.float64)
        self.lib.em2r_cell_norm_inverses(_ptr(toc), _ptr(data), len(toc) - 1, _ptr(n1), _ptr(n2))
        return n1, n2

    def gene_information_content(self, toc, data, gene_count, norm_inverse=None, gene_begin=0, gene_end=None):
        """-> dict(single float32, double, sum, expressing, positive, seconds) for the genes [gene_begin, gene_end)."""
        toc = np.ascontiguousarray(toc, dtype=np.uint64)
        data = np.ascontiguousarray(data, dtype=COUNT_DTYPE)
        gene_end = gene_count if gene_end is None else gene_end
        n = gene_end - gene_begin
        if norm_inverse is not None:
            norm_inverse = np.ascontiguousarray(norm_inverse, dtype=np.float64)
        out = {"single": np.zeros(n, np.float32), "double": np.zeros(n, np.float64), "sum": np.zeros(n, np.float64),
               "expressing": np.zeros(n, np.uint32), "positive": np.zeros(n, np.uint32)}
        seconds = c.c_double(0.)
        self.lib.em2r_gene_information_content(_ptr(toc), _ptr(data), len(toc) - 1, gene_begin, gene_end, _ptr(norm_inverse),
                                               _ptr(out["single"]), _ptr(out["double"]), _ptr(out["sum"]), _ptr(out["expressing"]),
                                               _ptr(out["positive"]), c.byref(seconds))
        out["seconds"] = seconds.value
        return out


@functools.lru_cache(maxsize=None)
def load():
    build = os.path.join(NATIVE_DIR, "build")
    os.makedirs(build, exist_ok=True)
    path = os.path.join(build, "libem2geneinformationrestatement.so")
    if not os.path.exists(path) or os.path.getmtime(path) < os.path.getmtime(SOURCE):
        tmp = path + ".%d.tmp" % os.getpid()
        cmd = ["g++", "-std=c++17", "-O2", "-msse4.2", "-ffp-contract=off", "-fPIC", "-shared", "-o", tmp, SOURCE]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError("gene information restatement build failed: " + r.stderr)
        os.replace(tmp, path)
    return GeneInformationRestatement(ctypes.CDLL(path))


# ---- inputs ----

def csr_of_columns(cell_count, columns):
    """columns: per gene (cells ascending, counts) -> (toc, data) of the cells' rows."""
    genes = np.concatenate([np.full(len(cells), g, dtype=np.uint32) for g, (cells, _) in enumerate(columns)] or [np.zeros(0, np.uint32)])
    cells = np.concatenate([np.asarray(cells, dtype=np.int64) for cells, _ in columns] or [np.zeros(0, np.int64)])
    counts = np.concatenate([np.asarray(v, dtype=np.float32) for _, v in columns] or [np.zeros(0, np.float32)])
    order = np.lexsort((genes, cells))
    toc = np.zeros(cell_count + 1, dtype=np.uint64)
    toc[1:] = np.cumsum(np.bincount(cells, minlength=cell_count))
    data = np.zeros(len(order), dtype=COUNT_DTYPE)
    data["gene"] = genes[order]
    data["count"] = counts[order]
    return toc, data


def random_matrix(cell_count, gene_count, density, seed):
    """Every (cell, gene) stored with probability `density`; counts a mix of small integers and non-integers."""
    rng = np.random.default_rng(seed)
    columns = []
    for g in range(gene_count):
        cells = np.nonzero(rng.random(cell_count) < density)[0]
        values = np.where(rng.random(len(cells)) < 0.5, rng.integers(1, 9, len(cells)).astype(np.float32),
                          rng.gamma(1.5, 2.0, len(cells)).astype(np.float32) + np.float32(0.01))
        columns.append((cells, values))
    return csr_of_columns(cell_count, columns)


def few_cells_many_genes(gene_count, cell_count, seed):
    """A handful of cells, each with 40 of the genes (gene_count - 1 among them in the last cell)."""
    rng = np.random.default_rng(seed)
    toc = np.arange(cell_count + 1, dtype=np.uint64) * 40
    data = np.zeros(cell_count * 40, dtype=COUNT_DTYPE)
    for cell in range(cell_count):
        genes = np.sort(rng.choice(gene_count - 1, 40, replace=False)).astype(np.uint32)
        if cell == cell_count - 1:
            genes[-1] = gene_count - 1
        data["gene"][cell * 40:(cell + 1) * 40] = genes
        data["count"][cell * 40:(cell + 1) * 40] = rng.integers(1, 20, 40)
    return toc, data


def segment_lengths(seed=5):
    """3 * CHUNK + 5 cells x 5 genes expressed in CHUNK - 1, CHUNK, CHUNK + 1, every and none of the cells."""
    rng = np.random.default_rng(seed)
    cells = 3 * CHUNK + 5
    columns = []
    for length in (CHUNK - 1, CHUNK, CHUNK + 1, cells, 0):
        where = np.sort(rng.choice(cells, length, replace=False))
        columns.append((where, rng.gamma(2.0, 1.5, length).astype(np.float32) + np.float32(0.05)))
    toc, data = csr_of_columns(cells, columns)
    return toc, data, 5


def one_gene_everywhere(seed=6):
    """70 000 cells x 3 genes: gene 0 in every cell (69 chunks), gene 1 in one cell, gene 2 in none."""
    rng = np.random.default_rng(seed)
    cells = 70000
    columns = [(np.arange(cells), rng.integers(1, 50, cells).astype(np.float32)), ([41234], [3.0]), ([], [])]
    toc, data = csr_of_columns(cells, columns)
    return toc, data, 3


def odd_content(seed=8):
    """300 cells x 12 genes of random data with: gene 0 in every cell; gene 3 with a stored zero in cell 10 (and positive entries); gene
    4 with stored zeros only; gene 5 with an inf count in cell 20; gene 6 expressed in one cell; gene 11 in none."""
    toc, data = random_matrix(300, 12, 0.3, seed)
    dense = np.zeros((300, 12), dtype=np.float32)
    stored = np.zeros((300, 12), dtype=bool)
    for cell in range(300):
        b, e = int(toc[cell]), int(toc[cell + 1])
        dense[cell, data["gene"][b:e]] = data["count"][b:e]
        stored[cell, data["gene"][b:e]] = True
    dense[~stored[:, 0], 0] = 1.5                      # gene 0 in every cell: no cell is empty
    stored[:, 0] = True
    stored[10, 3], dense[10, 3] = True, 0.0
    stored[:, 4] = False
    stored[[1, 2, 250], 4], dense[[1, 2, 250], 4] = True, 0.0
    stored[20, 5], dense[20, 5] = True, np.inf
    stored[:, 6] = False
    stored[150, 6], dense[150, 6] = True, 2.5
    stored[:, 11] = False
    columns = [(np.nonzero(stored[:, g])[0], dense[stored[:, g], g]) for g in range(12)]
    toc, data = csr_of_columns(300, columns)
    return toc, data, 12


def empty_cell(seed=9):
    """50 cells x 6 genes, cell 3 without an entry: under L1 / L2 its norm inverse is inf, and the reference's 0 * inf makes
    every gene with a positive entry NaN."""
    toc, data = random_matrix(50, 6, 0.4, seed)
    keep = np.ones(len(data), dtype=bool)
    keep[int(toc[3]):int(toc[4])] = False
    lengths = np.diff(toc.astype(np.int64))
    lengths[3] = 0
    new_toc = np.zeros(51, dtype=np.uint64)
    new_toc[1:] = np.cumsum(lengths)
    return new_toc, data[keep].copy(), 6


@functools.lru_cache(maxsize=None)
def case(name):
    """(toc, data, gene_count) of a named input; built once, never modified (the arrays are read-only)."""
    if name.startswith("random"):                       # random-<cells>x<genes>
        cells, genes = (int(x) for x in name.split("-")[1].split("x"))
        density = 1.0 if cells <= 2 else 0.25
        toc, data = random_matrix(cells, genes, density, seed=cells * 131 + genes)
        out = toc, data, genes
    elif name == "genes-65537":
        out = few_cells_many_genes(65537, 5, seed=3) + (65537,)
    else:
        out = {"segments": segment_lengths, "everywhere": one_gene_everywhere, "odd": odd_content, "empty-cell": empty_cell}[name]()
    for a in out[:2]:
        a.setflags(write=False)
    return out


SHAPE_CASES = ["random-1000x1", "random-2x2", "random-1x255", "random-1000x256", "random-1000x257", "random-300x600", "genes-65537",
               "segments", "everywhere"]
ALL_CASES = SHAPE_CASES + ["odd", "empty-cell"]


def norm_inverse_for(restatement, toc, data, method):
    """The restatement's norm inverses of the cells of the CSR itself (the CSR is the whole matrix here)."""
    if method == NONE:
        return None
    n1, n2 = restatement.cell_norm_inverses(toc, data)
    return n1 if method == L1 else n2


# ---- the yardstick ----

def higher_precision(toc, data, gene_count, norm_inverse=None):
    """R per gene: the reference's definition (src/ExpressionMatrix.cpp:1968-2018) with c the same floats, math.fsum for the sum
    and numpy.longdouble for p, the logarithms and the sum of the terms.  -> (R float64 [genes] (NaN where the definition gives
    NaN), n [genes] positive entries, weight [genes] = 1 + log2(N) + sum |p log2 p|)."""
    assert np.finfo(np.longdouble).nmant >= 63, "numpy.longdouble is no wider than double here"
    cells = len(toc) - 1
    rows = np.repeat(np.arange(cells), np.diff(toc.astype(np.int64)))
    factor = None if norm_inverse is None else np.asarray(norm_inverse, dtype=np.float64).astype(np.float32)
    with np.errstate(all="ignore"):
        value = data["count"] if factor is None else data["count"] * factor[rows]          # float32 products
        # a cell the gene is not stored in contributes 0 * factor: NaN where the factor is not finite
        poison = factor is not None and not np.all(np.isfinite(factor))
    order = np.argsort(data["gene"], kind="stable")
    bounds = np.searchsorted(data["gene"][order], np.arange(gene_count + 1))
    log_n = np.log(np.longdouble(cells))
    log_2 = np.log(np.longdouble(2))
    R = np.zeros(gene_count, dtype=np.float64)
    n = np.zeros(gene_count, dtype=np.int64)
    weight = np.zeros(gene_count, dtype=np.float64)
    for g in range(gene_count):
        v = value[order[bounds[g]:bounds[g + 1]]].astype(np.float64)
        positive = v[v > 0]
        n[g] = len(positive)
        if len(positive) == 0:
            R[g] = float(log_n / log_2)
            weight[g] = 1 + float(log_n / log_2)
            continue
        if poison or not np.all(np.isfinite(v)):
            R[g] = np.nan
            continue
        total = math.fsum(v.tolist())
        with np.errstate(all="ignore"):
            p = positive.astype(np.longdouble) / np.longdouble(total)
            terms = p * np.log(p)
            R[g] = float((log_n + np.sum(np.sort(terms))) / log_2)
            weight[g] = 1 + float(log_n / log_2) + float(np.sum(np.abs(terms)) / log_2)
    return R, n, weight


def bound(n, weight):
    """|I - R| <= 4 (n + 8) 2^-53 (1 + log2 N + sum |p log2 p|)."""
    return 4.0 * (n + 8) * 2.0 ** -53 * weight


def assert_within_bound(I, R, n, weight, what):
    I = np.asarray(I, dtype=np.float64)
    nan = np.isnan(R)
    assert np.array_equal(np.isnan(I), nan), what + ": NaN where R is not, or the reverse"
    error = np.abs(I[~nan] - R[~nan])
    limit = bound(n[~nan], weight[~nan])
    worst = np.argmax(error - limit) if len(error) else 0
    assert np.all(error <= limit), "%s: gene %d of the finite ones: |I - R| = %.3e > %.3e" % (what, worst, error[worst], limit[worst])
