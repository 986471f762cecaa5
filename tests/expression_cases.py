"""Random cases for the entries that read the expression counts themselves -- findSimilarPairs0, analyzeSimilarPairs,
analyzeLsh, createClusterGraph, findSimilarGenePairs0 and the gene information content -- shared by the parity sweep
(tools/fuzz_parity.py), tests/test_gpu_expression_sweep.py and tests/test_expression_cases_cpu.py.

Every entry of ENTRIES is a module-level object with
    draw(rng)            -> a case: a dict of plain numbers, strings and seeds that reproduces the inputs exactly
    cost(case)           -> an estimate of the CPU restatement's work, from the dict alone; a draw is run only below COST_CAP
    expect(case, r)      -> what the restatement (or the oracle, for analyze_lsh) gives; raises Discarded where the case reaches
                            a place the reference leaves open or asserts in (counted apart by the callers).  No GPU.
    check(case, r)       -> runs the device entry too: None, or a text naming the first difference; raises Discarded like expect,
                            after checking that the device entry answers such a case with the reference's text.
    reference()          -> the r to pass: the entry's C++ restatement, or the CPU oracle.
The comparisons are those of the entries' own test files: bit for bit (fsp0, gene_pairs, cluster_graph), both csv files byte for
byte (stored_pairs, analyze_lsh), gene_information_binding.assert_within_bound for the doubles of the information content and bit
for bit for the rest of it.  No tolerance is introduced here.

The lists the draws choose from hold the sizes at which the kernels change form: the wave (64) and block (256) sizes, the 1024
doubles of the cluster graph's chunks, the 128-gene tiles of the gene pairs, the block sizes of fsp0RowsKernel (12 000 and 30 000
genes) and the largest gene counts whose row vector still fits the LDS, with their successors.  The formulas of
csrc/em2_expression.h and csrc/em2_fsp0.hip that decide the form are restated below, for the draws and for the tests that assert
which forms a set of draws reaches."""
import os
import tempfile

import numpy as np

import cluster_graph_binding as cgb
import fsp0_binding
import gene_information_binding as gib
import gene_pairs_binding as gpb
import synth

COUNT_DTYPE = fsp0_binding.COUNT_DTYPE

CELL_COUNTS = [1, 2, 3, 63, 64, 65, 255, 256, 257, 600, 1025, 2100]
GENE_COUNTS = [1, 2, 31, 32, 33, 127, 128, 129, 1023, 1024, 1025, 2049, 12000, 30000]
K_VALUES = [0, 1, 2, 63, 64, 65, 100, "above", "exact", "below"]          # the last three: relative to the candidate count
THRESHOLDS = [-1.0, -0.5, 0.0, 0.1, 0.2, 0.9, 1.0]
COUNT_KINDS = ["integer", "non_integer", "wide"]
PLANTS = ["empty_cell", "constant_cell", "empty_gene", "stored_zero", "duplicate_cells", "duplicate_genes"]
PLANT_PROBABILITY = 0.08

SEEDS_PER_ENTRY = 8
CSV_LINE_COST = 150          # a line of the pairs' csv (four numbers through an ostream) against one step of the merge loop


class Discarded(Exception):
    """The case reaches a place the reference leaves open (a makeKnn tie, a NaN similarity) or asserts in (bin < binCount)."""


# ---- the formulas that decide a kernel's form ----

LDS_BYTES = 160 * 1024                      # kLdsBytes (csrc/em2_expression.h)
FSP0_MAX_THREADS = 1024                     # kMaxThreads (csrc/em2_fsp0.hip)
FSP0_MAX_SLOTS = 4096                       # kMaxSlots
ROW_SCRATCH_BLOCKS = 1024                   # kRowScratchBlocks
CLUSTER_CHUNK = 1024                        # kChunk (csrc/em2_cluster_graph.hip)
SELECT_LDS_ENTRIES = 8192                   # kSelectLdsEntries (csrc/em2_gene_pairs.hip)


def row_vector_bytes(genes):
    """rowVectorBytes: the floats, then the bitmap, each padded to 8 bytes."""
    return (genes * 4 + 7) // 8 * 8 + ((genes + 31) // 32 * 4 + 7) // 8 * 8


def slot_capacity(cells, k):
    """slotCapacityOf: min(k, cells - 1) rounded up to a power of two, at least 1."""
    needed = min(k, cells - 1) if cells else 0
    capacity = 1
    while capacity < needed:
        capacity <<= 1
    return capacity


def fsp0_own_lds_bytes(capacity):
    """fsp0Lds(capacity).totalBytes: the slots, the survivors of a batch, 32 words of state."""
    return capacity * 8 + FSP0_MAX_THREADS * 8 + 32 * 4


def largest_gene_count_in_lds(own_bytes=0):
    """The largest gene count whose row vector fits the LDS of a workgroup next to own_bytes of the kernel's own."""
    genes = (LDS_BYTES - own_bytes) // 4
    while row_vector_bytes(genes) + own_bytes > LDS_BYTES:
        genes -= 1
    assert row_vector_bytes(genes + 1) + own_bytes > LDS_BYTES
    return genes


def fsp0_form(cells, genes, k):
    """What runFsp0 launches: the row vector in LDS or not, the threads of a block, the column batches of a row."""
    capacity = slot_capacity(cells, k)
    own = fsp0_own_lds_bytes(capacity)
    in_lds = row_vector_bytes(genes) + own <= LDS_BYTES
    total = own + row_vector_bytes(genes)
    threads = 256 if not in_lds or total <= 40 * 1024 else 512 if total <= 80 * 1024 else FSP0_MAX_THREADS
    return {"in_lds": in_lds, "threads": threads, "batches": (cells + threads - 1) // threads, "slot_capacity": capacity,
            "supported": capacity <= FSP0_MAX_SLOTS}


def stored_pairs_in_lds(genes):
    """launchStoredPairs: the cut-over of fsp0 with one slot, although the kernel has no LDS of its own."""
    return row_vector_bytes(genes) + fsp0_own_lds_bytes(1) <= LDS_BYTES


FSP0_LIMIT_K1 = largest_gene_count_in_lds(fsp0_own_lds_bytes(1))
FSP0_LIMIT_K50 = largest_gene_count_in_lds(fsp0_own_lds_bytes(64))
ANALYZE_LSH_LIMIT = largest_gene_count_in_lds(0)
ROW_GENE_COUNTS = GENE_COUNTS + [FSP0_LIMIT_K1, FSP0_LIMIT_K1 + 1, FSP0_LIMIT_K50, FSP0_LIMIT_K50 + 1]
# analyzeSimilarPairs and analyzeLsh assert where a similarity is NaN or exactly 1 (bin < binCount).  One or two genes give
# nothing else, and so do cells of one or two entries (low densities of the small gene sets) and cells that one count
# dominates (the wide range): those draws would all be discarded, so the two entries draw without them.
ANALYSIS_GENE_COUNTS = [g for g in GENE_COUNTS if g > 2]
ANALYSIS_MATRIX = dict(small_densities=(0.25, 0.5), kinds=["integer", "non_integer"], plant_probability=0.03,
                       plants=["empty_cell", "constant_cell", "empty_gene", "stored_zero", "duplicate_cells"])


# ---- inputs ----

def choose(rng, values):
    value = values[int(rng.integers(len(values)))]
    return value if isinstance(value, str) else (float(value) if isinstance(value, float) else int(value))


def density_for(rng, genes, small=(0.03, 0.1, 0.25, 0.5)):
    """A few hundredths; up to 0.5 for small gene sets; a few thousandths for the large ones.  At 1023 genes and more the
    upper values give cells with more than 64 and more than 128 stored entries."""
    if genes >= 12000:
        return choose(rng, [0.001, 0.002, 0.004, 0.006])
    if genes >= 1023:
        return choose(rng, [0.01, 0.03, 0.08, 0.15])
    return choose(rng, list(small))


def k_value(rng, candidates, values=K_VALUES):
    k = choose(rng, values)
    return {"above": candidates + 5, "exact": candidates, "below": max(candidates - 1, 0)}.get(k, k)


def draw_matrix(rng, cell_counts=CELL_COUNTS, gene_counts=GENE_COUNTS, plants=PLANTS, plant_probability=PLANT_PROBABILITY,
                small_densities=(0.03, 0.1, 0.25, 0.5), kinds=COUNT_KINDS):
    genes = choose(rng, gene_counts)
    case = {"cells": choose(rng, cell_counts), "genes": genes, "density": density_for(rng, genes, small_densities),
            "clusters": choose(rng, [1, 3, 8]), "matrix_seed": int(rng.integers(1 << 30)), "counts": choose(rng, kinds)}
    case["plant"] = [name for name in plants if rng.random() < plant_probability]
    return case


def mean_entries(case):
    """Stored entries per cell, from the dict alone (synth.expression_matrix aims at density * genes, at least one)."""
    return max(1.0, case["density"] * case["genes"])


def csr_of(rows, genes, counts, cell_count):
    order = np.lexsort((genes, rows))
    toc = np.zeros(cell_count + 1, dtype=np.uint64)
    toc[1:] = np.cumsum(np.bincount(rows, minlength=cell_count))
    return toc, fsp0_binding.counts_of(genes[order].astype(np.uint32), counts[order].astype(np.float32))


def matrix(case):
    """(toc, data) of a case: synth.expression_matrix, the counts made non-integer / spread over 48 binary orders, then the
    planted oddities, each at places derived from matrix_seed:
      empty_cell       one cell without an entry
      constant_cell    one cell with the count 2.5 in every gene
      empty_gene       one gene without an entry (where a constant cell does not fill it)
      stored_zero      about every eleventh entry becomes a stored 0
      duplicate_cells  about every fourth cell repeats the cell before it
      duplicate_genes  about every fourth gene repeats the gene before it"""
    cells, genes, seed = case["cells"], case["genes"], case["matrix_seed"]
    toc, g, c = synth.expression_matrix(cells, genes, density=case["density"], cluster_count=case["clusters"], seed=seed)
    at = np.arange(len(c), dtype=np.uint64)
    if case["counts"] != "integer":
        c = (c.astype(np.float64) * (0.37 + synth.uniform01(seed, 77, at))).astype(np.float32)
    if case["counts"] == "wide":
        c = cgb.wide_range(fsp0_binding.counts_of(g, c), seed=seed % 1000)["count"]
    rows = np.repeat(np.arange(cells, dtype=np.int64), np.diff(toc.astype(np.int64)))
    g = g.astype(np.int64)
    plant = case["plant"]
    pick = lambda salt, n: int(synth.hash_u64(seed, salt, np.zeros(1, dtype=np.uint64))[0] % np.uint64(n))
    if "stored_zero" in plant:
        c = np.where(synth.hash_u64(seed, 81, at) % np.uint64(11) == 0, np.float32(0), c).astype(np.float32)
    if "duplicate_genes" in plant and genes > 1:
        odd = np.arange(1, genes, 2, dtype=np.uint64)
        repeated = np.zeros(genes + 1, dtype=bool)
        repeated[odd[synth.hash_u64(seed, 82, odd) % np.uint64(2) == 0]] = True
        keep = ~repeated[g]
        source = repeated[g + 1]                                  # entries of the gene before a repeated one
        rows, g, c = (np.concatenate([rows[keep], rows[source]]), np.concatenate([g[keep], g[source] + 1]),
                      np.concatenate([c[keep], c[source]]))
    if "duplicate_cells" in plant and cells > 1:
        odd = np.arange(1, cells, 2, dtype=np.uint64)
        repeated = np.zeros(cells + 1, dtype=bool)
        repeated[odd[synth.hash_u64(seed, 83, odd) % np.uint64(2) == 0]] = True
        keep = ~repeated[rows]
        source = repeated[rows + 1]
        rows, g, c = (np.concatenate([rows[keep], rows[source] + 1]), np.concatenate([g[keep], g[source]]),
                      np.concatenate([c[keep], c[source]]))
    if "empty_gene" in plant:
        keep = g != pick(84, genes)
        rows, g, c = rows[keep], g[keep], c[keep]
    if "constant_cell" in plant:
        cell = pick(85, cells)
        keep = rows != cell
        rows, g, c = (np.concatenate([rows[keep], np.full(genes, cell, dtype=np.int64)]),
                      np.concatenate([g[keep], np.arange(genes, dtype=np.int64)]),
                      np.concatenate([c[keep], np.full(genes, 2.5, dtype=np.float32)]))
    if "empty_cell" in plant:
        keep = rows != pick(86, cells)
        rows, g, c = rows[keep], g[keep], c[keep]
    return csr_of(rows, g, c, cells)


# Found by the sweep (analyze_lsh, seed 122): cell 0 has the same count in every gene, so it has no variance, and its numerator
# against cell 1 rounds away from 0: the exact similarity is +inf, not NaN.
INFINITE_SIMILARITY_CASE = {"cells": 3, "genes": 1025, "density": 0.03, "clusters": 3, "matrix_seed": 373992975, "counts": "non_integer",
                            "plant": ["constant_cell"], "lsh_count": 1, "seed": 719135, "downsample": 0.5}


def lds_limit_input(cells, genes, seed=3, non_integer=True):
    """A thin matrix (density 0.001) whose cells all end in one of the three highest genes: the last floats and the last bits of
    the row vector are in use -> (toc, data)."""
    toc, g, c = synth.expression_matrix(cells, genes, density=0.001, cluster_count=4, seed=seed)
    last = toc[1:].astype(np.int64) - 1
    g[last] = genes - 1 - np.arange(cells) % 3
    assert all((np.diff(g[int(toc[i]):int(toc[i + 1])].astype(np.int64)) > 0).all() for i in range(cells))
    if non_integer:
        c = (c.astype(np.float64) * (0.37 + synth.uniform01(seed, 77, np.arange(len(c), dtype=np.uint64)))).astype(np.float32)
    return toc, fsp0_binding.counts_of(g, c.astype(np.float32))


def first_difference(names, got, expected):
    """None, or which array differs first and at which rows."""
    for name, a, b in zip(names, got, expected):
        a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
        if a.shape != b.shape:
            return "%s: shape %s, expected %s" % (name, a.shape, b.shape)
        ua = a.view(np.uint32 if a.dtype.itemsize == 4 else np.uint64)
        ub = b.view(np.uint32 if b.dtype.itemsize == 4 else np.uint64)
        if not np.array_equal(ua, ub):
            different = (ua != ub).reshape(len(ua), -1).any(axis=1) if ua.ndim else np.array([True])
            where = np.nonzero(different)[0]
            r = int(where[0])
            return "%s differs in %d of %d rows, first %s; row %d: %s, expected %s" % (
                name, len(where), len(different), where[:12].tolist(), r, np.ravel(a[r])[:12].tolist(), np.ravel(b[r])[:12].tolist())
    return None


def read(path):
    with open(path, "rb") as f:
        return f.read()


def first_csv_difference(name, got, expected):
    if got == expected:
        return None
    a, b = got.split(b"\n"), expected.split(b"\n")
    for line, (x, y) in enumerate(zip(a, b)):
        if x != y:
            return "%s csv: line %d is %r, expected %r" % (name, line, x, y)
    return "%s csv: %d lines, expected %d" % (name, len(a), len(b))


def must_raise(call, text, what):
    """The device entry must answer with an error that holds `text`."""
    try:
        call()
    except RuntimeError as e:
        if text not in str(e):
            raise AssertionError("%s: the device entry raised %r, expected %r" % (what, str(e), text)) from None
        return
    raise AssertionError("%s: the device entry raised nothing, expected %r" % (what, text))


# ---- findSimilarPairs0 ----

def fsp0_device_rows(toc, data, genes, k, thr, begin, end):
    """capi.dev_find_similar_pairs0 for the rows [begin, end) with torch supplying the device memory and a workspace of exactly
    the size the library asks for; the outputs are filled with a non-zero pattern first.  -> the tuple of find_similar_pairs0."""
    import torch
    from expressionmatrix2_amd import capi
    toc = np.ascontiguousarray(toc, dtype=np.uint64)
    data = np.ascontiguousarray(data, dtype=COUNT_DTYPE)
    cells, rows = len(toc) - 1, end - begin
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()
    d_toc, d_data = d(toc), d(data) if len(data) else torch.zeros(8, dtype=torch.uint8, device="cuda")
    ws_bytes = capi.dev_find_similar_pairs0_workspace(cells, rows, genes, k)
    ws = torch.empty(max(ws_bytes, 8), dtype=torch.uint8, device="cuda")
    out_pairs = torch.full((max(rows * k, 1) * 8,), 0x5a, dtype=torch.uint8, device="cuda")
    out_used, out_index, out_low = (torch.full((max(rows, 1) * 4,), 0x5a, dtype=torch.uint8, device="cuda") for _ in range(3))
    capi.dev_find_similar_pairs0(d_toc.data_ptr(), d_data.data_ptr(), cells, genes, begin, end, k, thr, out_pairs.data_ptr(),
                                 out_used.data_ptr(), out_index.data_ptr(), out_low.data_ptr(), ws.data_ptr(), ws_bytes,
                                 torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return (out_pairs.cpu().numpy()[:rows * k * 8].view(capi.PAIR_DTYPE).reshape(rows, k), out_used.cpu().numpy()[:rows * 4].view(np.uint32),
            out_index.cpu().numpy()[:rows * 4].view(np.uint32), out_low.cpu().numpy()[:rows * 4].view(np.float32))


FSP0_NAMES = ("usedCount", "cell", "similarity", "lowestSimilarityIndex", "lowestSimilarity")


def fsp0_difference(device, expected):
    pairs, used, low_index, low = device
    cell, sim, e_used, e_low_index, e_low = expected
    return first_difference(FSP0_NAMES, (used, pairs["cell"], pairs["similarity"], low_index, low), (e_used, cell, sim, e_low_index, e_low))


class Fsp0:
    name = "fsp0"

    @staticmethod
    def reference():
        return fsp0_binding.load()

    @staticmethod
    def draw(rng):
        case = draw_matrix(rng, gene_counts=ROW_GENE_COUNTS, plants=[p for p in PLANTS if p != "duplicate_genes"])
        cells = case["cells"]
        case["k"] = k_value(rng, cells - 1)
        case["thr"] = choose(rng, THRESHOLDS)
        if case["genes"] > 30000:
            # one of the LDS limits: that of this draw's own slot capacity, or its successor
            beyond = int(case["genes"] in (FSP0_LIMIT_K1 + 1, FSP0_LIMIT_K50 + 1))
            case["genes"] = largest_gene_count_in_lds(fsp0_own_lds_bytes(slot_capacity(cells, case["k"]))) + beyond
        case["rows"] = None
        if rng.random() < 0.5:
            begin, end = sorted(int(x) for x in rng.integers(0, cells + 1, size=2))
            if begin == end:
                begin, end = (begin, begin + 1) if begin < cells else (begin - 1, begin)
            case["rows"] = [begin, end]
        return case

    @staticmethod
    def cost(case):
        """Pairs times mean entries per cell, the pairs those of the rows asked for; and, as SimilarPairs::add looks through the
        used slots at every offer, offers times a sixteenth of the slots (a comparison against a merge step)."""
        cells = case["cells"]
        pairs = cells * (cells - 1) / 2 if case["rows"] is None else (case["rows"][1] - case["rows"][0]) * (cells - 1)
        offers = pairs * (2 if case["rows"] is None else 1)
        return pairs * mean_entries(case) + offers * min(case["k"], max(cells - 1, 0)) / 16

    @staticmethod
    def expect(case, restatement):
        toc, data = matrix(case)
        rows = None if case["rows"] is None else tuple(case["rows"])
        return toc, data, restatement.find_similar_pairs0(toc, data, case["genes"], case["k"], case["thr"], rows=rows)

    @staticmethod
    def check(case, restatement):
        from expressionmatrix2_amd import capi
        toc, data, expected = Fsp0.expect(case, restatement)
        if case["rows"] is None:
            device = capi.find_similar_pairs0(toc, data, case["genes"], case["k"], case["thr"])
        else:
            device = fsp0_device_rows(toc, data, case["genes"], case["k"], case["thr"], *case["rows"])
        return fsp0_difference(device, expected)


# ---- analyzeSimilarPairs ----

def stored_object(case):
    """A synthetic stored object for the cells of a case: cell i stores used[i] <= k neighbours, none of them itself, with a
    made-up float similarity each -> (pairs [cells, k], usedCount)."""
    from expressionmatrix2_amd import capi
    cells, k, seed = case["cells"], case["k"], case["pairs_seed"]
    pairs = np.zeros((cells, k), dtype=capi.PAIR_DTYPE)
    i = np.arange(cells, dtype=np.uint64)[:, None]
    t = np.arange(k, dtype=np.uint64)[None, :]
    used = np.zeros(cells, dtype=np.uint32)
    if cells > 1:
        step = 1 + (t * np.uint64(7) + synth.hash_u64(seed, 1, i)) % np.uint64(cells - 1)            # 1 .. cells - 1: never the cell itself
        pairs["cell"] = ((i + step) % np.uint64(cells)).astype(np.uint32)
        pairs["similarity"] = (2. * synth.uniform01(seed, 2, i * np.uint64(k) + t) - 1.).astype(np.float32)
        used = (synth.hash_u64(seed, 3, i[:, 0]) % np.uint64(k + 1)).astype(np.uint32)
        used[synth.hash_u64(seed, 4, i[:, 0]) % np.uint64(4) == 0] = k                                # a quarter of the cells are full
    return pairs, used


class StoredPairs:
    name = "stored_pairs"

    @staticmethod
    def reference():
        return fsp0_binding.load()

    @staticmethod
    def draw(rng):
        case = draw_matrix(rng, gene_counts=ANALYSIS_GENE_COUNTS + [FSP0_LIMIT_K1, FSP0_LIMIT_K1 + 1], **ANALYSIS_MATRIX)
        case["k"] = choose(rng, [1, 2, 63, 64, 65, 100, 300])             # 300: more neighbours than the block has threads
        case["pairs_seed"] = int(rng.integers(1 << 30))
        case["downsample"] = choose(rng, [0.0, 0.01, 0.5, 1.0])
        return case

    @staticmethod
    def cost(case):
        """Stored pairs times mean entries per cell, a csv line taken as CSV_LINE_COST entries."""
        return case["cells"] * case["k"] * (mean_entries(case) + CSV_LINE_COST * case["downsample"])

    @staticmethod
    def _run(case, restatement, directory):
        toc, data = matrix(case)
        pairs, used = stored_object(case)
        ids = (np.arange(case["cells"], dtype=np.uint32) * 3 + 5).astype(np.uint32)
        rc = restatement.analyze_similar_pairs(toc, data, case["genes"], pairs["cell"], pairs["similarity"], used, ids, case["downsample"],
                                               os.path.join(directory, "r-pairs.csv"), os.path.join(directory, "r-stats.csv"))
        assert rc in (0, 1), "the restatement could not write its files"
        return toc, data, pairs, used, ids, rc

    @staticmethod
    def expect(case, restatement):
        with tempfile.TemporaryDirectory() as directory:
            rc = StoredPairs._run(case, restatement, directory)[-1]
            if rc == 1:
                raise Discarded("bin < binCount")
            return read(os.path.join(directory, "r-pairs.csv")), read(os.path.join(directory, "r-stats.csv"))

    @staticmethod
    def check(case, restatement):
        from expressionmatrix2_amd import capi
        with tempfile.TemporaryDirectory() as directory:
            toc, data, pairs, used, ids, rc = StoredPairs._run(case, restatement, directory)
            call = lambda: capi.analyze_similar_pairs(toc, data, case["genes"], pairs, used, ids, case["downsample"],
                                                      os.path.join(directory, "d-pairs.csv"), os.path.join(directory, "d-stats.csv"))
            if rc == 1:
                must_raise(call, "bin < binCount", "stored_pairs %r" % case)
                raise Discarded("bin < binCount")
            call()
            for name in ("pairs", "stats"):
                difference = first_csv_difference(name, read(os.path.join(directory, "d-%s.csv" % name)),
                                                  read(os.path.join(directory, "r-%s.csv" % name)))
                if difference:
                    return difference
        return None


# ---- analyzeLsh ----

class AnalyzeLsh:
    name = "analyze_lsh"

    @staticmethod
    def reference():
        import oracle_binding
        return oracle_binding.load_oracle()

    @staticmethod
    def draw(rng):
        case = draw_matrix(rng, cell_counts=[c for c in CELL_COUNTS if c > 1],
                           gene_counts=ANALYSIS_GENE_COUNTS + [ANALYZE_LSH_LIMIT, ANALYZE_LSH_LIMIT + 1], **ANALYSIS_MATRIX)
        case["lsh_count"] = choose(rng, [1, 64, 100, 192])
        case["seed"] = int(rng.integers(1 << 20))
        case["downsample"] = choose(rng, [0.0, 0.01, 0.5, 1.0])
        return case

    @staticmethod
    def cost(case):
        """Pairs times mean entries per cell, a csv line taken as CSV_LINE_COST entries."""
        return case["cells"] * (case["cells"] - 1) / 2 * (mean_entries(case) + CSV_LINE_COST * case["downsample"])

    @staticmethod
    def _run(case, oracle, directory):
        toc, data = matrix(case)
        genes, L = case["genes"], case["lsh_count"]
        g, c = np.ascontiguousarray(data["gene"]), np.ascontiguousarray(data["count"])
        vectors = oracle.generate_lsh_vectors(genes, L, case["seed"])
        sig = oracle.compute_signatures(toc, g, c, genes, vectors, L)
        ids = (np.arange(case["cells"], dtype=np.uint32) * 3 + 5).astype(np.uint32)
        o = oracle.analyze_lsh(toc, g, c, genes, sig, L, ids, case["seed"], case["downsample"], os.path.join(directory, "o-pairs.csv"),
                               os.path.join(directory, "o-stats.csv"))
        return toc, data, sig, ids, o

    @staticmethod
    def expect(case, oracle):
        with tempfile.TemporaryDirectory() as directory:
            o = AnalyzeLsh._run(case, oracle, directory)[-1]
            if o is None:
                raise Discarded("bin < binCount")
            return o, read(os.path.join(directory, "o-pairs.csv")), read(os.path.join(directory, "o-stats.csv"))

    @staticmethod
    def check(case, oracle):
        from expressionmatrix2_amd import capi
        with tempfile.TemporaryDirectory() as directory:
            toc, data, sig, ids, o = AnalyzeLsh._run(case, oracle, directory)
            call = lambda: capi.analyze_lsh(toc, data, case["genes"], sig, case["lsh_count"], ids, case["seed"], case["downsample"],
                                            os.path.join(directory, "d-pairs.csv"), os.path.join(directory, "d-stats.csv"), per_pair=True)
            if o is None:
                must_raise(call, "bin < binCount", "analyze_lsh %r" % case)
                raise Discarded("bin < binCount")
            d = call()
            pairs = len(d["exact"])
            names = ("exact", "lsh", "sum0", "sum1", "sum2")
            difference = first_difference(names, [d[n] for n in names], [o[n][:pairs] if n in ("exact", "lsh") else o[n] for n in names])
            if difference:
                return difference
            for name in ("pairs", "stats"):
                difference = first_csv_difference(name, read(os.path.join(directory, "d-%s.csv" % name)),
                                                  read(os.path.join(directory, "o-%s.csv" % name)))
                if difference:
                    return difference
        return None


# ---- createClusterGraph ----

def cluster_inputs(case):
    """-> (cgb.Case, cells of arbitrary lists, their offsets, edge0, edge1): planted clusters of very unequal size (each half the
    one before), some of them under two labels, the vertices in a hashed order; and for the two smaller entry points cell lists
    that are not ascending, name a cell twice and share cells, with edges between arbitrary lists."""
    cells, genes, seed = case["cells"], case["genes"], case["matrix_seed"]
    count = min(case["clusters"], cells)
    weights = 0.5 ** np.arange(count)
    sizes = np.maximum(1, np.floor(weights / weights.sum() * cells)).astype(np.int64)
    sizes[0] += cells - sizes.sum()
    assert sizes.min() >= 1
    # every second cluster is a relative of cluster 0 (similar averages: the merge and makeKnn have something to decide)
    spec = [(int(size), 0 if i % 2 else i, 0.25 + 0.05 * (i % 5)) for i, size in enumerate(sizes)]
    toc, data, owner = cgb.planted(spec, genes, case["density"], seed=seed % 100000, non_integer=case["counts"] != "integer",
                                   noise=case["noise"])
    if case["counts"] == "wide":
        data = cgb.wide_range(data, seed=seed % 1000)
    n = len(owner)
    piece = (synth.hash_u64(seed, 43, np.arange(n, dtype=np.uint64)) % np.uint64(5)).astype(np.uint32)
    labels = (owner * 5 + np.where(piece < case["split"], 0, piece)).astype(np.uint32)          # split 5: one label per cluster
    toc, data, labels = cgb.shuffled(toc, data, labels, seed=seed % 997)
    ids = sorted(set(labels.tolist()))
    pairs = [(a, b) for i, a in enumerate(ids) for b in ids[i + 1:] if (a + b + seed) % 4]
    v0, v1 = cgb.edges_between(labels, pairs, seed=seed % 991)
    rows = None
    if case["vertex_rows"]:
        # the CSR starts with three rows no vertex uses and holds the vertices' rows in reverse
        extra_toc, extra_data, _ = cgb.planted([(3, 0, 0.)], genes, case["density"], seed=27)
        pieces = [data[int(toc[c]):int(toc[c + 1])] for c in range(n - 1, -1, -1)]
        lengths = np.diff(toc.astype(np.int64))[::-1]
        toc = np.concatenate([extra_toc, extra_toc[-1] + np.cumsum(lengths).astype(np.uint64)])
        data = np.concatenate([extra_data] + pieces)
        rows = (3 + n - 1 - np.arange(n)).astype(np.uint32)
    graph = cgb.Case(toc, data, genes, labels, v0, v1, vertex_rows=rows, min_cluster_size=case["min_cluster_size"], k=case["k"],
                     similarity_threshold=case["thr"], similarity_threshold_for_merge=case["merge_thr"])
    total = len(toc) - 1
    order = cgb.interleave(np.zeros(total), seed=seed % 983)
    a = max(1, total * 3 // 5)
    lists = [order[:a], order[:1], np.array([order[0], order[0], order[-1]], dtype=np.uint32), np.arange(total - 1, -1, -1, dtype=np.uint32)[:max(1, total // 2)]]
    list_cells = np.concatenate(lists).astype(np.uint32)
    offsets = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.uint64)
    e0, e1 = np.array([0, 0, 3, 2, 1, 3], dtype=np.uint32), np.array([1, 3, 2, 0, 3, 0], dtype=np.uint32)
    return graph, list_cells, offsets, e0, e1


class ClusterGraph:
    name = "cluster_graph"

    @staticmethod
    def reference():
        return cgb.load()

    @staticmethod
    def draw(rng):
        genes = choose(rng, [2, 31, 32, 33, 127, 128, 129, 1023, 1024, 1025, 2049])
        case = {"cells": choose(rng, [3, 63, 64, 65, 255, 256, 257, 600, 1025, 2100]), "genes": genes,
                "density": choose(rng, [0.08, 0.15] if genes >= 1023 else [0.1, 0.25, 0.5]), "clusters": choose(rng, [1, 2, 3, 5, 8]),
                "matrix_seed": int(rng.integers(1 << 30)), "counts": choose(rng, COUNT_KINDS), "noise": choose(rng, [0.2, 0.35]),
                "split": choose(rng, [3, 5, 5])}
        case["min_cluster_size"] = choose(rng, [1, 2, 5, 20, 100])
        case["k"] = choose(rng, [1, 2, 3, 100])
        case["thr"] = choose(rng, [-1.0, 0.0, 0.2, 0.5])
        case["merge_thr"] = choose(rng, [0.5, 0.75, 0.9, 2.0])
        case["vertex_rows"] = bool(rng.random() < 0.5)
        return case

    @staticmethod
    def cost(case):
        """The planted input is built gene by gene for every cell: cells times genes."""
        return case["cells"] * case["genes"]

    @staticmethod
    def _expect(case, restatement):
        graph, list_cells, offsets, e0, e1 = cluster_inputs(case)
        try:
            expected = restatement.create(*graph.arguments(), **graph.parameters)
        except cgb.NanSimilarity:
            return graph, None, None
        averages = restatement.average_expression(graph.toc, graph.data, graph.genes, list_cells, offsets)
        similarity = restatement.similarities(averages, e0, e1)
        return graph, expected, (list_cells, offsets, e0, e1, averages, similarity)

    @staticmethod
    def expect(case, restatement):
        graph, expected, lists = ClusterGraph._expect(case, restatement)
        if expected is None:
            raise Discarded("NaN similarity")
        try:
            cgb.assert_parity_case(expected)
        except AssertionError:
            raise Discarded("makeKnn tie" if expected["knnTie"] else "NaN edge similarity") from None
        return expected, lists

    @staticmethod
    def check(case, restatement):
        from expressionmatrix2_amd import capi
        graph, expected, lists = ClusterGraph._expect(case, restatement)
        if expected is None:
            must_raise(lambda: capi.cluster_graph_create(*graph.arguments(), **graph.parameters), "NaN", "cluster_graph %r" % case)
            raise Discarded("NaN similarity")
        try:
            cgb.assert_parity_case(expected)
        except AssertionError:
            raise Discarded("makeKnn tie" if expected["knnTie"] else "NaN edge similarity") from None
        got = capi.cluster_graph_create(*graph.arguments(), **graph.parameters)
        difference = first_difference(cgb.RESULT_KEYS, [got[key] for key in cgb.RESULT_KEYS], [expected[key] for key in cgb.RESULT_KEYS])
        if difference:
            return difference
        list_cells, offsets, e0, e1, averages, similarity = lists
        got_averages = capi.cluster_average_expression(graph.toc, graph.data, graph.genes, list_cells, offsets)
        difference = first_difference(("averages of arbitrary lists",), (got_averages,), (averages,))
        if difference:
            return difference
        return first_difference(("similarities of arbitrary lists",), (capi.cluster_similarities(averages, e0, e1),), (similarity,))


# ---- findSimilarGenePairs0 ----

class GenePairs:
    name = "gene_pairs"

    @staticmethod
    def reference():
        return gpb.load()

    @staticmethod
    def draw(rng):
        case = draw_matrix(rng, cell_counts=[1, 2, 3, 15, 16, 17, 63, 64, 65, 255, 256, 257, 600, 1025, 2100],
                           gene_counts=[g for g in GENE_COUNTS if g <= 2049], plants=PLANTS)
        case["method"] = choose(rng, [gpb.NONE, gpb.L1, gpb.L2])
        case["k"] = k_value(rng, case["genes"] - 1)
        case["thr"] = choose(rng, THRESHOLDS)
        case["buffer_mb"] = choose(rng, ["", "", "0", "1"])                # EM2_GENE_PAIRS_BUFFER_MB: unset, "0", "1"
        return case

    @staticmethod
    def cost(case):
        """Gene pairs times cells."""
        return case["genes"] * (case["genes"] - 1) / 2 * case["cells"]

    @staticmethod
    def expect(case, restatement):
        toc, data = matrix(case)
        return toc, data, restatement.find_similar_gene_pairs0(toc, data, case["genes"], case["method"], case["k"], case["thr"], True)

    @staticmethod
    def check(case, restatement):
        from expressionmatrix2_amd import capi
        toc, data, (gene, sim, used, r) = GenePairs.expect(case, restatement)
        saved = os.environ.get("EM2_GENE_PAIRS_BUFFER_MB")
        try:
            os.environ.pop("EM2_GENE_PAIRS_BUFFER_MB", None)
            if case["buffer_mb"]:
                os.environ["EM2_GENE_PAIRS_BUFFER_MB"] = case["buffer_mb"]
            pairs, d_used, d_r = capi.find_similar_gene_pairs0(toc, data, case["genes"], case["method"], case["k"], case["thr"], True)
        finally:
            os.environ.pop("EM2_GENE_PAIRS_BUFFER_MB", None)
            if saved is not None:
                os.environ["EM2_GENE_PAIRS_BUFFER_MB"] = saved
            capi.apply_gene_pairs_buffer()
        return first_difference(("usedCount", "gene", "similarity", "allSimilarities"), (d_used, pairs["cell"], pairs["similarity"], d_r),
                                (used, gene, sim, r))


# ---- gene information content ----

class GeneInformation:
    name = "gene_information"

    @staticmethod
    def reference():
        return gib.load()

    @staticmethod
    def draw(rng):
        case = draw_matrix(rng, plants=[p for p in PLANTS if p != "duplicate_genes"])
        case["method"] = choose(rng, [gib.NONE, gib.L1, gib.L2])
        case["max_blocks"] = choose(rng, [0, 2])
        return case

    @staticmethod
    def cost(case):
        """The higher-precision statement walks the genes one by one in Python: genes, and a hundredth of the entries."""
        return case["genes"] + case["cells"] * mean_entries(case) / 100

    @staticmethod
    def expect(case, restatement):
        toc, data = matrix(case)
        norm = gib.norm_inverse_for(restatement, toc, data, case["method"])
        R, n, weight = gib.higher_precision(toc, data, case["genes"], norm)
        return toc, data, norm, (R, n, weight), restatement.gene_information_content(toc, data, case["genes"], norm)

    @staticmethod
    def check(case, restatement):
        from expressionmatrix2_amd import capi
        toc, data, norm, (R, n, weight), theirs = GeneInformation.expect(case, restatement)
        genes = case["genes"]
        capi.load().em2_set_gene_information_max_blocks(case["max_blocks"])
        try:
            single, double, expressing = capi.gene_information_content(toc, data, genes, norm)
        finally:
            capi.load().em2_set_gene_information_max_blocks(0)
        try:
            gib.assert_within_bound(double, R, n, weight, "the doubles")
        except AssertionError as e:
            return str(e)
        none = theirs["positive"] == 0
        return first_difference(
            ("the floats as roundings of the doubles", "expressingCellCount", "expressingCellCount against the restatement",
             "floats of genes without a positive entry", "doubles of genes without a positive entry", "NaN floats"),
            (single, expressing, expressing, single[none], double[none], np.isnan(single).astype(np.uint32)),
            (double.astype(np.float32), np.bincount(data["gene"], minlength=genes).astype(np.uint32), theirs["expressing"],
             theirs["single"][none], theirs["double"][none], np.isnan(theirs["single"]).astype(np.uint32)))


def forms(name, case):
    """The kernel forms and input kinds a case reaches, as a set of words: from the dict and the formulas above, and the longest
    cell from the matrix itself."""
    out = set()
    cells, genes = case["cells"], case["genes"]
    if name != "cluster_graph":
        toc = matrix(case)[0]
        longest = int(np.diff(toc.astype(np.int64)).max())
        out.update("planted " + p for p in case["plant"])
        out.add("counts " + case["counts"])
    else:
        longest = int(np.diff(cluster_inputs(case)[0].toc.astype(np.int64)).max())
    if longest > 64:
        out.add("a cell with more than 64 entries")
    if longest > 128:
        out.add("a cell with more than 128 entries")
    if name == "fsp0":
        form = fsp0_form(cells, genes, case["k"])
        out.add("row vector in LDS" if form["in_lds"] else "row vector in global memory")
        if form["in_lds"]:
            out.add("%d threads" % form["threads"])
            if form["batches"] > 1:
                out.add("%d threads, several batches" % form["threads"])
        elif cells > ROW_SCRATCH_BLOCKS:
            out.add("more rows than blocks")
        out.add("ranged" if case["rows"] else "all rows")
        if case["k"] > cells - 1:
            out.add("k above the candidate count")
        if case["k"] == cells - 1:
            out.add("k the candidate count")
        if 0 < case["k"] < cells - 1 and case["thr"] <= 0.0:
            out.add("evictions")
        if form["slot_capacity"] > 128:
            out.add("more than 128 slots")
        own = fsp0_own_lds_bytes(form["slot_capacity"])
        if genes - largest_gene_count_in_lds(own) in (0, 1):
            out.add("at the LDS limit")
    if name == "stored_pairs":
        out.add("row vector in LDS" if stored_pairs_in_lds(genes) else "row vector in global memory")
        if case["k"] > 256:
            out.add("more neighbours than threads")
        if genes in (FSP0_LIMIT_K1, FSP0_LIMIT_K1 + 1):
            out.add("at the LDS limit")
    if name == "analyze_lsh":
        out.add("row vector in LDS" if genes <= ANALYZE_LSH_LIMIT else "row vector in global memory")
        if genes in (ANALYZE_LSH_LIMIT, ANALYZE_LSH_LIMIT + 1):
            out.add("at the LDS limit")
        if cells - 1 > ROW_SCRATCH_BLOCKS and genes > ANALYZE_LSH_LIMIT:
            out.add("more rows than blocks")
    if name == "cluster_graph":
        out.add("one chunk of genes" if genes <= CLUSTER_CHUNK else "several chunks of genes")
        if genes == CLUSTER_CHUNK:
            out.add("exactly one chunk of genes")
        out.add("vertex rows" if case["vertex_rows"] else "no vertex rows")
        out.add("counts " + case["counts"])
    if name == "gene_pairs":
        out.add("method %d" % case["method"])
        out.add("buffer %s" % (case["buffer_mb"] or "unset"))
        out.add("several tiles" if genes > 128 else "one tile")
        if case["k"] >= genes - 1:
            out.add("k at or above the candidate count")
        if 0 < case["k"] < genes - 1 and case["thr"] <= 0.0:
            out.add("selection")
    if name == "gene_information":
        out.add("method %d" % case["method"])
        out.add("max blocks %d" % case["max_blocks"])
        if genes > 256:
            out.add("more than 256 genes")
    return out


# What the eight fixed draws of an entry must reach between them (tests/test_expression_cases_cpu.py).
REQUIRED_FORMS = {
    "fsp0": ["row vector in LDS", "row vector in global memory", "256 threads", "512 threads", "1024 threads", "ranged", "all rows",
             "k above the candidate count", "evictions", "planted duplicate_cells", "a cell with more than 128 entries"],
    "stored_pairs": ["row vector in LDS", "row vector in global memory", "more neighbours than threads", "a cell with more than 128 entries"],
    "analyze_lsh": ["row vector in LDS", "row vector in global memory", "a cell with more than 128 entries"],
    "cluster_graph": ["one chunk of genes", "several chunks of genes", "vertex rows", "no vertex rows", "counts wide",
                      "a cell with more than 128 entries"],
    "gene_pairs": ["method 0", "method 1", "method 2", "buffer unset", "buffer 0", "buffer 1", "several tiles",
                   "k at or above the candidate count", "selection", "planted duplicate_genes"],
    "gene_information": ["method 0", "method 1", "method 2", "max blocks 0", "max blocks 2", "a cell with more than 128 entries",
                         "more than 256 genes"],
}


ENTRIES = {entry.name: entry for entry in (Fsp0, StoredPairs, AnalyzeLsh, ClusterGraph, GenePairs, GeneInformation)}

# The cap of cost(case) per entry, chosen so that the slowest restatement of a fixed draw stays at about 2 s on one CPU thread
# (measured; see tests/test_gpu_expression_sweep.py).
COST_CAP = {"fsp0": 1.3e8, "stored_pairs": 1.3e8, "analyze_lsh": 1.3e8, "cluster_graph": 5e6, "gene_pairs": 5e8,
            "gene_information": 4e4}

# The seeds of the fixed draws of tests/test_gpu_expression_sweep.py, a draw being draw(rng_of(entry, seed)): eight of the seeds
# 1 .. 200 per entry, picked (greedily, lowest seed first among equals) so that between them the eight reach every form of
# REQUIRED_FORMS and every other word forms() has for the runnable draws of those 200 seeds.
FIXED_SEEDS = {
    "fsp0": [1, 2, 3, 11, 13, 27, 86, 197],
    "stored_pairs": [1, 2, 4, 5, 12, 67, 112, 162],
    "analyze_lsh": [2, 4, 5, 6, 7, 10, 22, 32],
    "cluster_graph": [1, 2, 3, 4, 5, 6, 17, 27],
    "gene_pairs": [1, 2, 3, 4, 23, 61, 75, 98],
    "gene_information": [1, 2, 3, 4, 5, 6, 19, 54],
}
assert all(len(seeds) == SEEDS_PER_ENTRY for seeds in FIXED_SEEDS.values())
SWEEP_DRAWS = 200           # the draws of an entry that tests/test_expression_cases_cpu.py counts the skipped ones of: seeds 1 .. 200


def rng_of(name, seed):
    return np.random.default_rng([sorted(ENTRIES).index(name), int(seed)])


def fixed_draws(name):
    return [ENTRIES[name].draw(rng_of(name, seed)) for seed in FIXED_SEEDS[name]]


def runnable(name, case):
    return ENTRIES[name].cost(case) < COST_CAP[name]
