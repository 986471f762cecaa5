"""findSimilarPairs0 / analyzeSimilarPairs without a GPU: the C++ restatement the device is compared with
(tests/native/em2_fsp0_restatement.cpp) is itself checked against independent statements -- the oracle's analyzeLsh for
the per-pair similarity, a pure-Python SimilarPairs::add for the selection, numpy.corrcoef on ToyTest1 -- and the host-only
methods (computeCellSimilarity, compareSimilarPairs) against it."""
import os

import numpy as np
import pytest

import fsp0_binding
import synth
import toytest1
from expressionmatrix2_amd import ExpressionMatrix, capi, files

FLT_MAX = np.float32(3.4028234663852886e38)
INVALID = 0xFFFFFFFF


@pytest.fixture(scope="module")
def restatement():
    return fsp0_binding.load()


def python_slot_machine(exact, cell_count, k, thr):
    """SimilarPairs::add (src/SimilarPairs.cpp:170-232) and sort (:399-405), written from those lines alone, over the
    candidates of findSimilarPairs0's loop (src/ExpressionMatrixFindSimilarPairs.cpp:60-76): unordered pairs in order,
    each survivor offered to cell 0 and then to cell 1."""
    slots = [[] for _ in range(cell_count)]
    low_index = [INVALID] * cell_count
    low = [FLT_MAX] * cell_count

    def add(c, other, s):
        mine = slots[c]
        if len(mine) < k:
            if any(o == other for o, _ in mine):
                return
            if s < low[c]:
                low_index[c], low[c] = len(mine), s
            mine.append((other, s))
            return
        if s <= low[c]:
            return
        if any(o == other for o, _ in mine):
            return
        mine[low_index[c]] = (other, s)
        low_index[c], low[c] = INVALID, FLT_MAX
        for i, (_, value) in enumerate(mine):
            if value < low[c]:
                low_index[c], low[c] = i, value

    at = 0
    for c0 in range(cell_count - 1):
        for c1 in range(c0 + 1, cell_count):
            s = exact[at]
            at += 1
            if s > thr:
                add(c0, c1, np.float32(s))
                add(c1, c0, np.float32(s))
    cell = np.zeros((cell_count, k), dtype=np.uint32)
    sim = np.zeros((cell_count, k), dtype=np.float32)
    used = np.zeros(cell_count, dtype=np.uint32)
    for c in range(cell_count):
        ordered = sorted(slots[c], key=lambda p: (-p[1], p[0]))
        used[c] = len(ordered)
        for i, (o, s) in enumerate(ordered):
            cell[c, i], sim[c, i] = o, s
    return cell, sim, used, np.array(low_index, dtype=np.uint32), np.array(low, dtype=np.float32)


def same_result(a, b):
    return all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(a, b))


@pytest.mark.parametrize("cells,genes,density,seed,non_integer", [
    (90, 400, 0.05, 3, False),
    (120, 700, 0.03, 8, True),
    (64, 50, 0.3, 21, True),
])
def test_pair_similarity_equals_the_oracles_analyze_lsh(restatement, oracle, tmp_path, cells, genes, density, seed, non_integer):
    toc, data = fsp0_binding.clustered(cells, genes, density, seed=seed, cluster_count=4, non_integer=non_integer)
    assert (np.diff(toc.astype(np.int64)) >= 2).all()
    L = 64
    vectors = oracle.generate_lsh_vectors(genes, L, 1)
    sig = oracle.compute_signatures(toc, data["gene"], data["count"], genes, vectors, L)
    o = oracle.analyze_lsh(toc, data["gene"], data["count"], genes, sig, L, np.arange(cells, dtype=np.uint32), 1, 0.,
                           str(tmp_path / "p.csv"), str(tmp_path / "s.csv"))
    assert o is not None                                       # (no duplicate cells, every cell with variance)
    exact = restatement.pair_similarities(toc, data, genes)
    assert np.array_equal(exact.view(np.uint64), o["exact"][:len(exact)].view(np.uint64))
    assert restatement.cell_similarity(toc, data, genes, 3, 17) == exact[3 * (cells - 1) - 3 * 2 // 2 + (17 - 3 - 1)]


@pytest.mark.parametrize("k,thr", [(3, -1.0), (4, 0.0), (5, 0.05), (1, 0.3), (200, 0.2), (0, 0.2)])
def test_selection_equals_a_python_slot_machine_on_tied_input(restatement, k, thr):
    toc, data, genes = fsp0_binding.duplicated_cells_input()
    n = len(toc) - 1
    exact = restatement.pair_similarities(toc, data, genes)
    assert same_result(restatement.find_similar_pairs0(toc, data, genes, k, thr), python_slot_machine(exact, n, k, thr))


def test_selection_equals_a_python_slot_machine_on_clustered_input(restatement):
    toc, data = fsp0_binding.clustered(150, 500, 0.05, seed=5, cluster_count=5, non_integer=True)
    exact = restatement.pair_similarities(toc, data, 500)
    for k, thr in [(10, 0.2), (7, -0.5)]:
        assert same_result(restatement.find_similar_pairs0(toc, data, 500, k, thr), python_slot_machine(exact, 150, k, thr))


def ranged_equals_slice(restatement, toc, data, genes, k, thr, ranges):
    full = restatement.find_similar_pairs0(toc, data, genes, k, thr)
    for begin, end in ranges:
        ranged = restatement.find_similar_pairs0(toc, data, genes, k, thr, rows=(begin, end))
        assert all(len(a) == end - begin for a in ranged)
        assert same_result(ranged, tuple(a[begin:end] for a in full)), (k, thr, begin, end)
    return full


@pytest.mark.parametrize("k,thr", [(3, -1.0), (4, 0.0), (5, 0.05), (1, 0.3), (200, 0.2), (0, 0.2)])
def test_ranged_restatement_equals_the_slice_of_a_full_run_on_tied_input(restatement, k, thr):
    """The row range of the restatement (every row from its own candidates in ascending id of the other cell) against the
    reference's loop over the unordered pairs, where ties make the order of the offers decide: the whole range, single rows
    at both ends, an empty range and ranges inside."""
    toc, data, genes = fsp0_binding.duplicated_cells_input()
    n = len(toc) - 1
    ranged_equals_slice(restatement, toc, data, genes, k, thr, [(0, n), (0, 1), (n - 1, n), (40, 40), (17, 93), (n - 8, n)])


def test_ranged_restatement_equals_the_slice_of_a_full_run_with_evictions(restatement):
    """Clustered non-integer input whose rows fill and then evict (k = 7 of 299 candidates at threshold -1), and an input
    with an empty cell (NaN similarities, never stored) and a cell without variance."""
    toc, data = fsp0_binding.clustered(300, 400, 0.06, seed=15, cluster_count=5, non_integer=True)
    full = ranged_equals_slice(restatement, toc, data, 400, 7, -1.0, [(0, 300), (0, 8), (292, 300), (100, 101)])
    assert (full[2] == 7).all()
    toc2, data2 = fsp0_binding.repeat_cells(toc, data, [1] * 20)
    flat = fsp0_binding.counts_of(np.arange(400, dtype=np.uint32), np.full(400, 1.5, dtype=np.float32))
    toc2 = np.concatenate([toc2, toc2[-1:], toc2[-1:] + np.uint64(400)])         # cell 20 empty, cell 21 constant
    data2 = np.concatenate([data2, flat])
    full = ranged_equals_slice(restatement, toc2, data2, 400, 5, 0.0, [(0, 22), (19, 22), (20, 21)])
    assert full[2][20] == 0                                   # (the constant cell's similarities are NaN or +-inf, as IEEE has it)
    with pytest.raises(ValueError):
        restatement.find_similar_pairs0(toc2, data2, 400, 5, 0.0, rows=(3, 23))


def test_tie_input_is_not_a_plain_top_k(restatement):
    """On the duplicated-cells input the slot machine's result is NOT 'the k best by (similarity desc, id asc)': which of
    several tied entries is evicted depends on the slots' history.  Otherwise the GPU tie cases would prove nothing."""
    toc, data, genes = fsp0_binding.duplicated_cells_input()
    n = len(toc) - 1
    exact = restatement.pair_similarities(toc, data, genes)
    for k, thr in [(3, -1.0), (4, 0.0), (5, 0.05)]:
        cell, sim, used, _, _ = restatement.find_similar_pairs0(toc, data, genes, k, thr)
        top_cell, top_sim, top_used = fsp0_binding.best_k_by_similarity_then_id(exact, n, k, thr)
        differing = [c for c in range(n) if not np.array_equal(cell[c], top_cell[c])]
        assert len(differing) >= 1, (k, thr)
        assert np.array_equal(used, top_used)                    # (the counts agree: only the choice among ties differs)
        assert (used == k).sum() > n // 2                        # (and most cells are full, so evictions happen)


def test_toytest1_matches_corrcoef(restatement):
    """ToyTest1 (3 cells x 3 genes), defaults k=100, threshold 0.2, against numpy.corrcoef of the dense matrix.
    Tolerance: both sides evaluate the same correlation coefficient in doubles by different formulas; with counts below
    2^5 and 3 genes every sum and product up to numerator and the two variance factors is exact in a double (integers
    below 2^53) on the restatement's side, which leaves its square root, its division and the float conversion: relative
    error <= 2 * 2^-53 + 2^-24.  corrcoef's centred formula rounds about ten times in doubles (<= 10 * 2^-53).  The bound
    used, 2^-23 relative, is twice the float conversion and covers both."""
    genes, toc, g, c = toytest1.load()
    data = fsp0_binding.counts_of(g, c)
    n = len(toc) - 1
    dense = np.zeros((n, genes))
    for cell in range(n):
        for i in range(int(toc[cell]), int(toc[cell + 1])):
            dense[cell, g[i]] = c[i]
    expected = np.corrcoef(dense)
    cell, sim, used, low_index, low = restatement.find_similar_pairs0(toc, data, genes, 100, 0.2)
    for c0 in range(n):
        wanted = sorted(((-expected[c0, c1], c1) for c1 in range(n) if c1 != c0 and expected[c0, c1] > 0.2))
        assert used[c0] == len(wanted)
        for i, (negative, c1) in enumerate(wanted):
            assert cell[c0, i] == c1
            assert abs(float(sim[c0, i]) + negative) <= 2.0 ** -23 * abs(negative)
        if used[c0]:
            assert low[c0] == sim[c0, used[c0] - 1] and low_index[c0] < used[c0]
        else:
            assert low[c0] == FLT_MAX and low_index[c0] == INVALID
    assert used.sum() > 0


def test_find_similar_pairs0_fails_loudly_without_gpu():
    if capi.device_count() > 0:
        pytest.skip("a GPU is present")
    toc, data = fsp0_binding.clustered(8, 30, 0.3, seed=1)
    with pytest.raises(RuntimeError, match="no HIP device"):
        capi.find_similar_pairs0(toc, data, 30, 3, 0.2)
    # the argument checks answer before any device call
    with pytest.raises(RuntimeError, match="similarityThreshold <= 1"):
        capi.find_similar_pairs0(toc, data, 30, 3, 1.5)


@pytest.fixture()
def data_dir(tmp_path):
    d = str(tmp_path / "data")
    cells, genes = 40, 120
    toc, data = fsp0_binding.clustered(cells, genes, 0.1, seed=33, cluster_count=3, non_integer=True)
    files.create_directory(d, genes, toc, data)
    files.add_gene_set(d, "Some", np.unique((np.arange(70) * 5) % genes).astype(np.uint32))
    files.add_cell_set(d, "Odd", np.arange(1, cells, 2, dtype=np.uint32))
    return d


def test_compute_cell_similarity_on_a_directory(restatement, data_dir):
    e = ExpressionMatrix(data_dir)
    for gene_set in ("AllGenes", "Some"):
        n_genes, toc, data = e._subset(gene_set, "AllCells")
        for c0, c1 in [(0, 1), (5, 31), (39, 2), (7, 7)]:
            got = e.computeCellSimilarity(geneSetName=gene_set, cellId0=c0, cellId1=c1)
            want = restatement.cell_similarity(toc, data, n_genes, c0, c1)
            assert np.float64(got).view(np.uint64) == np.float64(want).view(np.uint64)
    assert e.computeCellSimilarity(cellId0=0, cellId1=1) == e.computeCellSimilarity("AllGenes", 0, 1)
    with pytest.raises(RuntimeError, match="Gene set Nope does not exist."):
        e.computeCellSimilarity("Nope", 0, 1)
    with pytest.raises(RuntimeError, match="cell id"):
        e.computeCellSimilarity("AllGenes", 0, 40)


def test_compare_similar_pairs_on_a_directory(restatement, data_dir, tmp_path, monkeypatch):
    e = ExpressionMatrix(data_dir)
    n_genes, toc, data = e._subset("Some", "Odd")
    n = len(toc) - 1
    results = {}
    for name, k, thr in (("A", 4, 0.1), ("B", 6, 0.1), ("C", 4, 0.1)):
        cell, sim, used, _, _ = restatement.find_similar_pairs0(toc, data, n_genes, k, thr)
        pairs = np.zeros((n, k), dtype=capi.PAIR_DTYPE)
        pairs["cell"], pairs["similarity"] = cell, sim
        files.write_similar_pairs(data_dir, name, "Some", "Odd", k, pairs, used)
        results[name] = (sim, used)
    files.write_similar_pairs(data_dir, "Other", "AllGenes", "Odd", 4, np.zeros((n, 4), dtype=capi.PAIR_DTYPE), np.zeros(n, dtype=np.uint32))
    monkeypatch.chdir(tmp_path)
    e.compareSimilarPairs("A", "B")
    lines = ["CellId,Stored0,Stored1,Lowest0,Lowest1,"]
    (sim0, used0), (sim1, used1) = results["A"], results["B"]
    for c in range(n):
        n0, n1 = int(used0[c]), int(used1[c])
        low0 = float(sim0[c, n0 - 1]) if n0 else 1.
        low1 = float(sim1[c, n1 - 1]) if n1 else 1.
        if n0 == n1 and low0 == low1:
            continue
        lines.append("%d,%d,%d,%s,%s," % (c, n0, n1, "%g" % low0 if n0 else "", "%g" % low1 if n1 else ""))
    assert len(lines) > 3
    assert open(tmp_path / "CompareSimilarPairs.csv").read() == "\n".join(lines) + "\n"
    e.compareSimilarPairs("A", "C")                                  # equal objects: the header alone
    assert open(tmp_path / "CompareSimilarPairs.csv").read() == lines[0] + "\n"
    with pytest.raises(RuntimeError, match="getGeneSet"):
        e.compareSimilarPairs("A", "Other")
