"""findSimilarGenePairs0 on the GPU (em2_gene_pairs.hip) against the C++ restatement of
src/ExpressionMatrixFindSimilarGenePairs.cpp:16-198 (tests/native/em2_gene_pairs_restatement.cpp): partner ids, float
similarity bits, usedCount and every r of allSimilarities, bit for bit; no tolerance anywhere.

The pair kernel works on tiles of 128 x 128 genes and stages 16 cells per step; lists of up to 8192 candidates are selected in
LDS, longer ones in global memory."""
import os

import numpy as np
import pytest

import fsp0_binding
import gene_pairs_binding as gpb
from expressionmatrix2_amd import ExpressionMatrix, NormalizationMethod, capi, files

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def restatement():
    return gpb.load()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def check(restatement, toc, data, genes, method, k, thr, all_similarities=True, label=""):
    gene, sim, used, r = restatement.find_similar_gene_pairs0(toc, data, genes, method, k, thr, all_similarities)
    device = capi.find_similar_gene_pairs0(toc, data, genes, method, k, thr, all_similarities)
    assert np.array_equal(device[1], used), label
    assert np.array_equal(device[0]["cell"], gene), label
    assert np.array_equal(bits(device[0]["similarity"]), bits(sim)), label
    if all_similarities:
        assert np.array_equal(bits(device[2]), bits(r)), label
    return gene, sim, used, r


@pytest.mark.parametrize("genes", [1, 2, 5, 129, 257, 513])
def test_gene_counts_around_tile_edges(restatement, genes):
    """One gene; two; fewer than a tile; one more than one, two and four tiles: diagonal and ragged tiles."""
    toc, data = fsp0_binding.clustered(40, genes, 0.25, seed=genes, cluster_count=3, non_integer=True)
    _, _, used, _ = check(restatement, toc, data, genes, gpb.L2, 10, 0.2)
    assert genes < 129 or used.sum() > 0


@pytest.mark.parametrize("cells", [1, 15, 16, 17, 1000])
def test_cell_counts_around_the_staging_chunk(restatement, cells):
    toc, data = fsp0_binding.clustered(cells, 150, 0.2, seed=cells, cluster_count=4, non_integer=True)
    _, _, used, _ = check(restatement, toc, data, 150, gpb.L2, 10, 0.2)
    assert cells == 1 or used.sum() > 0


@pytest.mark.parametrize("method", [gpb.NONE, gpb.L1, gpb.L2])
def test_normalization_methods(restatement, method):
    toc, data = fsp0_binding.clustered(60, 200, 0.15, seed=5, cluster_count=4, non_integer=True)
    _, _, used, _ = check(restatement, toc, data, 200, method, 100, 0.2)
    assert used.sum() > 0


@pytest.mark.parametrize("k", [0, 1, 100, 200])
def test_k(restatement, k):
    """k = 200 is greater than the gene count: no list is ever cut."""
    toc, data = fsp0_binding.clustered(70, 90, 0.2, seed=9, cluster_count=3, non_integer=True)
    _, _, used, _ = check(restatement, toc, data, 90, gpb.L2, k, 0.0)
    assert k == 0 or used.sum() > 0


@pytest.mark.parametrize("thr", [-1.0, 0.0, 0.2, 1.0])
def test_thresholds_with_lists_that_fit_lds(restatement, thr):
    """At -1 every pair that is not NaN survives: lists of 299 candidates against k = 10, selected in LDS."""
    toc, data = fsp0_binding.clustered(50, 300, 0.2, seed=13, cluster_count=4, non_integer=True)
    _, _, used, r = check(restatement, toc, data, 300, gpb.L2, 10, thr)
    if thr == -1.0:
        assert (used == 10).sum() > 250
    if thr == 1.0:
        assert (r.astype(np.float64) > 1.0).sum() == used.sum()          # (only what rounding lifted above 1, if anything)


def test_threshold_minus_one_with_lists_that_do_not_fit_lds(restatement):
    """12 001 genes x 6 cells at threshold -1: more than 8193 genes have variance, so their lists hold more than 8192
    candidates and are selected on their segments in global memory (the restatement alone needs about 5 s for its 7 * 10^7 pairs on one CPU thread:
    the smallest gene count that leaves the LDS form with these inputs).  (allSimilarities is refused at this size.)"""
    genes = 12001
    toc, data = fsp0_binding.clustered(6, genes, 0.9, seed=3, cluster_count=2, non_integer=True)
    dense = gpb.to_dense(toc, data, genes)
    assert ((dense != dense[0:1, :]).any(axis=0)).sum() > 8192 + 2
    _, _, used, _ = check(restatement, toc, data, genes, gpb.NONE, 3, -1.0, all_similarities=False)
    assert (used == 3).sum() > 8192
    with pytest.raises(RuntimeError, match="allSimilarities is an aid"):
        capi.find_similar_gene_pairs0(toc, data, genes, gpb.NONE, 3, -1.0, all_similarities=True)


def dense_input(cells, genes, seed):
    """Every cell stores every gene, with a non-integer count: every gene varies and no r is NaN."""
    rng = np.random.default_rng(seed)
    dense = (rng.gamma(2.0, 1.5, (cells, genes)) + 0.05).astype(np.float32)
    assert (dense != dense[0:1, :]).any(axis=0).all()
    return dense


def assert_every_r_is_above_minus_one(dense):
    """Every list holds all genes - 1 candidates at threshold -1 if no r is NaN or -1: the correlations once more in numpy doubles,
    band by band, with a margin of 10^-6 that is a thousand times the float rounding of r."""
    z = dense.astype(np.float64)
    z = z - z.mean(axis=0)
    z = z / np.sqrt((z * z).sum(axis=0))
    lowest = min(float((z[:, begin:begin + 1024].T @ z).min()) for begin in range(0, z.shape[1], 1024))
    assert lowest > -1. + 1e-6


@pytest.mark.parametrize("k", [299, 298])
def test_lists_at_the_length_k(restatement, k):
    """300 genes that all vary, threshold -1: every list has 299 candidates.  k = 299 leaves the lists alone (n <= k, heap.hpp:118);
    k = 298 is the shortest selection there is, the introselect of 298 among 299."""
    dense = dense_input(50, 300, seed=29)
    toc, data = gpb.dense_to_csr(dense)
    gene, sim, used, r = check(restatement, toc, data, 300, gpb.L2, k, -1.0)
    assert not np.isnan(r[~np.eye(300, dtype=bool)]).any() and (r[~np.eye(300, dtype=bool)].astype(np.float64) > -1.0).all()
    assert (used == k).all()


@pytest.mark.parametrize("genes", [8193, 8194])
def test_lists_at_the_lds_boundary(restatement, genes):
    """A dense 6-cell matrix in which every gene varies, threshold -1: with 8193 genes every list has exactly 8192 candidates, the
    longest that is selected in LDS; with 8194 genes 8193, the shortest that is selected in global memory.  (allSimilarities is
    refused above 8192 genes, so the lengths are asserted through numpy; the restatement needs about 3 s.)"""
    dense = dense_input(6, genes, seed=genes)
    assert_every_r_is_above_minus_one(dense)
    toc, data = gpb.dense_to_csr(dense)
    gene, sim, used, _ = check(restatement, toc, data, genes, gpb.NONE, 3, -1.0, all_similarities=False)
    assert (used == 3).all() and not np.isnan(sim).any()


def test_more_cells_than_one_grid_of_threads(restatement):
    """4 194 304 + 300 cells x 3 genes: the per-cell kernels run on a grid capped at 16 384 blocks of 256 threads and must
    stride over it; the cells behind the cap carry counts (so their sums and their normalisation show in every r) and, in
    the second call, the one bad gene id, which must be found before anything indexes with it."""
    cells, genes = 16384 * 256 + 300, 3
    rng = np.random.default_rng(41)
    present = rng.random((cells, genes)) < 0.5
    present[-1, :] = True
    toc = np.zeros(cells + 1, dtype=np.uint64)
    toc[1:] = np.cumsum(present.sum(axis=1))
    data = np.zeros(int(toc[-1]), dtype=gpb.COUNT_DTYPE)
    data["gene"] = np.nonzero(present)[1]
    data["count"] = (rng.random(len(data)) * 7. + 0.25).astype(np.float32)
    _, _, used, r = check(restatement, toc, data, genes, gpb.L2, 2, -1.0)
    assert (used == 2).all() and np.isfinite(r).all()
    data["gene"][-1] = genes
    with pytest.raises(RuntimeError, match="not below geneCount"):
        capi.find_similar_gene_pairs0(toc, data, genes)


@pytest.mark.parametrize("k,thr", [(3, 0.0), (5, 0.2), (12, -1.0), (1, 0.5)])
def test_ties_at_the_selection_boundary_and_inside_the_list(restatement, k, thr):
    """Duplicated genes and genes expressed in exactly one shared cell, small k:
    tests/test_gene_pairs_cpu.py::test_tie_input_is_not_a_plain_top_k shows that a plain top-k does not give this result."""
    toc, data, genes = gpb.tie_input()
    check(restatement, toc, data, genes, gpb.L2, k, thr)
    check(restatement, toc, data, genes, gpb.NONE, k, thr)


@pytest.mark.parametrize("method", [gpb.NONE, gpb.L1, gpb.L2])
def test_genes_without_variance(restatement, method):
    """An all-zero gene and a gene with the same count in every cell: NaN (or inf) by IEEE rules, nothing is special-cased,
    nothing is stored for NaN and nothing faults.  (After L1 / L2 the constant gene is no longer constant.)"""
    genes = 140
    toc, data = fsp0_binding.clustered(30, genes, 0.3, seed=17, cluster_count=3, non_integer=True)
    dense = gpb.to_dense(toc, data, genes)
    dense[:, 4] = 0.
    dense[:, 131] = 3.25
    toc, data = gpb.dense_to_csr(dense)
    gene, sim, used, r = check(restatement, toc, data, genes, method, 20, -1.0)
    assert np.isnan(r[4, [g for g in range(genes) if g != 4]]).all() and used[4] == 0
    if method == gpb.NONE:
        assert not np.isfinite(r[131, [g for g in range(genes) if g != 131]]).any()
    assert used.sum() > 0


@pytest.mark.parametrize("method", [gpb.NONE, gpb.L1, gpb.L2])
def test_empty_cell_and_subnormal_cell(restatement, method):
    """An empty cell (scaling == 0: the cell is left alone) and a cell whose only count is the smallest float subnormal: under
    L1 its factor float(1 / 1.4e-45) is inf, 0 * inf makes the whole cell NaN and with it every gene, so nothing at all is
    stored; under L2 its sum of squares is 0 and it is left alone."""
    genes = 140
    toc, data = fsp0_binding.clustered(30, genes, 0.3, seed=18, cluster_count=3, non_integer=True)
    dense = np.concatenate([gpb.to_dense(toc, data, genes), np.zeros((2, genes), dtype=np.float32)])
    dense[7, :] = 0.
    dense[:, 4] = 0.
    dense[31, 20] = np.float32(1e-45)
    toc, data = gpb.dense_to_csr(dense)
    assert toc[8] == toc[7] and toc[31] == toc[30] and toc[32] - toc[31] == 1
    gene, sim, used, r = check(restatement, toc, data, genes, method, 20, -1.0)
    if method == gpb.L1:
        assert used.sum() == 0 and np.isnan(r[~np.eye(genes, dtype=bool)]).all()
    else:
        assert used.sum() > 0 and used[4] == 0


def test_capacity_rerun(restatement, monkeypatch, capfd):
    """A buffer of 1 MB (43 690 records) and of 0 MB against 400 * 399 records at threshold -1: the pair kernel runs once
    more with the exact size, and the result is the unconstrained one."""
    genes = 400
    toc, data = fsp0_binding.clustered(45, genes, 0.25, seed=23, cluster_count=4, non_integer=True)
    monkeypatch.setenv("EM2_TIMING", "1")
    monkeypatch.delenv("EM2_GENE_PAIRS_BUFFER_MB", raising=False)
    unconstrained = capi.find_similar_gene_pairs0(toc, data, genes, gpb.L2, 7, -1.0, all_similarities=True)
    assert "exact size" not in capfd.readouterr().err
    for megabytes in ("1", "0"):
        monkeypatch.setenv("EM2_GENE_PAIRS_BUFFER_MB", megabytes)
        gene, sim, used, r = check(restatement, toc, data, genes, gpb.L2, 7, -1.0)
        assert "pair kernel (again, exact size)" in capfd.readouterr().err
        constrained = capi.find_similar_gene_pairs0(toc, data, genes, gpb.L2, 7, -1.0, all_similarities=True)
        for a, b in zip(unconstrained, constrained):
            assert a.tobytes() == b.tobytes()
    monkeypatch.delenv("EM2_GENE_PAIRS_BUFFER_MB")
    capi.apply_gene_pairs_buffer()


def test_input_errors():
    toc, data = fsp0_binding.clustered(30, 50, 0.2, seed=2)
    bad = data.copy()
    bad["gene"][5] = 50
    with pytest.raises(RuntimeError, match="not below geneCount"):
        capi.find_similar_gene_pairs0(toc, bad, 50)
    unsorted = data.copy()
    first = int(toc[3])
    unsorted["gene"][first], unsorted["gene"][first + 1] = data["gene"][first + 1], data["gene"][first]
    with pytest.raises(RuntimeError, match="strictly ascending"):
        capi.find_similar_gene_pairs0(toc, unsorted, 50)
    with pytest.raises(RuntimeError, match="invalid normalization method"):
        capi.find_similar_gene_pairs0(toc, data, 50, normalization_method=3)


@pytest.fixture()
def data_dir(tmp_path):
    d = str(tmp_path / "data")
    cells, genes = 300, 500
    toc, data = fsp0_binding.clustered(cells, genes, 0.06, seed=21, cluster_count=5, non_integer=True)
    files.create_directory(d, genes, toc, data)
    files.add_gene_set(d, "HighInformationGenes", np.unique((np.arange(260) * 7) % genes).astype(np.uint32))
    files.add_cell_set(d, "Subset", np.arange(3, cells, 2, dtype=np.uint32))
    return d


@pytest.mark.parametrize("gene_set,cell_set,method,k,thr", [("HighInformationGenes", "Subset", NormalizationMethod.L1, 12, 0.1),
                                                            ("AllGenes", "AllCells", None, 100, 0.2)])
def test_facade_writes_the_three_files(restatement, data_dir, gene_set, cell_set, method, k, thr):
    e = ExpressionMatrix(data_dir)
    if method is None:
        e.findSimilarGenePairs0(similarGenePairsName="Genes")                # the binding's defaults: L2, k = 100, 0.2
    else:
        e.findSimilarGenePairs0(geneSetName=gene_set, cellSetName=cell_set, normalizationMethod=method,
                                similarGenePairsName="Genes", k=k, similarityThreshold=thr)
    n_genes, toc, data = e._subset(gene_set, cell_set)
    gene, sim, used, _ = restatement.find_similar_gene_pairs0(toc, data, n_genes, int(method if method is not None else 2), k, thr)
    k2, pairs, used2 = files.read_similar_gene_pairs(data_dir, "Genes")
    assert k2 == k and np.array_equal(used2, used) and used.sum() > 0
    assert np.array_equal(pairs["cell"], gene) and np.array_equal(bits(pairs["similarity"]), bits(sim))
    info = files.similar_gene_pairs_info(data_dir, "Genes")
    assert (info["geneSetName"], info["cellSetName"], info["geneCount"]) == (gene_set, cell_set, n_genes)
    assert info["normalizationMethod"] == int(method if method is not None else NormalizationMethod.L2)
    e.removeSimilarGenePairs("Genes")
    for part in ("Info", "Pairs", "GeneInfo"):
        assert not os.path.exists(os.path.join(data_dir, "SimilarGenePairs-Genes-" + part))
    with pytest.raises(RuntimeError, match="Error removing similar gene pairs object Genes"):
        e.removeSimilarGenePairs("Genes")
