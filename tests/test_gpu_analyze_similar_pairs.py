"""ExpressionMatrix.analyzeSimilarPairs on the GPU (exact similarity of every stored pair on the device, bins / draws / csv
lines on the host in the reference's order) against the C++ restatement of src/ExpressionMatrixLsh.cpp:55-150: both csv
files byte for byte, the bins' sums bit for bit."""
import numpy as np
import pytest

import expression_cases as ec
import fsp0_binding
from expressionmatrix2_amd import ExpressionMatrix, capi, files

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def restatement():
    return fsp0_binding.load()


@pytest.fixture()
def data_dir(tmp_path):
    d = str(tmp_path / "data")
    cells, genes = 700, 900
    toc, data = fsp0_binding.clustered(cells, genes, 0.03, seed=21, cluster_count=5, non_integer=True)
    files.create_directory(d, genes, toc, data)
    files.add_gene_set(d, "HighInformationGenes", np.unique((np.arange(300) * 7) % genes).astype(np.uint32))
    files.add_cell_set(d, "Subset", np.arange(3, cells, 2, dtype=np.uint32))
    return d


def check_files(restatement, e, data_dir, tmp_path, name, downsample):
    k, pairs, used = files.read_similar_pairs(data_dir, name)
    _, _, gene_set, cell_set = files.similar_pairs_info(data_dir, name)
    n_genes, toc, data = e._subset(gene_set, cell_set)
    ids = e._cell_set(cell_set)
    assert used.sum() > 0
    rc = restatement.analyze_similar_pairs(toc, data, n_genes, pairs["cell"], pairs["similarity"], used, ids, downsample,
                                           str(tmp_path / "r-pairs.csv"), str(tmp_path / "r-stats.csv"))
    assert rc == 0
    e.analyzeSimilarPairs(name, downsample)
    assert open(tmp_path / (name + "-analysis.csv"), "rb").read() == open(tmp_path / "r-pairs.csv", "rb").read()
    assert open(tmp_path / (name + "-analysis-statistics.csv"), "rb").read() == open(tmp_path / "r-stats.csv", "rb").read()
    assert len(open(tmp_path / "r-stats.csv").read().splitlines()) > 2


def test_analyze_an_fsp4_result(restatement, data_dir, tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    e = ExpressionMatrix(data_dir)
    e.findSimilarPairs4(geneSetName="HighInformationGenes", cellSetName="Subset", similarPairsName="Lsh", k=15, similarityThreshold=0.2,
                        lshCount=256)
    check_files(restatement, e, data_dir, tmp_path, "Lsh", 0.05)


def test_analyze_an_fsp0_result(restatement, data_dir, tmp_path, monkeypatch):
    """An exact result has at most the float conversion as error; a pair with exact similarity 1 would trip the
    reference's bin assert, so the threshold stays low and the cells distinct."""
    monkeypatch.chdir(tmp_path)
    e = ExpressionMatrix(data_dir)
    e.findSimilarPairs0(similarPairsName="Exact", k=8, similarityThreshold=0.1)
    check_files(restatement, e, data_dir, tmp_path, "Exact", 1.0)


def test_bin_assert_is_reported(restatement, tmp_path):
    """Two identical cells stored as each other's neighbour: exact similarity 1, bin 200, CZI_ASSERT(bin < binCount)."""
    toc, data = fsp0_binding.clustered(6, 40, 0.3, seed=3)
    toc, data = fsp0_binding.repeat_cells(toc, data, [2, 1, 1, 1, 1, 1])
    n = len(toc) - 1
    pairs = np.zeros((n, 2), dtype=capi.PAIR_DTYPE)
    pairs["cell"][0, 0], pairs["similarity"][0, 0] = 1, 1.0
    used = np.zeros(n, dtype=np.uint32)
    used[0] = 1
    ids = np.arange(n, dtype=np.uint32)
    assert restatement.analyze_similar_pairs(toc, data, 40, pairs["cell"], pairs["similarity"], used, ids, 1.0,
                                             str(tmp_path / "r.csv"), str(tmp_path / "rs.csv")) == 1
    with pytest.raises(RuntimeError, match="bin < binCount"):
        capi.analyze_similar_pairs(toc, data, 40, pairs, used, ids, 1.0, str(tmp_path / "d.csv"), str(tmp_path / "ds.csv"))


def test_infinite_similarity_trips_the_bin_assert(restatement, tmp_path):
    """The input of tests/test_gpu_analyze_lsh.py::test_analyze_lsh_infinite_similarity_trips_the_bin_assert: cell 0 has no
    variance and its exact similarity to cell 1 is +inf.  Converting that to size_t is undefined; the assert must fire on both
    sides whatever the compiler makes of it."""
    toc, data = ec.matrix(ec.INFINITE_SIMILARITY_CASE)
    assert np.isposinf(restatement.cell_similarity(toc, data, 1025, 0, 1))
    pairs = np.zeros((3, 1), dtype=capi.PAIR_DTYPE)
    pairs["cell"][:, 0], pairs["similarity"][:, 0] = [1, 2, 1], 0.25
    used = np.array([1, 1, 1], dtype=np.uint32)
    ids = np.arange(3, dtype=np.uint32)
    assert restatement.analyze_similar_pairs(toc, data, 1025, pairs["cell"], pairs["similarity"], used, ids, 1.0,
                                             str(tmp_path / "r.csv"), str(tmp_path / "rs.csv")) == 1
    with pytest.raises(RuntimeError, match="bin < binCount"):
        capi.analyze_similar_pairs(toc, data, 1025, pairs, used, ids, 1.0, str(tmp_path / "d.csv"), str(tmp_path / "ds.csv"))


def test_global_memory_form(restatement, tmp_path):
    """More genes than LDS holds and more rows than the global-memory form has blocks (fsp0_binding.wide_matrix).  The stored
    object is a synthetic one as below: k = 8, usedCount varying, one cell that stores nothing."""
    toc, data, genes = fsp0_binding.wide_matrix()
    cells, k = len(toc) - 1, 8
    pairs = np.zeros((cells, k), dtype=capi.PAIR_DTYPE)
    pairs["cell"] = (np.arange(cells, dtype=np.uint32)[:, None] + 1 + np.arange(k, dtype=np.uint32)[None, :] * 7) % cells
    pairs["similarity"] = 0.25
    used = (k - (np.arange(cells) % 5)).astype(np.uint32)
    used[1050] = 0
    ids = (np.arange(cells, dtype=np.uint32) * 3 + 5).astype(np.uint32)
    rc = restatement.analyze_similar_pairs(toc, data, genes, pairs["cell"], pairs["similarity"], used, ids, 0.5,
                                           str(tmp_path / "r-pairs.csv"), str(tmp_path / "r-stats.csv"))
    if rc == 1:
        pytest.fail("the synthetic input holds a pair with exact similarity 1: choose another seed")
    capi.analyze_similar_pairs(toc, data, genes, pairs, used, ids, 0.5, str(tmp_path / "d-pairs.csv"), str(tmp_path / "d-stats.csv"))
    for name in ("pairs", "stats"):
        assert open(tmp_path / ("d-%s.csv" % name), "rb").read() == open(tmp_path / ("r-%s.csv" % name), "rb").read()
    assert len(open(tmp_path / "r-pairs.csv").read().splitlines()) > 1000
    assert len(open(tmp_path / "r-stats.csv").read().splitlines()) > 2


@pytest.mark.parametrize("beyond", [0, 1])
def test_at_the_lds_limit(restatement, tmp_path, beyond):
    """storedPairsKernel has no LDS of its own, but its launch takes the cut-over of fsp0 with one slot: the largest gene count
    that rule leaves in LDS, and one gene more (the global-memory form); every cell's last entry is on one of the three highest
    genes.  The stored object is a synthetic one (expression_cases.stored_object): k = 65, a quarter of the cells full."""
    cells, k = 130, 65
    genes = ec.largest_gene_count_in_lds(ec.fsp0_own_lds_bytes(1)) + beyond
    assert ec.stored_pairs_in_lds(genes) == (beyond == 0) and ec.row_vector_bytes(genes) <= 160 * 1024
    toc, data = ec.lds_limit_input(cells, genes, non_integer=False)
    pairs, used = ec.stored_object({"cells": cells, "k": k, "pairs_seed": 5})
    assert (used == k).sum() > 10 and (pairs["cell"] != np.arange(cells)[:, None]).all()
    ids = (np.arange(cells, dtype=np.uint32) * 3 + 5).astype(np.uint32)
    rc = restatement.analyze_similar_pairs(toc, data, genes, pairs["cell"], pairs["similarity"], used, ids, 0.5,
                                           str(tmp_path / "r-pairs.csv"), str(tmp_path / "r-stats.csv"))
    if rc == 1:
        pytest.fail("the synthetic input holds a pair with exact similarity 1: choose another seed")
    capi.analyze_similar_pairs(toc, data, genes, pairs, used, ids, 0.5, str(tmp_path / "d-pairs.csv"), str(tmp_path / "d-stats.csv"))
    for name in ("pairs", "stats"):
        assert open(tmp_path / ("d-%s.csv" % name), "rb").read() == open(tmp_path / ("r-%s.csv" % name), "rb").read()
    assert len(open(tmp_path / "r-pairs.csv").read().splitlines()) > 1000


def test_more_stored_pairs_than_one_chunk(restatement, tmp_path):
    """The device works in chunks of 2^24 slots: 70 000 cells x k = 300 is 21M slots, two chunks; the bins and the draws carry
    over.  The stored object is a synthetic one (each cell's next 300 cells with a made-up similarity)."""
    cells, genes, k = 70000, 200, 300
    toc, data = fsp0_binding.clustered(cells, genes, 0.05, seed=6, cluster_count=16, non_integer=True)
    pairs = np.zeros((cells, k), dtype=capi.PAIR_DTYPE)
    pairs["cell"] = (np.arange(cells, dtype=np.uint32)[:, None] + 1 + np.arange(k, dtype=np.uint32)[None, :] * 7) % cells
    pairs["similarity"] = 0.25
    used = (k - (np.arange(cells) % 5)).astype(np.uint32)
    ids = np.arange(cells, dtype=np.uint32)
    rc = restatement.analyze_similar_pairs(toc, data, genes, pairs["cell"], pairs["similarity"], used, ids, 0.0001,
                                           str(tmp_path / "r-pairs.csv"), str(tmp_path / "r-stats.csv"))
    if rc == 1:
        pytest.fail("the synthetic input holds a pair with exact similarity 1: choose another seed")
    capi.analyze_similar_pairs(toc, data, genes, pairs, used, ids, 0.0001, str(tmp_path / "d-pairs.csv"), str(tmp_path / "d-stats.csv"))
    for name in ("pairs", "stats"):
        assert open(tmp_path / ("d-%s.csv" % name), "rb").read() == open(tmp_path / ("r-%s.csv" % name), "rb").read()
