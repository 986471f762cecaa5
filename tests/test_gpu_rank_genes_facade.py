"""rankGenesByMetaData, rankGenesByClusterGraph, compareCellSets and topGenes on a synthetic store of 400 cells in four planted
clusters (tests/synth.py: most of a cell's genes come from its cluster's pool): the three methods against the independent
numpy statement (tests/rank_genes_binding.py) on the subset's CSR with the norm inverses of the cells' whole rows, the cluster
graph's ranking against compareCellSets(cluster, rest), the planted genes on top, and the error texts."""
import collections

import numpy as np
import pytest

import rank_genes_binding as rgb
import synth
from expressionmatrix2_amd import ExpressionMatrix, NormalizationMethod, capi, files, topGenes

pytestmark = pytest.mark.gpu

CELLS, GENES, CLUSTERS, SEED = 400, 600, 4, 78
SOME_GENES = np.arange(0, GENES, 3, dtype=np.uint32)
ODD_CELLS = np.arange(1, CELLS, 2, dtype=np.uint32)


def planted_cluster():
    return (synth.hash_u64(SEED, 11, np.arange(CELLS, dtype=np.uint64)) % np.uint64(CLUSTERS)).astype(np.int64)


def planted_genes(cluster):
    """The pool of a cluster, as synth.expression_matrix draws it."""
    pool_size = max(4, GENES // 50)
    slots = np.arange(pool_size, dtype=np.uint64)
    return set((synth.hash_u64(SEED, 15, np.uint64(cluster), slots) % np.uint64(GENES)).astype(np.int64).tolist())


@pytest.fixture(scope="module")
def store(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("rank_genes") / "data")
    toc, g, c = synth.expression_matrix(CELLS, GENES, density=0.05, cluster_count=CLUSTERS, seed=SEED)
    data = capi.make_counts(g, c)
    files.create_directory(d, GENES, toc, data)
    files.add_gene_set(d, "Some", SOME_GENES)
    files.add_cell_set(d, "Odd", ODD_CELLS)
    e = ExpressionMatrix(d)
    cluster = planted_cluster()
    for cell in range(CELLS):
        if cell % 17 != 3:                                                # the others have no field: the value ""
            e.setCellMetaData(cell, "Planted", "c%d" % cluster[cell])
    e.findSimilarPairs4(similarPairsName="P", k=20, similarityThreshold=0.2)
    e.createCellGraph("G", "AllCells", "P", similarityThreshold=0.3, k=10)
    e.createClusterGraph("G", "CG", minClusterSize=20)
    n1, n2 = rgb.norm_inverses(toc, data)
    yield e, {NormalizationMethod.none: None, NormalizationMethod.L1: n1, NormalizationMethod.L2: n2}
    e.close()


def expected(e, norms, gene_set, cell_ids, group, groups, method):
    """The numpy statement over the rows of cell_ids restricted to the gene set, [groups][genes] like the facade's arrays."""
    e.createCellSet("Expected", cell_ids)
    try:
        genes, toc, data = e._subset(gene_set, "Expected")
    finally:
        e.removeCellSet("Expected")
    norm = None if norms[method] is None else norms[method][np.sort(np.asarray(cell_ids))]
    theirs = rgb.numpy_statement(toc, data, genes, group, groups, norm)
    out = {name: np.ascontiguousarray(theirs[name].T) for name in ("nonZeroCount", "rankSum2", "zScore", "auc")}
    out.update(groupSizes=theirs["groupSize"], tieSum=theirs["tieSum"], pValue=rgb.p_values(out["zScore"]))
    return out


def assert_result(result, theirs, gene_ids, what):
    assert np.array_equal(result["geneIds"], gene_ids), what
    for name, array in theirs.items():
        a, b = result[name], array
        assert a.shape == b.shape and a.dtype == b.dtype, "%s: %s is %s %s, not %s %s" % (what, name, a.dtype, a.shape, b.dtype, b.shape)
        if a.dtype == np.float64:
            a, b = a.view(np.uint64), b.view(np.uint64)
        assert np.array_equal(a, b), "%s: %s differs" % (what, name)


@pytest.mark.parametrize("gene_set,cell_set,method", [("AllGenes", "AllCells", NormalizationMethod.L2), ("Some", "Odd", NormalizationMethod.L1),
                                                      ("Some", "AllCells", NormalizationMethod.none)])
def test_rank_genes_by_meta_data(store, gene_set, cell_set, method):
    e, norms = store
    cells = np.arange(CELLS, dtype=np.uint32) if cell_set == "AllCells" else ODD_CELLS
    gene_ids = np.arange(GENES, dtype=np.uint32) if gene_set == "AllGenes" else SOME_GENES
    cluster = planted_cluster()
    values = ["c%d" % cluster[cell] if cell % 17 != 3 else "" for cell in cells.tolist()]
    histogram = sorted(collections.Counter(values).items(), key=lambda item: (-item[1], item[0]))
    names = [value for value, _ in histogram]
    assert names == [value for value, _ in e._meta_data_histogram(cell_set, "Planted")] and "" in names and len(names) == CLUSTERS + 1
    group = np.array([names.index(value) for value in values], dtype=np.uint32)
    result = e.rankGenesByMetaData(gene_set, cell_set, "Planted", method)
    assert result["groupNames"] == names and result["groupSizes"].tolist() == [count for _, count in histogram]
    assert_result(result, expected(e, norms, gene_set, cells, group, len(names), method), gene_ids, "%s %s" % (gene_set, cell_set))
    assert result["zScore"].shape == (len(names), len(gene_ids))


def cluster_groups(e):
    """(cell ids of the universe ascending, group per cell, cluster ids) of the cluster graph CG."""
    cluster_ids = e.getClusterGraphVertices("CG")
    vertices = np.sort(np.asarray(e._cluster_graph("CG")["vertexCellIds"], dtype=np.uint32))
    group = np.full(len(vertices), rgb.NO_GROUP, dtype=np.uint32)
    for at, cluster_id in enumerate(cluster_ids):
        group[np.isin(vertices, e.getClusterCells("CG", cluster_id))] = at
    return vertices, group, cluster_ids


def test_rank_genes_by_cluster_graph(store):
    e, norms = store
    vertices, group, cluster_ids = cluster_groups(e)
    assert len(cluster_ids) >= 2
    result = e.rankGenesByClusterGraph("CG")
    assert result["groupNames"] == cluster_ids
    theirs = expected(e, norms, "AllGenes", vertices, group, len(cluster_ids), NormalizationMethod.L2)
    assert_result(result, theirs, np.arange(GENES, dtype=np.uint32), "the cluster graph's own gene set")
    some = e.rankGenesByClusterGraph("CG", "Some", NormalizationMethod.none)
    assert_result(some, expected(e, norms, "Some", vertices, group, len(cluster_ids), NormalizationMethod.none), SOME_GENES, "Some")


def test_one_cluster_against_the_rest_is_compare_cell_sets(store):
    e, _ = store
    vertices, group, cluster_ids = cluster_groups(e)
    ranked = e.rankGenesByClusterGraph("CG")
    e.createCellSet("Cluster", vertices[group == 1])
    e.createCellSet("Rest", vertices[group != 1])
    try:
        two = e.compareCellSets("AllGenes", "Cluster", "Rest")
        with pytest.raises(ValueError, match="share a cell"):
            e.compareCellSets("AllGenes", "Cluster", "AllCells")
    finally:
        e.removeCellSet("Cluster")
        e.removeCellSet("Rest")
    assert two["groupNames"] == ["Cluster", "Rest"] and two["groupSizes"].tolist() == [int((group == 1).sum()), int((group != 1).sum())]
    for name in ("nonZeroCount", "rankSum2", "zScore", "auc", "pValue"):
        assert np.array_equal(two[name][0].view(np.uint64 if two[name].dtype == np.float64 else two[name].dtype),
                              ranked[name][1].view(np.uint64 if two[name].dtype == np.float64 else two[name].dtype)), name
    assert np.array_equal(two["tieSum"], ranked["tieSum"])
    # two complementary groups: the rank sums add up to twice 1 + ... + N, z is mirrored exactly, auc up to its own rounding
    assert np.all(two["rankSum2"][0] + two["rankSum2"][1] == len(vertices) * (len(vertices) + 1))
    assert np.array_equal(two["zScore"][1], -two["zScore"][0]) and np.all(np.abs(two["auc"][0] + two["auc"][1] - 1.) <= 2. ** -52)


def test_top_genes_finds_the_planted_genes(store):
    e, _ = store
    result = e.rankGenesByMetaData(metaDataName="Planted")
    top = topGenes(result, 5)
    assert set(top) == set(result["groupNames"])
    for cluster in range(CLUSTERS):
        assert set(top["c%d" % cluster]) <= planted_genes(cluster), cluster
        z = result["zScore"][result["groupNames"].index("c%d" % cluster)]
        order = sorted(range(GENES), key=lambda g: (-z[g], g))
        assert top["c%d" % cluster] == order[:5]


def test_error_texts(store):
    e, _ = store
    with pytest.raises(RuntimeError, match=r"^Gene set Nothing does not exist\.$"):
        e.rankGenesByMetaData("Nothing", "AllCells", "Planted")
    with pytest.raises(RuntimeError, match=r"^Cell set Nothing does not exist\.$"):
        e.rankGenesByMetaData("AllGenes", "Nothing", "Planted")
    with pytest.raises(RuntimeError, match=r"^Meta data field Nothing not found\.$"):
        e.rankGenesByMetaData("AllGenes", "AllCells", "Nothing")
    with pytest.raises(TypeError):
        e.rankGenesByMetaData()
    with pytest.raises(RuntimeError, match=r"^Cluster graph Nothing does not exist\.$"):
        e.rankGenesByClusterGraph("Nothing")
    with pytest.raises(RuntimeError, match=r"^Gene set Nothing does not exist\.$"):
        e.rankGenesByClusterGraph("CG", "Nothing")
    with pytest.raises(RuntimeError, match=r"^Gene set Nothing does not exist\.$"):
        e.compareCellSets("Nothing", "Odd", "AllCells")
    with pytest.raises(RuntimeError, match=r"^Cell set Nothing does not exist\.$"):
        e.compareCellSets("AllGenes", "Odd", "Nothing")
    lib = capi.load()
    out = capi.rank_genes_arrays(GENES, 2)
    group = np.zeros(CELLS, dtype=np.uint32)
    arguments = (capi._ptr(group), 2, capi._ptr(out["groupSize"]), capi._ptr(out["nonZeroCount"]), capi._ptr(out["rankSum2"]),
                 capi._ptr(out["tieSum"]), None, None)
    assert lib.em2_matrix_rank_genes(e._handle, b"Nothing", b"AllCells", 2, *arguments) != 0
    assert lib.em2_last_error().decode() == "Gene set Nothing does not exist."
    assert lib.em2_matrix_rank_genes(e._handle, b"AllGenes", b"Nothing", 2, *arguments) != 0
    assert lib.em2_last_error().decode() == "Cell set Nothing does not exist."
    assert lib.em2_matrix_rank_genes(e._handle, b"AllGenes", b"AllCells", 2, *arguments) == 0 and out["groupSize"].tolist() == [CELLS, 0]
