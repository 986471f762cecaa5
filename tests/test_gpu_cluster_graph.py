"""createClusterGraph on the GPU: em2_cluster_average_expression, em2_cluster_similarities and em2_cluster_graph_create
against the C++ restatement of src/ClusterGraph.cpp:59-386 / src/ExpressionMatrix.cpp:1179-1296 /
src/regressionCoefficient.cpp (tests/native/em2_cluster_graph_restatement.cpp), bit for bit: clusters, cell order, final
ids, every double of the averages, every edge and its similarity.  Then the facade from findSimilarPairs4 on, its error
texts, and BASELINE config B's size.  Every parity case checks on the restatement's output that neither of the two places
the reference leaves open (a makeKnn tie, a NaN similarity) was reached."""
import time

import numpy as np
import pytest

import cluster_graph_binding as cgb
import fsp0_binding
import synth
from expressionmatrix2_amd import ExpressionMatrix, capi, files

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def restatement():
    return cgb.load()


def check_entry_points(restatement, case):
    """The three entry points on one case."""
    expected = restatement.create(*case.arguments(), **case.parameters)
    cgb.assert_parity_case(expected)
    got = capi.cluster_graph_create(*case.arguments(), **case.parameters)
    cgb.assert_same_graph(got, expected)
    # the averages and similarities of the graph as the constructor leaves it (every label a cluster) and after the merge
    # (cell lists that are not ascending), through the two smaller entry points
    rows = case.vertex_rows if case.vertex_rows is not None else np.arange(len(case.labels), dtype=np.uint32)
    for stage in (1, 2):
        graph = restatement.create(*case.arguments(), stop_after=stage, **case.parameters)
        offsets = graph["cellOffsets"]
        cells = rows[graph["cells"]]
        averages = capi.cluster_average_expression(case.toc, case.data, case.genes, cells, offsets)
        # stop_after 2 leaves the averages of before the merge in the graph: restate them for these lists
        wanted = restatement.average_expression(case.toc, case.data, case.genes, cells, offsets)
        assert np.array_equal(cgb.bits(averages), cgb.bits(wanted))
        position = {int(label): i for i, label in enumerate(graph["clusterIds"].tolist())}
        e0 = np.array([position[int(x)] for x in graph["edgeCluster0"]], dtype=np.uint32)
        e1 = np.array([position[int(x)] for x in graph["edgeCluster1"]], dtype=np.uint32)
        similarity = capi.cluster_similarities(wanted, e0, e1)
        assert np.array_equal(cgb.bits(similarity), cgb.bits(restatement.similarities(wanted, e0, e1)))
        if stage == 1:
            assert np.array_equal(cgb.bits(similarity), cgb.bits(graph["edgeSimilarity"]))
            assert np.array_equal(cgb.bits(wanted), cgb.bits(graph["averages"]))
    return got, expected


@pytest.mark.parametrize("name", sorted(cgb.SMALL_CASES))
def test_hand_made_cases(restatement, name):
    got, expected = check_entry_points(restatement, cgb.SMALL_CASES[name]())
    if name.startswith("merge_split"):
        assert sorted(np.diff(got["cellOffsets"]).tolist()) == [14, 15, 24] and len(got["edgeSimilarity"]) == 1
    if name == "chain3":
        assert sorted(np.diff(got["cellOffsets"]).tolist()) == [12, 30]
    if name in ("small", "rows", "wide"):
        assert len(got["unclusteredCells"]) == 8 and len(got["clusterIds"]) == 3
    if name == "knn":
        assert len(got["edgeSimilarity"]) == 5
    if name == "renumber":
        assert len(got["clusterIds"]) == 48


def test_averages_of_arbitrary_lists(restatement):
    """Lists that are not ascending, a cell in two lists and twice in one, a cluster of one cell, an entry per gene."""
    for non_integer in (False, True):
        toc, data = fsp0_binding.clustered(300, 700, 0.05, seed=31, cluster_count=4, non_integer=non_integer)
        if non_integer:
            data = cgb.wide_range(data)
        cells = np.concatenate([cgb.interleave(np.zeros(300), seed=2)[:170], [5], [9, 9, 250, 3], np.arange(299, 100, -1)]).astype(np.uint32)
        offsets = np.array([0, 170, 171, 175, len(cells)], dtype=np.uint64)
        got = capi.cluster_average_expression(toc, data, 700, cells, offsets)
        assert np.array_equal(cgb.bits(got), cgb.bits(restatement.average_expression(toc, data, 700, cells, offsets)))
        e0, e1 = np.array([0, 0, 3, 2, 1], dtype=np.uint32), np.array([1, 3, 2, 0, 3], dtype=np.uint32)
        similarity = capi.cluster_similarities(got, e0, e1)
        assert np.array_equal(cgb.bits(similarity), cgb.bits(restatement.similarities(got, e0, e1)))
        assert not np.isnan(similarity).any()


@pytest.mark.parametrize("density", [0.15, 0.4])
@pytest.mark.parametrize("genes", [1023, 1024, 1025, 2049])
def test_gene_counts_around_the_chunk_of_1024(restatement, genes, density):
    """clusterNormalizeKernel, clusterVertexSumsKernel and clusterEdgeKernel add a vector's products in chunks of 1024 doubles:
    one gene less than a chunk, exactly one, one gene into the second, one gene into the third.  Counts non-integer and spread
    over 48 binary orders; lists as in test_averages_of_arbitrary_lists.  The generator draws most of a cell's genes from a small
    pool, so density 0.15 does not store the 150 entries per cell it aims at but a median of 64 (128 at 2049 genes): the second
    stride of clusterGatherKernel's 64 lanes in half the cells.  Density 0.4 stores a median of 130 (270): the third stride and
    more in most cells.  (With these averages a few genes dominate every sum; what shows the ORDER inside a later chunk is
    test_edge_sums_in_later_chunks.)"""
    toc, data = fsp0_binding.clustered(300, genes, density, seed=31, cluster_count=4, non_integer=True)
    data = cgb.wide_range(data)
    lengths = np.diff(toc.astype(np.int64))
    assert np.median(lengths) >= 64 and lengths.max() > 64 and (density < 0.4 or np.median(lengths) > 128)
    assert genes < 2049 or (np.median(lengths) >= 128 and lengths.max() > 128)
    cells = np.concatenate([cgb.interleave(np.zeros(300), seed=2)[:170], [5], [9, 9, 250, 3], np.arange(299, 100, -1)]).astype(np.uint32)
    offsets = np.array([0, 170, 171, 175, len(cells)], dtype=np.uint64)
    got = capi.cluster_average_expression(toc, data, genes, cells, offsets)
    assert np.array_equal(cgb.bits(got), cgb.bits(restatement.average_expression(toc, data, genes, cells, offsets)))
    e0, e1 = np.array([0, 0, 3, 2, 1], dtype=np.uint32), np.array([1, 3, 2, 0, 3], dtype=np.uint32)
    similarity = capi.cluster_similarities(got, e0, e1)
    assert np.array_equal(cgb.bits(similarity), cgb.bits(restatement.similarities(got, e0, e1)))
    assert not np.isnan(similarity).any()


@pytest.mark.parametrize("genes", [1025, 1027, 1040, 2049])
def test_edge_sums_in_later_chunks(restatement, genes):
    """The order of clusterEdgeKernel's additions inside the chunks behind the first: 24 vectors of signed values over 16 binary
    orders (no gene dominates, the sums cancel, so one rounding of sxy shows in the quotient) and all 276 pairs of them through
    capi.cluster_similarities.  Adding the products of the later chunks in descending order changes 13 of the 276 similarities at
    1027 genes (a second chunk of three products), 48 at 1040, 253 at 2049, counted with the sums written out in Python; at 1025
    genes the second chunk holds one product and only its place can show, not its order."""
    rng = np.random.default_rng(71 + genes)
    table = rng.standard_normal((24, genes)) * np.exp2(rng.integers(-8, 8, (24, genes)).astype(np.float64))
    e0 = np.array([i for i in range(24) for j in range(i + 1, 24)], dtype=np.uint32)
    e1 = np.array([j for i in range(24) for j in range(i + 1, 24)], dtype=np.uint32)
    expected = restatement.similarities(table, e0, e1)
    assert not np.isnan(expected).any() and len(set(cgb.bits(expected).tolist())) == 276
    assert np.array_equal(cgb.bits(capi.cluster_similarities(table, e0, e1)), cgb.bits(expected))


def test_create_at_1025_genes(restatement):
    """One full createClusterGraph whose vectors reach into the second chunk: five planted clusters, two of them split over labels,
    non-integer counts spread over 48 binary orders, through all three entry points."""
    spec = [(120, 0, 0.), (100, 0, 0.25), (80, 0, 0.35), (60, 3, 0.), (40, 3, 0.3)]
    toc, data, owner = cgb.planted(spec, 1025, 0.15, seed=51, non_integer=True, noise=0.2)
    data = cgb.wide_range(data)
    assert np.diff(toc.astype(np.int64)).max() > 128
    piece = (synth.hash_u64(53, np.arange(len(owner), dtype=np.uint64)) % np.uint64(5)).astype(np.uint32)
    labels = (owner * 5 + np.where(piece < 3, 0, piece)).astype(np.uint32)
    toc, data, labels = cgb.shuffled(toc, data, labels, seed=54)
    ids = sorted(set(labels.tolist()))
    v0, v1 = cgb.edges_between(labels, [(a, b) for i, a in enumerate(ids) for b in ids[i + 1:] if (a + b) % 3])
    case = cgb.Case(toc, data, 1025, labels, v0, v1, min_cluster_size=30, k=3, similarity_threshold=-1.)
    got, expected = check_entry_points(restatement, case)
    assert len(expected["clusterIds"]) >= 2 and len(expected["edgeSimilarity"]) > 0


def test_more_edges_than_blocks(restatement):
    """clusterEdgeKernel strides the edges over at most 2^20 blocks: 2^20 + 5 edges over 3 clusters x 8 genes, so five blocks take
    a second edge -- between another pair of clusters than their first."""
    rng = np.random.default_rng(61)
    averages = rng.gamma(2.0, 1.5, (3, 8)) * np.exp2(rng.integers(-20, 20, (3, 8)).astype(np.float64))
    edges = (1 << 20) + 5
    at = np.arange(edges, dtype=np.uint64)
    e0 = (synth.hash_u64(62, at) % np.uint64(3)).astype(np.uint32)
    e1 = ((e0 + 1 + synth.hash_u64(63, at) % np.uint64(2)) % 3).astype(np.uint32)
    for e in range(1 << 20, edges):                              # the strided edges join another pair than the block's first edge
        first = e - (1 << 20)
        e0[e] = (e0[first] + 1) % 3
        e1[e] = (e0[e] + 1 + (e1[first] == (e0[e] + 1) % 3)) % 3
        assert {int(e0[e]), int(e1[e])} != {int(e0[first]), int(e1[first])} and e0[e] != e1[e]
    expected = restatement.similarities(averages, e0, e1)
    assert len(set(cgb.bits(expected).tolist())) == 3 and not np.isnan(expected).any()
    got = capi.cluster_similarities(averages, e0, e1)
    assert np.array_equal(cgb.bits(got), cgb.bits(expected))


def test_a_few_thousand_cells_many_labels(restatement):
    """3000 planted cells under 24 labels of very different size (three fifths of a cluster, and two slivers of it), integer and not."""
    for non_integer in (False, True):
        spec = [(600, 0, 0.), (500, 0, 0.25), (450, 0, 0.35), (400, 3, 0.), (350, 3, 0.3), (300, 5, 0.), (250, 5, 0.3), (150, 0, 0.5)]
        toc, data, owner = cgb.planted(spec, 400, 0.12, seed=41, non_integer=non_integer, noise=0.2)
        n = len(owner)
        piece = (synth.hash_u64(43, np.arange(n, dtype=np.uint64)) % np.uint64(5)).astype(np.uint32)
        labels = (owner * 5 + np.where(piece < 3, 0, piece)).astype(np.uint32)          # 3/5 of a cluster, and two slivers
        toc, data, labels = cgb.shuffled(toc, data, labels, seed=44)
        ids = sorted(set(labels.tolist()))
        pairs = [(a, b) for i, a in enumerate(ids) for b in ids[i + 1:] if (a + b) % 3]
        v0, v1 = cgb.edges_between(labels, pairs)
        case = cgb.Case(toc, data, 400, labels, v0, v1, min_cluster_size=100, k=3)
        got, expected = check_entry_points(restatement, case)
        assert len(expected["unclusteredCells"]) > 0 and 2 <= len(expected["clusterIds"]) < len(ids)
        assert len(expected["edgeSimilarity"]) > 0


def test_nan_similarity_is_an_error(restatement):
    case = cgb.case_nan()
    with pytest.raises(cgb.NanSimilarity):
        restatement.create(*case.arguments(), **case.parameters)
    with pytest.raises(RuntimeError, match="NaN"):
        capi.cluster_graph_create(*case.arguments(), **case.parameters)


def test_bad_arguments():
    case = cgb.case_small()
    bad = case.data.copy()
    bad["gene"][3] = case.genes
    with pytest.raises(RuntimeError, match="not below geneCount"):
        capi.cluster_graph_create(case.toc, bad, case.genes, None, case.v0, case.v1, case.labels, **case.parameters)
    with pytest.raises(RuntimeError, match="does not exist"):
        capi.cluster_average_expression(case.toc, case.data, case.genes, [len(case.labels)], [0, 1])
    with pytest.raises(RuntimeError, match="does not exist"):
        capi.cluster_similarities(np.ones((2, 8)), [0], [2])


def facade_against_restatement(restatement, e, cell_graph, cluster_graph, **parameters):
    """createClusterGraph through the facade and every accessor against the restatement fed the same labels."""
    g = e._cell_graph(cell_graph)
    cell_ids, labels = e.labelPropagationClustering(cell_graph)
    t0 = time.time()
    e.createClusterGraph(cell_graph, cluster_graph, **parameters)
    seconds = time.time() - t0
    gene_set = files.similar_pairs_info(e.directoryName, g["similarPairsName"])[2]
    gene_count, toc, data = e._subset(gene_set, g["cellSetName"])
    graph_cells = e._cell_set(g["cellSetName"])
    rows = np.searchsorted(graph_cells, cell_ids).astype(np.uint32)
    assert np.array_equal(graph_cells[rows], cell_ids)
    v0, v1 = g["edgeVertices"]
    t0 = time.time()
    expected = restatement.create(toc, data, gene_count, rows, v0, v1, labels,
                                  min_cluster_size=parameters.get("minClusterSize", 100), k=parameters.get("k", 3),
                                  similarity_threshold=parameters.get("similarityThreshold", 0.5),
                                  similarity_threshold_for_merge=parameters.get("similarityThresholdForMerge", 0.9))
    print("createClusterGraph: %d cells, %d labels -> %d clusters, %d edges; facade %.2f s, one-thread restatement %.2f s"
          % (len(labels), len(set(labels.tolist())), len(expected["clusterIds"]), len(expected["edgeSimilarity"]), seconds,
             time.time() - t0))
    cgb.assert_parity_case(expected)
    ids = expected["clusterIds"].tolist()
    assert e.getClusterGraphVertices(cluster_graph) == sorted(ids) == list(range(len(ids)))
    assert len(e.getClusterGraphGenes(cluster_graph)) == gene_count
    for at, cluster_id in enumerate(ids):
        begin, end = int(expected["cellOffsets"][at]), int(expected["cellOffsets"][at + 1])
        assert e.getClusterCells(cluster_graph, cluster_id) == cell_ids[expected["cells"][begin:end]].tolist()
        average = np.array(e.getClusterAverageExpression(cluster_graph, cluster_id), dtype=np.float64)
        assert np.array_equal(cgb.bits(average), cgb.bits(expected["averages"][at]))
    edges = e._cluster_graph_edges(cluster_graph)
    assert [(a, b) for a, b, _ in edges] == list(zip(expected["edgeCluster0"].tolist(), expected["edgeCluster1"].tolist()))
    assert np.array_equal(cgb.bits([s for _, _, s in edges]), cgb.bits(expected["edgeSimilarity"]))
    assert e._cluster_graph_unclustered_cells(cluster_graph) == cell_ids[expected["unclusteredCells"]].tolist()
    return expected, labels


def test_facade_end_to_end(restatement, tmp_path):
    d = str(tmp_path / "data")
    cells, genes = 4000, 1500
    toc, g, c = synth.expression_matrix(cells, genes, density=0.03, cluster_count=12, seed=77)
    files.create_directory(d, genes, toc, capi.make_counts(g, c))
    gene_ids = np.unique((np.arange(1000) * 7) % genes).astype(np.uint32)                 # fewer than all genes
    files.add_gene_set(d, "Some", gene_ids)
    files.add_cell_set(d, "Most", np.arange(1, cells, dtype=np.uint32)[np.arange(1, cells) % 7 != 0])
    e = ExpressionMatrix(d)
    e.findSimilarPairs4(geneSetName="Some", cellSetName="Most", similarPairsName="P", k=20, similarityThreshold=0.2)
    e.createCellGraph("G", "Most", "P", similarityThreshold=0.3, k=10)
    _, labels = e.labelPropagationClustering("G")
    sizes = np.sort(np.bincount(labels))[::-1]
    assert len(sizes) > 2 and sizes[0] > sizes[-1]
    # between the sizes of the second largest and the smallest label: some clusters go and (at least) two stay
    min_cluster_size = int(sizes[-1]) + 1 if sizes[1] > sizes[-1] else int(sizes[0])
    expected, _ = facade_against_restatement(restatement, e, "G", "C", minClusterSize=min_cluster_size, k=2,
                                             similarityThreshold=0.1, similarityThresholdForMerge=0.8)
    assert len(expected["unclusteredCells"]) > 0 and len(expected["clusterIds"]) > 0
    assert e.getClusterGraphGenes("C") == gene_ids.tolist()
    # the reference's error texts (src/ExpressionMatrix.cpp:2125, :2138, :2215, :2263)
    with pytest.raises(RuntimeError, match=r"^Cell graph Nope does not exist\.$"):
        e.createClusterGraph("Nope", "C2")
    with pytest.raises(RuntimeError, match=r"^Cluster graph C already exists\.$"):
        e.createClusterGraph("G", "C")
    for call in (e.getClusterGraphVertices, e.getClusterGraphGenes):
        with pytest.raises(RuntimeError, match=r"^Cluster graph Nope does not exist\.$"):
            call("Nope")
    with pytest.raises(RuntimeError, match=r"^Cluster graph Nope does not exist\.$"):
        e.getClusterCells("Nope", 0)
    missing = len(expected["clusterIds"])
    with pytest.raises(RuntimeError, match=r"^Cluster %d of cluster graph C does not exist\.$" % missing):
        e.getClusterCells("C", missing)
    with pytest.raises(RuntimeError, match=r"^Cluster %d of cluster graph C does not exist\.$" % missing):
        e.getClusterAverageExpression("C", missing)
    # the defaults are the reference's (src/PythonModule.cpp:1083-1089) and labelPropagationClustering is unchanged
    e.createClusterGraph(cellGraphName="G", clusterGraphName="Defaults")
    again = capi.cell_graph_label_propagation(e._cell_graph("G")["vertexCellIds"], *e._cell_graph("G")["edgeVertices"],
                                              e._cell_graph("G")["edgeSimilarity"])[0]
    assert np.array_equal(again, labels)


def test_baseline_config_b_size(restatement, tmp_path):
    """BASELINE config B: 100 000 cells x 20 000 genes, 1 % density; labels from the chain findSimilarPairs4 ->
    createCellGraph -> label propagation; everything compared with the restatement."""
    d = str(tmp_path / "data")
    cells, genes = 100000, 20000
    toc, g, c = synth.expression_matrix(cells, genes, density=0.01, cluster_count=64, seed=12345)
    files.create_directory(d, genes, toc, capi.make_counts(g, c))
    e = ExpressionMatrix(d)
    e.findSimilarPairs4(similarPairsName="P", k=100, similarityThreshold=0.2)
    e.createCellGraph("G", "AllCells", "P", similarityThreshold=0.2, k=20)       # the chain's threshold (BASELINE configs[4])
    expected, labels = facade_against_restatement(restatement, e, "G", "C")
    assert len(labels) > 0.9 * cells and len(expected["clusterIds"]) > 1
