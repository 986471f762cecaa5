"""createGeneGraph and getGeneGraphConnectivity on the GPU (csrc/em2_gene_graph.hip) against
tests/native/em2_gene_graph_restatement.cpp, which tests/test_gene_graph_cpu.py holds against the closed form in Python and
against hand-written expectations.  Index work only: the three sizes and every array of em2_gene_graph_get equal the
restatement's bit for bit (the float arrays are compared as uint32)."""
import ctypes

import numpy as np
import pytest

import gene_graph_binding as ggb
import synth
from expressionmatrix2_amd import ExpressionMatrix, capi, files

pytestmark = pytest.mark.gpu

INVALID = 1


@pytest.mark.parametrize("name", ggb.GRAPH_CASES)
def test_graph_equals_the_restatement(name):
    """The shapes of the issue: gene counts 1, 63, 64, 65, 257, 1000; usedCount 0 and k; limits 1, 0, 2^64 - 1, reached on the
    last stored pair and by a duplicate add_edge; thresholds equal to a stored float, one ulp above, 0.2 against float32(0.2), a
    NaN; S equal to P, a subset, a superset, interleaved, disjoint, each with consecutive ids and with gaps; edges selected by
    both ends, the lower, the higher; asymmetric similarities; isolated vertices; the hub."""
    ggb.assert_same_graph(capi.gene_graph_create(*ggb.arguments(ggb.case(name))), ggb.reference(name), name)


def test_disjoint_sets_give_an_empty_graph():
    for spacing in ("consecutive", "gaps"):
        c = ggb.case("sets-disjoint-" + spacing)
        graph = capi.gene_graph_create(*ggb.arguments(c))
        assert len(graph["vertices"]) == len(graph["edgeGene0"]) == len(graph["connectivityGenes"]) == 0
        assert graph["removedCount"] == len(c["S"]) and graph["connectivityOffsets"].tolist() == [0] * (len(c["S"]) + 1)


def test_the_hub_has_599_neighbours():
    graph = capi.gene_graph_create(*ggb.arguments(ggb.case("hub")))
    assert np.diff(graph["connectivityOffsets"]).tolist() == [599] + [1] * 599
    assert graph["connectivityGenes"][:599].tolist() == list(range(1, 600)) and graph["removedCount"] == 0


@pytest.mark.parametrize("name", ["genes-1", "genes-257", "sets-interleaved-gaps", "sets-disjoint-consecutive", "nan", "hub", "k-16"])
def test_device_entry_equals_the_host_entry_and_a_call_repeats_itself(name):
    arguments = ggb.arguments(ggb.case(name))
    first = capi.gene_graph_create(*arguments)
    second = capi.gene_graph_create(*arguments)
    device = capi.dev_gene_graph_create(*arguments)
    for key in ggb.GRAPH_KEYS:
        assert first[key].tobytes() == second[key].tobytes() == device[key].tobytes(), key
    ggb.assert_same_graph(device, ggb.reference(name), name)


def test_the_scratch_cache_is_only_a_cache():
    """A large call leaves large blocks in the cache; a small one after it, and one after the cache was emptied, agree."""
    for name in ("genes-1000", "edge-kinds", "genes-65"):
        ggb.assert_same_graph(capi.gene_graph_create(*ggb.arguments(ggb.case(name))), ggb.reference(name), name)
    capi.load().em2_dev_release_scratch()
    for name in ("edge-kinds", "genes-1000"):
        ggb.assert_same_graph(capi.gene_graph_create(*ggb.arguments(ggb.case(name))), ggb.reference(name), name + " after the release")


def _raw_create(entry, c):
    handle = ctypes.c_void_p(None)
    lib = capi.load()
    rc = getattr(lib, entry)(capi._ptr(c["pairs"]), capi._ptr(c["used"]), len(c["P"]), c["pairs"].shape[1], capi._ptr(c["P"]),
                             capi._ptr(c["S"]), len(c["S"]), c["threshold"], c["limit"] % 2 ** 64, ctypes.byref(handle))
    return rc, lib.em2_last_error().decode(), handle


def test_a_self_pair_and_a_partner_out_of_range_are_errors():
    entry = "em2_gene_graph_create"
    good = [[(1, 0.9)], [(0, 0.9), (2, 0.8)], [(1, 0.8)], []]
    rc, _, handle = _raw_create(entry, ggb.lists_to_case(good, 2, np.arange(4), np.arange(4), 0.5, 0))
    assert rc == 0 and handle.value
    capi.load().em2_gene_graph_free(handle)
    for lists, text in [
            ([[(1, 0.9)], [(0, 0.9), (1, 0.8)], [(1, 0.8)], []], "a stored pair names its own gene"),
            ([[(1, 0.9)], [(0, 0.9), (2, 0.8)], [(4, 0.8)], []], "a stored pair names a gene outside the pairs' gene set"),
            ([[(1, 0.9)], [(0, 0.9), (2, 0.8)], [(0xffffffff, 0.8)], []], "a stored pair names a gene outside the pairs' gene set"),
            # also below the threshold, where the walk would never come, and for a gene that is not in S
            ([[(1, 0.9)], [(0, 0.9), (2, 0.8)], [(1, 0.8), (2, 0.1)], []], "a stored pair names its own gene")]:
        for s_ids in (np.arange(4), np.arange(2)):
            rc, message, handle = _raw_create(entry, ggb.lists_to_case(lists, 2, np.arange(4), s_ids, 0.5, 0))
            assert (rc, message, handle.value) == (INVALID, entry + ": " + text, None)
    # a slot behind usedCount is not a stored pair
    c = ggb.lists_to_case(good, 2, np.arange(4), np.arange(4), 0.5, 0)
    c["pairs"][0, 1] = (0, 0.5)
    c["pairs"][3, 0] = (77, 0.5)
    ggb.assert_same_graph(capi.gene_graph_create(*ggb.arguments(c)), ggb.load().gene_graph(*ggb.arguments(c)), "unused slots")
    c["used"][3] = 3                                          # above k = 2
    rc, message, handle = _raw_create(entry, c)
    assert (rc, message, handle.value) == (INVALID, entry + ": a usedCount is above k", None)


def test_fuzz_against_the_restatement():
    restatement = ggb.load()
    for i in range(ggb.FUZZ_COUNT):
        arguments = ggb.arguments(ggb.fuzz_case(i))
        ggb.assert_same_graph(capi.gene_graph_create(*arguments), restatement.gene_graph(*arguments), "fuzz case %d" % i)


# ---- end to end through ExpressionMatrix ----

@pytest.fixture(scope="module")
def matrix(tmp_path_factory):
    cells, genes = 300, 200
    toc, g, c = synth.expression_matrix(cells, genes, density=0.15, cluster_count=4, seed=5)
    directory = str(tmp_path_factory.mktemp("gene_graph") / "data")
    files.create_directory(directory, genes, toc, capi.make_counts(g, c))
    files.add_gene_set(directory, "Tail", np.arange(150, 200, dtype=np.uint32))
    files.add_gene_set(directory, "Sparse", np.arange(3, 200, 7, dtype=np.uint32))
    files.add_gene_set(directory, "NoGenes", np.zeros(0, dtype=np.uint32))
    e = ExpressionMatrix(directory)
    e.findSimilarGenePairs0(similarGenePairsName="All", k=10, similarityThreshold=0.05)
    e.findSimilarGenePairs0(geneSetName="Sparse", similarGenePairsName="OfSparse", k=5, similarityThreshold=0.0)
    assert e.createGeneSetDifference("AllGenes", "Tail", "Head") is True
    yield e, directory
    e.close()


def _expected(directory, pairs_name, pairs_set, graph_set, threshold, k):
    _, pairs, used = files.read_similar_gene_pairs(directory, pairs_name)
    return ggb.load().gene_graph(pairs, used, np.asarray(pairs_set, dtype=np.uint32), np.asarray(graph_set, dtype=np.uint32), threshold, k)


def _lists(graph):
    offsets = graph["connectivityOffsets"].tolist()
    both = list(zip(graph["connectivityGenes"].tolist(), graph["connectivitySimilarities"].tolist()))
    return [both[offsets[v]:offsets[v + 1]] for v in range(len(offsets) - 1)]


@pytest.mark.parametrize("gene_set,pairs_name,k,threshold", [
    ("Head", "All", 3, 0.1), ("AllGenes", "All", 0, 0.2), ("Head", "All", -1, 0.15), ("Sparse", "All", 2, 0.05),
    ("AllGenes", "OfSparse", 4, 0.0), ("Head", "OfSparse", 1, 0.0)])
def test_facade_graph(matrix, capsys, gene_set, pairs_name, k, threshold):
    e, directory = matrix
    graph_genes = e.getGeneSetGenes(gene_set)
    pairs_genes = e.getGeneSetGenes({"All": "AllGenes", "OfSparse": "Sparse"}[pairs_name])
    theirs = _expected(directory, pairs_name, pairs_genes, graph_genes, threshold, k)
    name = "%s-%s-%d" % (gene_set, pairs_name, k)
    capsys.readouterr()
    e.createGeneGraph(geneGraphName=name, geneSetName=gene_set, similarGenePairsName=pairs_name, k=k, similarityThreshold=threshold)
    assert capsys.readouterr().out == "The gene graph has %d vertices and %d edges\nafter %d vertices were removed. \n" % (
        len(theirs["vertices"]), len(theirs["edgeGene0"]), theirs["removedCount"])
    assert len(theirs["edgeGene0"]) > 5
    if pairs_name == "OfSparse":                             # most genes of the graph's set have no stored list
        assert theirs["removedCount"] > 100
    assert name in e.getGeneGraphNames()
    connectivity = e.getGeneGraphConnectivity(name)
    expected = _lists(theirs)
    assert len(connectivity) == len(graph_genes)
    for mine, wanted in zip(connectivity, expected):
        assert [gene for gene, _ in mine] == [gene for gene, _ in wanted]
        assert all(type(gene) is int and type(similarity) is float for gene, similarity in mine)
        assert ggb.bits([s for _, s in mine]).tolist() == ggb.bits([s for _, s in wanted]).tolist()
    kept = set(theirs["vertices"].tolist())
    assert all((v in kept) == bool(connectivity[v]) for v in range(len(graph_genes)))           # removed genes: empty lists
    assert e.getGeneGraphVertices(name).tolist() == [graph_genes[v] for v in theirs["vertices"].tolist()]
    v0, v1, similarity = e.getGeneGraphEdges(name)
    assert np.array_equal(v0, theirs["edgeGene0"]) and np.array_equal(v1, theirs["edgeGene1"])
    assert np.array_equal(ggb.bits(similarity), ggb.bits(theirs["edgeSimilarity"]))
    e.removeGeneGraph(name)
    assert name not in e.getGeneGraphNames()


def test_facade_default_gene_set_is_all_genes(matrix, capsys):
    e, directory = matrix
    e.createGeneGraph("Default", similarGenePairsName="All", k=3, similarityThreshold=0.1)
    theirs = _expected(directory, "All", np.arange(200), np.arange(200), 0.1, 3)
    assert e.getGeneGraphConnectivity("Default") == [[(g, float(np.float32(s))) for g, s in row] for row in _lists(theirs)]
    e.removeGeneGraph("Default")
    capsys.readouterr()


def test_facade_errors_and_the_first_graph_stays(matrix, capsys):
    e, directory = matrix
    arguments = dict(similarGenePairsName="All", k=3, similarityThreshold=0.1)
    e.createGeneGraph(geneGraphName="Twice", geneSetName="Head", **arguments)
    first = e.getGeneGraphConnectivity("Twice")
    capsys.readouterr()
    # a second graph under the same name is built (its message is printed) and dropped: map::insert keeps the first
    e.createGeneGraph(geneGraphName="Twice", geneSetName="AllGenes", similarGenePairsName="All", k=0, similarityThreshold=0.3)
    other = _expected(directory, "All", np.arange(200), np.arange(200), 0.3, 0)
    assert capsys.readouterr().out == "The gene graph has %d vertices and %d edges\nafter %d vertices were removed. \n" % (
        len(other["vertices"]), len(other["edgeGene0"]), other["removedCount"])
    assert e.getGeneGraphConnectivity("Twice") == first and len(first) == 150 and e.getGeneGraphNames() == ["Twice"]
    # the name is checked against the SIGNATURE graphs, and with their text
    e.computeLshSignatures(lshName="Bits", lshCount=8)
    e.createSignatureGraph(signatureGraphName="Taken", lshName="Bits", minCellCount=1)
    for call_arguments, text in [
            (dict(geneGraphName="Taken", **arguments), "Signature graph Taken already exists."),
            (dict(geneGraphName="G", geneSetName="Missing", **arguments), "Gene set Missing does not exist."),
            (dict(geneGraphName="G", geneSetName="NoGenes", **arguments), "Gene set NoGenes is empty.")]:
        with pytest.raises(RuntimeError) as error:
            e.createGeneGraph(**call_arguments)
        assert str(error.value) == text
    e.removeSignatureGraph("Taken")
    # a missing or inconsistent SimilarGenePairs object: the reader's own errors
    for pairs_name in ("Missing",):
        with pytest.raises(RuntimeError) as error:
            e.createGeneGraph(geneGraphName="G", similarGenePairsName=pairs_name, k=3, similarityThreshold=0.1)
        with pytest.raises(RuntimeError) as readers:
            files.read_similar_gene_pairs(directory, pairs_name)
        assert str(error.value) == str(readers.value)
    assert e.getGeneGraphNames() == ["Twice"]
    e.removeGeneGraph("Twice")
    for call in (lambda: e.removeGeneGraph("Twice"), lambda: e.getGeneGraphConnectivity("Twice"),
                 lambda: e.getGeneGraphVertices("Twice"), lambda: e.getGeneGraphEdges("Twice")):
        with pytest.raises(RuntimeError) as error:
            call()
        assert str(error.value) == "Gene graph Twice does not exists."


def test_facade_inconsistent_pairs_object(matrix, capsys):
    """The gene set of the pairs changed after they were written: the reader's hash check speaks, for the graph as for the read."""
    e, directory = matrix
    files.add_gene_set(directory, "Moving", np.arange(0, 60, dtype=np.uint32))
    before = ExpressionMatrix(directory)
    before.findSimilarGenePairs0(geneSetName="Moving", similarGenePairsName="OfMoving", k=4, similarityThreshold=0.0)
    before.createGeneGraph("Fine", similarGenePairsName="OfMoving", k=2, similarityThreshold=0.0)
    assert before.getGeneGraphNames() == ["Fine"]
    before.close()
    files.add_gene_set(directory, "Moving", np.arange(1, 61, dtype=np.uint32))
    after = ExpressionMatrix(directory)
    with pytest.raises(RuntimeError) as error:
        after.createGeneGraph("Broken", similarGenePairsName="OfMoving", k=2, similarityThreshold=0.0)
    assert str(error.value) == ("Hash for gene set Moving is not consistent with the value at the time SimilarGenePairs object "
                                "OfMoving was created.")
    with pytest.raises(RuntimeError) as readers:
        files.read_similar_gene_pairs(directory, "OfMoving")
    assert str(readers.value) == str(error.value) and after.getGeneGraphNames() == []
    after.close()
    capsys.readouterr()
