"""The yardstick of the gene graph tests, without a GPU: tests/native/em2_gene_graph_restatement.cpp (std::map vertex table,
std::set out-edges, std::list of edges, removal of the isolated vertices) against an independent Python statement of the
closed form on every shared case and on the fuzz cases; the three gene set operations of ExpressionMatrix (host only) against
Python's set; and the argument checks of the library's entries, none of which reaches a device."""
import ctypes

import numpy as np
import pytest

import gene_graph_binding as ggb
from expressionmatrix2_amd import capi

OK, INVALID, NO_DEVICE = 0, 1, 2


def closed_form(pairs, used, p_ids, s_ids, threshold, limit):
    """sel(v): the first `limit` stored pairs at or above the threshold whose partner is in S.  Edges, in insertion order: for v0
    ascending, for v1 in sel(v0) in order, unless v1 came earlier in sel(v0) or v1 < v0 and v0 is in sel(v1).  The connectivity
    is both directions of every edge, ordered by (vertex, neighbour)."""
    limit %= 2 ** 64
    p_of = {int(g): i for i, g in enumerate(p_ids)}
    s_of = {int(g): i for i, g in enumerate(s_ids)}
    sel = []
    for g in s_ids.tolist():
        mine = []
        if g in p_of:
            row = p_of[g]
            for j in range(int(used[row])):
                similarity = pairs[row, j]["similarity"]                 # np.float32
                if float(similarity) < threshold:                         # float promoted to double; false for a NaN
                    break
                partner = int(p_ids[int(pairs[row, j]["cell"])])
                if partner not in s_of:
                    continue
                mine.append((s_of[partner], similarity))
                if len(mine) == limit:
                    break
        sel.append(mine)
    chosen = [[v for v, _ in mine] for mine in sel]
    edges = []
    for v0, mine in enumerate(sel):
        for j, (v1, similarity) in enumerate(mine):
            if v1 in chosen[v0][:j] or (v1 < v0 and v0 in chosen[v1]):
                continue
            edges.append((v0, v1, similarity))
    directed = sorted([(a, b, s) for a, b, s in edges] + [(b, a, s) for a, b, s in edges], key=lambda r: (r[0], r[1]))
    degree = np.bincount(np.array([r[0] for r in directed], dtype=np.int64), minlength=len(s_ids))
    vertices = np.nonzero(degree)[0]
    return {
        "vertices": vertices.astype(np.uint32),
        "edgeGene0": np.array([e[0] for e in edges], dtype=np.uint32),
        "edgeGene1": np.array([e[1] for e in edges], dtype=np.uint32),
        "edgeSimilarity": np.array([e[2] for e in edges], dtype=np.float32),
        "connectivityOffsets": np.concatenate([[0], np.cumsum(degree)]).astype(np.uint64),
        "connectivityGenes": np.array([r[1] for r in directed], dtype=np.uint32),
        "connectivitySimilarities": np.array([r[2] for r in directed], dtype=np.float32),
        "removedCount": len(s_ids) - len(vertices),
    }


@pytest.mark.parametrize("name", ggb.GRAPH_CASES)
def test_restatement_agrees_with_the_closed_form(name):
    ggb.assert_same_graph(closed_form(*ggb.arguments(ggb.case(name))), ggb.reference(name), name)


def test_restatement_agrees_with_the_closed_form_on_the_fuzz_cases():
    restatement = ggb.load()
    edges = 0
    for i in range(ggb.FUZZ_COUNT):
        arguments = ggb.arguments(ggb.fuzz_case(i))
        theirs = restatement.gene_graph(*arguments)
        ggb.assert_same_graph(closed_form(*arguments), theirs, "fuzz case %d" % i)
        edges += len(theirs["edgeGene0"])
    assert edges > 5 * ggb.FUZZ_COUNT


def _edges(graph):
    return list(zip(graph["edgeGene0"].tolist(), graph["edgeGene1"].tolist(), graph["edgeSimilarity"].tolist()))


def _lists(graph):
    offsets = graph["connectivityOffsets"].tolist()
    both = list(zip(graph["connectivityGenes"].tolist(), graph["connectivitySimilarities"].tolist()))
    return [both[offsets[v]:offsets[v + 1]] for v in range(len(offsets) - 1)]


def f32(x):
    return float(np.float32(x))


def test_the_cases_are_what_they_are_meant_to_be():
    for n in (1, 63, 64, 65, 257, 1000):
        c = ggb.case("genes-%d" % n)
        assert len(c["S"]) == len(c["P"]) == n and c["used"][0] == 0 and (n < 10 or c["used"][1] == c["pairs"].shape[1])
    assert ggb.reference("genes-1")["vertices"].tolist() == [] and ggb.reference("genes-1")["connectivityOffsets"].tolist() == [0, 0]
    assert len(ggb.reference("genes-1000")["edgeGene0"]) > 1000
    for spacing, consecutive in (("consecutive", True), ("gaps", False)):
        for kind in ggb.SET_KINDS:
            c = ggb.case("sets-%s-%s" % (kind, spacing))
            p, s = set(c["P"].tolist()), set(c["S"].tolist())
            assert {"equal": p == s, "subset": s < p, "superset": s > p, "interleaved": bool(p - s and s - p and p & s),
                    "disjoint": not p & s}[kind], (kind, spacing)
            assert (int(c["S"][-1] - c["S"][0]) == len(s) - 1) == consecutive, (kind, spacing)
            graph = ggb.reference("sets-%s-%s" % (kind, spacing))
            if kind == "disjoint":
                assert len(graph["vertices"]) == len(graph["edgeGene0"]) == 0 and not graph["connectivityOffsets"].any()
            else:
                assert len(graph["edgeGene0"]) > 10
    one, zero, negative = (ggb.reference("limit-" + which) for which in ("1", "0", "negative"))
    ggb.assert_same_graph(zero, negative, "no limit either way")
    assert len(one["edgeGene0"]) < len(zero["edgeGene0"])


def test_the_limit():
    last = ggb.reference("limit-on-the-last-pair")
    assert _edges(last) == [(0, 1, f32(0.9)), (0, 2, f32(0.8)), (0, 3, f32(0.7)), (4, 0, f32(0.9)), (4, 1, f32(0.8)), (4, 2, f32(0.7))]
    duplicate = ggb.reference("limit-reached-by-a-duplicate")
    assert _edges(duplicate) == [(0, 1, f32(0.9)), (1, 2, f32(0.8)), (4, 5, f32(0.9))]
    assert duplicate["vertices"].tolist() == [0, 1, 2, 4, 5] and duplicate["removedCount"] == 1


def test_the_threshold():
    equal, above, fifth = (ggb.reference("threshold-" + which) for which in ("equal", "ulp-above", "0.2"))
    stored = float(ggb.STORED)
    assert _edges(equal) == [(0, 1, f32(0.9)), (0, 2, stored), (4, 5, f32(0.9))]              # equal is kept
    assert _edges(above) == [(0, 1, f32(0.9)), (4, 5, f32(0.9))]                              # one ulp of the double above: cut
    # float32(0.2) is above the double 0.2 and stays; the float below it is cut
    assert _edges(fifth) == [(0, 1, f32(0.9)), (0, 2, stored), (0, 3, 0.5), (4, 5, f32(0.9)), (4, 6, f32(0.2))]
    nan = ggb.reference("nan")                               # a NaN is not below the threshold: kept, and the walk goes on
    assert nan["edgeGene0"].tolist() == [0, 0, 0, 5] and nan["edgeGene1"].tolist() == [1, 2, 3, 0]
    assert np.isnan(nan["edgeSimilarity"][[1, 3]]).all() and nan["edgeSimilarity"][2] == np.float32(0.7)
    assert nan["vertices"].tolist() == [0, 1, 2, 3, 5] and _lists(nan)[4] == []


def test_the_edges():
    kinds = ggb.reference("edge-kinds")
    assert _edges(kinds) == [(0, 1, f32(0.9)), (2, 3, f32(0.8)), (5, 4, f32(0.7))]
    asymmetric = ggb.reference("asymmetric")
    assert _edges(asymmetric) == [(0, 1, f32(0.9)), (3, 2, f32(0.7)), (5, 4, f32(0.6))]
    assert _lists(asymmetric) == [[(1, f32(0.9))], [(0, f32(0.9))], [(3, f32(0.7))], [(2, f32(0.7))], [(5, f32(0.6))], [(4, f32(0.6))]]


def test_the_isolated_vertices():
    incoming = ggb.reference("incoming-only")
    assert incoming["vertices"].tolist() == [0, 1, 2, 3, 4] and incoming["removedCount"] == 1
    assert _lists(incoming)[5] == [] and _lists(incoming)[3] == [(0, f32(0.7))]
    ring = ggb.reference("nothing-isolated")
    assert ring["removedCount"] == 0 and len(ring["edgeGene0"]) == 70 and np.all(np.diff(ring["connectivityOffsets"]) == 2)
    nothing = ggb.reference("everything-isolated")
    assert nothing["removedCount"] == 300 and len(nothing["vertices"]) == 0 and not nothing["connectivityOffsets"].any()
    hub = ggb.reference("hub")
    assert np.diff(hub["connectivityOffsets"]).tolist() == [599] + [1] * 599
    assert hub["connectivityGenes"][:599].tolist() == list(range(1, 600))


# ---- the gene set operations (host only) ----

@pytest.fixture(scope="module")
def matrix(tmp_path_factory):
    import synth
    from expressionmatrix2_amd import ExpressionMatrix, files
    genes = 40
    toc, g, counts = synth.expression_matrix(20, genes, density=0.2, cluster_count=2, seed=3)
    directory = str(tmp_path_factory.mktemp("gene_sets") / "data")
    files.create_directory(directory, genes, toc, capi.make_counts(g, counts))
    sets = {"Even": list(range(0, 40, 2)), "Thirds": list(range(0, 40, 3)), "Low": list(range(0, 12)), "High": list(range(30, 40)),
            "Gapped": [1, 2, 3, 17, 18, 30, 39], "Nothing": []}
    for name, ids in sets.items():
        files.add_gene_set(directory, name, np.array(ids, dtype=np.uint32))
    sets["AllGenes"] = list(range(genes))
    e = ExpressionMatrix(directory)
    yield e, sets
    e.close()


def _fold(sets, names, operation):
    out = set(sets[names[0]])
    for name in names[1:]:
        out = operation(out, set(sets[name]))
    return sorted(out)


@pytest.mark.parametrize("names", [("Even", "Thirds"), ("Even", "Thirds", "Low"), ("Gapped", "Even"), ("Low", "High"), ("Even", "Nothing"),
                                   ("Nothing",), ("AllGenes", "Gapped", "Thirds"), ("Even", "Even")])
def test_intersection_and_union(matrix, capsys, names):
    e, sets = matrix
    joined = ",".join(names)
    assert e.createGeneSetIntersection(joined, "I-" + joined) is True
    assert e.createGeneSetUnion(joined, "U-" + joined) is True
    assert capsys.readouterr().out == ""
    assert e.getGeneSetGenes("I-" + joined) == _fold(sets, names, set.intersection)
    assert e.getGeneSetGenes("U-" + joined) == _fold(sets, names, set.union)
    # the new sets are sets like any other: operands of the next call
    assert e.createGeneSetDifference("U-" + joined, "I-" + joined, "D-" + joined) is True
    assert e.getGeneSetGenes("D-" + joined) == sorted(set(_fold(sets, names, set.union)) - set(_fold(sets, names, set.intersection)))
    for prefix in "IUD":
        e.removeGeneSet(prefix + "-" + joined)


@pytest.mark.parametrize("name0,name1", [("Even", "Thirds"), ("Thirds", "Even"), ("Gapped", "Low"), ("Low", "AllGenes"), ("Nothing", "Even"),
                                         ("Even", "Nothing"), ("High", "Low")])
def test_difference(matrix, name0, name1):
    e, sets = matrix
    assert e.createGeneSetDifference(name0, name1, "Difference") is True
    assert e.getGeneSetGenes("Difference") == sorted(set(sets[name0]) - set(sets[name1]))
    e.removeGeneSet("Difference")


def test_an_empty_result_is_a_gene_set(matrix):
    e, _ = matrix
    assert e.createGeneSetIntersection("Low,High", "Empty") is True and e.getGeneSetGenes("Empty") == []
    assert e.createGeneSetUnion("Empty,Gapped", "Again") is True and e.getGeneSetGenes("Again") == [1, 2, 3, 17, 18, 30, 39]
    # the files are there for the next object that opens the directory
    from expressionmatrix2_amd import ExpressionMatrix
    other = ExpressionMatrix(e.directoryName)
    assert other.getGeneSetGenes("Empty") == [] and other.getGeneSetGenes("Again") == [1, 2, 3, 17, 18, 30, 39]
    other.close()
    e.removeGeneSet("Empty")
    e.removeGeneSet("Again")


def test_the_operations_return_false_and_print(matrix, capsys):
    e, _ = matrix
    for call, line in [
            (lambda: e.createGeneSetIntersection("Even,Thirds", "Low"), "Gene set Low already exists."),
            (lambda: e.createGeneSetUnion("Even,Thirds", "AllGenes"), "Gene set AllGenes already exists."),
            (lambda: e.createGeneSetDifference("Even", "Thirds", "High"), "Gene set High already exists."),
            (lambda: e.createGeneSetIntersection("Even,Missing,AlsoMissing", "New"), "gene set Missing does not exists."),
            (lambda: e.createGeneSetUnion("Missing", "New"), "gene set Missing does not exists."),
            (lambda: e.createGeneSetUnion("Even,,Thirds", "New"), "gene set  does not exists."),       # boost::split keeps the empty piece
            (lambda: e.createGeneSetUnion("Even, Thirds", "New"), "gene set  Thirds does not exists."),  # and trims nothing
            (lambda: e.createGeneSetIntersection("", "New"), "gene set  does not exists."),
            (lambda: e.createGeneSetDifference("Missing", "Even", "New"), "Gene set Missing does not exists."),
            (lambda: e.createGeneSetDifference("Even", "Missing", "New"), "Gene set Missing does not exists."),
            (lambda: e.createGeneSetDifference("Missing0", "Missing1", "New"), "Gene set Missing0 does not exists."),
            (lambda: e.createGeneSetDifference("Missing", "Even", "Low"), "Gene set Low already exists.")]:     # the output comes first
        assert call() is False
        assert capsys.readouterr().out == line + "\n"
    with pytest.raises(RuntimeError, match=r"^Gene set New does not exist\.$"):
        e.getGeneSetGenes("New")


# ---- the library's argument checks: return code and the whole text; nothing here reaches a device ----

def _call(name, *arguments):
    lib = capi.load()
    rc = getattr(lib, name)(*arguments)
    return rc, lib.em2_last_error().decode()


PAIRS = np.zeros((4, 2), dtype=capi.PAIR_DTYPE)
USED = np.zeros(4, dtype=np.uint32)
IDS = np.arange(4, dtype=np.uint32)


@pytest.mark.parametrize("name", ["em2_gene_graph_create", "em2_dev_gene_graph_create"])
def test_entry_argument_errors(name):
    handle = ctypes.c_void_p(None)
    p, u, ids = PAIRS.ctypes.data, USED.ctypes.data, IDS.ctypes.data
    unsorted, repeated = np.array([0, 2, 1, 3], dtype=np.uint32), np.array([0, 1, 1, 3], dtype=np.uint32)
    assert _call(name, p, u, 4, 2, ids, ids, 4, 0.5, 0, None) == (INVALID, name + ": null pointer")
    assert _call(name, p, u, 4, 2, ids, ids, 0, 0.5, 0, ctypes.byref(handle)) == (INVALID, name + ": graphGeneCount must be positive")
    for arguments in ((None, u, 4, 2, ids, ids, 4), (p, None, 4, 2, ids, ids, 4), (p, u, 4, 2, None, ids, 4), (p, u, 4, 2, ids, None, 4)):
        assert _call(name, *arguments, 0.5, 0, ctypes.byref(handle)) == (INVALID, name + ": null pointer")
    for bad in (unsorted, repeated):
        text = name + ": a gene set is not in strictly ascending order"
        assert _call(name, p, u, 4, 2, bad.ctypes.data, ids, 4, 0.5, 0, ctypes.byref(handle)) == (INVALID, text)
        assert _call(name, p, u, 4, 2, ids, bad.ctypes.data, 4, 0.5, 0, ctypes.byref(handle)) == (INVALID, text)
    if capi.device_count() == 0:
        assert _call(name, p, u, 4, 2, ids, ids, 4, 0.5, 0, ctypes.byref(handle)) == (
            NO_DEVICE, name + ": no HIP device is visible (this library has no CPU path)")
    assert not handle.value


def test_null_handles():
    assert _call("em2_gene_graph_sizes", None, None, None, None) == (INVALID, "em2_gene_graph_sizes: null pointer")
    assert _call("em2_gene_graph_get", *[None] * 8) == (INVALID, "em2_gene_graph_get: null pointer")
    capi.load().em2_gene_graph_free(None)


def test_facade_arguments_and_names(matrix):
    """What the facade decides before any device work: the required arguments, the names and the reference's look-ups."""
    e, _ = matrix
    with pytest.raises(TypeError, match="geneGraphName, similarGenePairsName, k and similarityThreshold are required"):
        e.createGeneGraph(geneGraphName="G", similarGenePairsName="Pairs", k=3)
    for bad in (2 ** 31, -2 ** 31 - 1, 1.5):
        with pytest.raises(ValueError, match="k must be an integer that fits an int"):
            e.createGeneGraph(geneGraphName="G", similarGenePairsName="Pairs", k=bad, similarityThreshold=0.5)
    for call in (lambda: e.removeGeneGraph("G"), lambda: e.getGeneGraphConnectivity("G"), lambda: e.getGeneGraphVertices("G"),
                 lambda: e.getGeneGraphEdges("G")):
        with pytest.raises(RuntimeError, match=r"^Gene graph G does not exists\.$"):
            call()
    assert e.getGeneGraphNames() == []
    with pytest.raises(RuntimeError, match=r"^Gene set Missing does not exist\.$"):
        e.createGeneGraph(geneGraphName="G", geneSetName="Missing", similarGenePairsName="Pairs", k=3, similarityThreshold=0.5)
    with pytest.raises(RuntimeError, match=r"^Gene set Nothing is empty\.$"):
        e.createGeneGraph(geneGraphName="G", geneSetName="Nothing", similarGenePairsName="Pairs", k=3, similarityThreshold=0.5)
    with pytest.raises(RuntimeError):                        # the reader's error for an object that is not there
        e.createGeneGraph(geneGraphName="G", similarGenePairsName="Pairs", k=3, similarityThreshold=0.5)
    assert e.getGeneGraphNames() == []
