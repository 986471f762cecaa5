"""compareCellGraphs and reuseCellGraphColors on a synthetic store that went through findSimilarPairs4, createCellGraph,
computeCellGraphLayout, createClusterGraph and createMetaDataFromClusterGraph: the comparison equals the restatement fed with
getCellGraphEdges, and the reused colours are the restatement's, proper, and what the SVG and the raster show."""
import numpy as np
import pytest

import draw_binding as db
import graph_compare_binding as gb
import synth
from expressionmatrix2_amd import ExpressionMatrix, capi, files
from expressionmatrix2_amd.expression_matrix import CATEGORY_PALETTE

pytestmark = pytest.mark.gpu

CELLS, GENES, SEED = 400, 600, 78
SIZE = 96


@pytest.fixture(scope="module")
def matrix(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("compare") / "data")
    toc, g, c = synth.expression_matrix(CELLS, GENES, density=0.05, cluster_count=4, seed=SEED)
    files.create_directory(d, GENES, toc, capi.make_counts(g, c))
    e = ExpressionMatrix(d)
    e.findSimilarPairs4(similarPairsName="P", k=20, similarityThreshold=0.2)
    e.createCellGraph("Loose", "AllCells", "P", similarityThreshold=0.3, k=10)
    e.createCellGraph("Tight", "AllCells", "P", similarityThreshold=0.45, k=6)
    e.createCellGraph("Again", "AllCells", "P", similarityThreshold=0.3, k=10)
    e.computeCellGraphLayout("Loose")
    yield e
    e.close()


def restated(e, name):
    """The graph as the restatement takes it, from the facade's public view of it: the cell ids of getCellGraphEdges over an
    identity vertex list of all cells the graph holds."""
    g = e._cell_graph(name)
    edges = e.getCellGraphEdges(name)
    cells = np.asarray(g["vertexCellIds"], dtype=np.uint32)
    position = {cell: at for at, cell in enumerate(cells.tolist())}
    return gb.graph(cells, [position[a] for a, _ in edges], [position[b] for _, b in edges], g["edgeSimilarity"])


def test_two_thresholds(matrix):
    r = matrix.compareCellGraphs("Loose", "Tight")
    status, reference = gb.load().compare(restated(matrix, "Loose"), restated(matrix, "Tight"))
    assert status == gb.OK
    mine = {key: r[key] for key in ("commonVertexCount", "commonEdgeCount", "commonIdenticalEdgeCount")}
    mine.update(edgeCount0=r["graphs"][0]["edgeCount"], edgeCount1=r["graphs"][1]["edgeCount"], binDelta=r["histogramDelta"],
                binCount=r["histogramCount"])
    gb.assert_same_comparison(mine, reference, "Loose against Tight")
    assert 0 < r["commonEdgeCount"] < r["graphs"][0]["edgeCount"] and r["commonVertexCount"] > 50
    assert r["commonIdenticalEdgeCount"] == r["commonEdgeCount"]          # the same SimilarPairs: the same similarities
    assert r["histogramDelta"].tolist() == [0.0] and not np.signbit(r["histogramDelta"][0])
    for which, (name, threshold, k) in enumerate((("Loose", 0.3, 10), ("Tight", 0.45, 6))):
        g = matrix._cell_graph(name)
        assert r["graphs"][which] == {"cellSetName": "AllCells", "similarPairsName": "P", "similarityThreshold": threshold,
                                      "maxConnectivity": k, "vertexCount": g["vertexCount"],
                                      "isolatedRemovedVertexCount": g["isolatedRemovedVertexCount"],
                                      "edgeCount": r["graphs"][which]["edgeCount"]}
        assert r["graphs"][which]["edgeCount"] <= g["edgeCount"]


def test_a_graph_with_itself_under_another_name(matrix):
    r = matrix.compareCellGraphs("Loose", "Again")
    edges = r["graphs"][0]["edgeCount"]
    assert edges == r["graphs"][1]["edgeCount"] == r["commonEdgeCount"] == r["commonIdenticalEdgeCount"] > 50
    assert r["commonVertexCount"] == matrix._cell_graph("Loose")["vertexCount"]
    assert gb.bits(r["histogramDelta"]).tolist() == [0] and r["histogramCount"].tolist() == [edges]
    with pytest.raises(RuntimeError) as error:
        matrix.compareCellGraphs("Loose", "Loose")
    assert str(error.value) == "Comparison of a cell graph with itself requested. "
    with pytest.raises(RuntimeError) as error:
        matrix.compareCellGraphs("Loose", "Missing")
    assert str(error.value) == "Did not find one or both of the cell graphs to be compared."


def test_reused_colours(matrix, tmp_path):
    e = matrix
    g = e._cell_graph("Loose")
    with pytest.raises(RuntimeError, match='is not a "category" colouring'):
        e.reuseCellGraphColors("Loose")
    # 29 categories that follow the graph: strips of the layout by x, so that a strip's neighbours are mostly the strips next to it
    strip = np.empty(g["vertexCount"], dtype=np.int64)
    strip[np.argsort(g["layout"][0], kind="stable")] = np.arange(g["vertexCount"]) * 29 // g["vertexCount"]
    for cell, s in zip(g["vertexCellIds"].tolist(), strip.tolist()):
        e.setCellMetaData(cell, "Patch", "p%02d" % s)
    before = e.computeCellGraphColors("Loose", "byMetaData", metaDataName="Patch", metaDataMeaning="category")
    assert len(before["frequencyTable"]) == 29 and before["couldNotColor"] > 0
    r = e.reuseCellGraphColors("Loose")
    assert r["couldNotColor"] < before["couldNotColor"]
    v0, v1 = g["edgeVertices"]
    status, reference = gb.load().group_colors(before["groups"], v0, v1)
    assert status == gb.OK
    gb.assert_proper(reference, "the restatement")
    assert r["colorTable"].dtype == np.uint32 and np.array_equal(r["colorTable"], reference["colorTable"])
    assert np.array_equal(r["groups"], before["groups"]) and r["frequencyTable"] == before["frequencyTable"]
    # no edge joins two groups of one colour index
    groups = r["groups"]
    between = groups[v0] != groups[v1]
    assert between.any() and (r["colorTable"][groups[v0]][between] != r["colorTable"][groups[v1]][between]).all()
    # the colours are the palette's entries of the table, "black" from index 12 on
    expected = {group: (CATEGORY_PALETTE[c] if c < 12 else "black") for group, c in enumerate(r["colorTable"].tolist())}
    assert r["groupColors"] == expected and r["colors"] == [expected[group] for group in groups.tolist()]
    assert r["couldNotColor"] == sum(1 for c in r["colors"] if c == "black")
    assert len(set(r["colors"])) > 1 and r["colors"] != before["colors"]
    # the SVG and the raster show them
    x, y = g["layout"]
    path = str(tmp_path / "reused.svg")
    e.writeCellGraphSvg("Loose", path)
    default = db.python_default_view(x, y, 600.)
    svg = db.python_svg(x, y, g["vertexCellIds"], v0, v1, False, 600., *default, "AllGenes", r["colors"], groups, r["groupColors"])
    with open(path, "rb") as f:
        assert f.read() == svg
    image = e.drawCellGraph("Loose", sizePixels=SIZE)
    restatement = db.load()
    xc, yc, half, radius = db.python_default_view(x, y, float(SIZE))[:4]
    order = np.argsort(groups, kind="stable")
    position = np.empty(len(order), dtype=np.uint32)
    position[order] = np.arange(len(order), dtype=np.uint32)
    top, hits = restatement.graph_draw(x[order], y[order], position[v0], position[v1], SIZE, xc, yc, half, radius)
    rgb = np.asarray([0 if c == "black" else int(c[1:], 16) for c in r["colors"]], dtype=np.uint32)
    assert np.array_equal(image, restatement.graph_compose(top, hits, rgb[order], 255))
    # a second call changes nothing
    again = e.reuseCellGraphColors("Loose")
    assert np.array_equal(again["colorTable"], r["colorTable"]) and again["colors"] == r["colors"]
