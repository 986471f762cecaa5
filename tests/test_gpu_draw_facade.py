"""computeCellGraphColors, writeCellGraphSvg and drawCellGraph on a synthetic store that went through findSimilarPairs4,
createCellGraph, computeCellGraphLayout, createClusterGraph and createMetaDataFromClusterGraph: for every colouring option the SVG's
bytes equal the Python statement of CellGraph::writeSvg (tests/draw_binding.py), the image equals the restatement's raster and
composition, and the PNG decodes to the image."""
import numpy as np
import pytest

import draw_binding as db
import synth
from expressionmatrix2_amd import ExpressionMatrix, NormalizationMethod, capi, files

pytestmark = pytest.mark.gpu

CELLS, GENES, SEED = 400, 600, 77
SIZE = 96


@pytest.fixture(scope="module")
def restatement():
    return db.load()


@pytest.fixture(scope="module")
def matrix(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("draw") / "data")
    toc, g, c = synth.expression_matrix(CELLS, GENES, density=0.05, cluster_count=4, seed=SEED)
    files.create_directory(d, GENES, toc, capi.make_counts(g, c))
    files.add_gene_set(d, "Most", np.array([gene for gene in range(GENES) if gene % 11 != 4], dtype=np.uint32))
    e = ExpressionMatrix(d)
    e.findSimilarPairs4(geneSetName="Most", similarPairsName="P", k=20, similarityThreshold=0.2)
    e.createCellGraph("G", "AllCells", "P", similarityThreshold=0.3, k=10)
    with pytest.raises(RuntimeError) as error:
        e.drawCellGraph("G")
    assert str(error.value) == "Layout for graph G is not available."
    e.computeCellGraphLayout("G")
    e.createClusterGraph("G", "C", minClusterSize=5)
    e.createMetaDataFromClusterGraph("C", "Cluster")
    for cell in range(CELLS):
        e.setCellMetaData(cell, "Paint", "#%02x%02x%02x" % (cell % 256, (7 * cell) % 256, (cell // 3) % 256))
        e.setCellMetaData(cell, "Tissue", "t%d" % ((cell * cell) % 5))
        e.setCellMetaData(cell, "Score", "high" if cell % 17 == 0 else repr(0.25 * (cell % 23) - 2.))
    yield e
    e.close()


def graph_of(e):
    g = e._cell_graph("G")
    assert g["vertexCount"] > 50 and g["edgeCount"] > 50
    return g


def check_picture(e, restatement, tmp_path, name, result, rgb, **view):
    """The SVG, the image and the PNG of the colouring computed last."""
    g = graph_of(e)
    x, y = g["layout"]
    v0, v1 = g["edgeVertices"]
    cells = g["vertexCellIds"]
    # the SVG, with the page's defaults and with a view of its own
    for hide, svg_view in ((False, {}), (True, dict(svgSizePixels=450, xViewBoxCenter=0.5, yViewBoxCenter=-1.25, viewBoxHalfSize=3.,
                                                    vertexRadius=0.04, edgeThickness=0.003))):
        path = str(tmp_path / ("%s-%d.svg" % (name, hide)))
        e.writeCellGraphSvg("G", path, hideEdges=hide, **svg_view)
        size = float(svg_view.get("svgSizePixels", 600))
        default = db.python_default_view(x, y, size)
        arguments = [svg_view.get(key, default[at]) for at, key in enumerate(("xViewBoxCenter", "yViewBoxCenter", "viewBoxHalfSize",
                                                                              "vertexRadius", "edgeThickness"))]
        expected = db.python_svg(x, y, cells, v0, v1, hide, size, *arguments, "Most", result["colors"], result["groups"],
                                 result["groupColors"])
        with open(path, "rb") as f:
            assert f.read() == expected, "%s: the SVG differs" % name
    # the image
    path = str(tmp_path / (name + ".png"))
    for shade in (40, 255):
        image = e.drawCellGraph("G", fileName=path, sizePixels=SIZE, edgeShade=shade, **view)
        default = db.python_default_view(x, y, float(SIZE))
        xc, yc, half, radius = [view.get(key, default[at]) for at, key in enumerate(("xViewBoxCenter", "yViewBoxCenter", "viewBoxHalfSize",
                                                                                     "vertexRadius"))]
        order = np.argsort(result["groups"], kind="stable") if result["groupColors"] else np.arange(len(x))
        position = np.empty(len(order), dtype=np.uint32)
        position[order] = np.arange(len(order), dtype=np.uint32)
        top, hits = restatement.graph_draw(x[order], y[order], position[v0], position[v1], SIZE, xc, yc, half, radius)
        expected = restatement.graph_compose(top, hits, np.asarray(rgb, dtype=np.uint32)[order], shade)
        assert image.shape == (SIZE, SIZE, 4) and image.dtype == np.uint8
        assert np.array_equal(image, expected), "%s: the image differs" % name
        assert np.array_equal(db.read_png(path), image)
    assert (image[..., 3] == 255).all() and (image[..., :3] != 255).any()
    return image


def rgb_of_strings(colors):
    return [0 if c in ("", "black") else int(c[1:], 16) for c in colors]


def test_no_colouring(matrix, restatement, tmp_path):
    result = matrix.computeCellGraphColors("G")
    n = graph_of(matrix)["vertexCount"]
    assert result["colors"] == [""] * n and result["values"] is None and result["groupColors"] == {}
    image = check_picture(matrix, restatement, tmp_path, "none", result, [0] * n)
    assert set(map(tuple, image.reshape(-1, 4).tolist())) == {(255, 255, 255, 255), (0, 0, 0, 255)}


@pytest.mark.parametrize("method", (NormalizationMethod.L2, NormalizationMethod.none))
def test_by_gene_expression(matrix, restatement, tmp_path, method):
    g = graph_of(matrix)
    dense = matrix.getDenseExpressionMatrix("Most", "AllCells", method, dtype=np.float32)
    local = int(np.argmax((dense[g["vertexCellIds"]] > 0).sum(axis=0)))                  # the gene most vertices express
    gene = [x for x in range(GENES) if x % 11 != 4][local]
    result = matrix.computeCellGraphColors("G", "byGeneExpression", geneId=gene, normalizationMethod=method)
    column = dense[:, local]
    assert np.array_equal(result["values"], column[g["vertexCellIds"]].astype(np.float64))
    rgb, value_range = restatement.spectral_colors(result["values"])
    assert result["colors"] == db.color_strings(rgb) and (result["minValue"], result["maxValue"]) == (value_range[0], value_range[1])
    assert result["minValue"] == result["values"].min() and result["maxValue"] == result["values"].max() > 0.
    check_picture(matrix, restatement, tmp_path, "gene-%d" % method, result, rgb)
    for bad in (4, GENES + 5):                                    # outside the gene set: the reference's assertion
        with pytest.raises(RuntimeError, match="localGeneId != invalidGeneId"):
            matrix.computeCellGraphColors("G", "byGeneExpression", geneId=bad)
    with pytest.raises(RuntimeError) as error:
        matrix.computeCellGraphColors("G", "byGeneExpression")
    assert str(error.value) == "Gene not found."


def test_by_similarity_with_explicit_colour_bounds(matrix, restatement, tmp_path):
    g = graph_of(matrix)
    cell = int(g["vertexCellIds"][3])
    result = matrix.computeCellGraphColors("G", "bySimilarity", cellId=cell, minColorValue=0.1, maxColorValue=0.6)
    pairs = [matrix.computeCellSimilarity("Most", cell, int(c)) for c in g["vertexCellIds"][:40]]
    assert result["values"][:40].tolist() == pairs and result["values"][3] > 0.999
    rgb, value_range = restatement.spectral_colors(result["values"], 0.1, 0.6)
    assert result["colors"] == db.color_strings(rgb) and result["colors"][3] == "#00ff00"
    assert (result["minValue"], result["maxValue"]) == (value_range[0], value_range[1])
    check_picture(matrix, restatement, tmp_path, "similarity", result, rgb, vertexRadius=0.08)
    for bad in (-1, CELLS, None):
        with pytest.raises(RuntimeError) as error:
            matrix.computeCellGraphColors("G", "bySimilarity", cellId=bad)
        assert str(error.value) == "Invalid cell id."


def test_by_number(matrix, restatement, tmp_path):
    g = graph_of(matrix)
    result = matrix.computeCellGraphColors("G", "byMetaData", metaDataName="Score", metaDataMeaning="number")
    expected = np.array([db.NO_VALUE if c % 17 == 0 else 0.25 * (c % 23) - 2. for c in g["vertexCellIds"].tolist()])
    assert np.array_equal(result["values"], expected)
    rgb, _ = restatement.spectral_colors(expected)
    assert result["colors"] == db.color_strings(rgb) and "" in result["colors"]
    assert (result["minValue"], result["maxValue"]) == (-2., 3.5)
    check_picture(matrix, restatement, tmp_path, "number", result, rgb)


def test_by_colour(matrix, restatement, tmp_path):
    g = graph_of(matrix)
    result = matrix.computeCellGraphColors("G", "byMetaData", metaDataName="Paint", metaDataMeaning="color")
    assert result["colors"] == ["#%02x%02x%02x" % (c % 256, (7 * c) % 256, (c // 3) % 256) for c in g["vertexCellIds"].tolist()]
    check_picture(matrix, restatement, tmp_path, "colour", result, rgb_of_strings(result["colors"]))
    # a colour name goes into the SVG as it is, and is refused by the raster
    cell = int(g["vertexCellIds"][5])
    matrix.setCellMetaData(cell, "Paint", "red")
    try:
        result = matrix.computeCellGraphColors("G", "byMetaData", metaDataName="Paint", metaDataMeaning="color")
        matrix.writeCellGraphSvg("G", str(tmp_path / "named.svg"))
        assert b" fill='red'>" in (tmp_path / "named.svg").read_bytes()
        with pytest.raises(ValueError, match="'red'"):
            matrix.drawCellGraph("G", sizePixels=SIZE)
    finally:
        matrix.setCellMetaData(cell, "Paint", "#000000")


@pytest.mark.parametrize("field", ("Cluster", "Tissue"))
def test_by_category_in_the_painter_order_of_the_groups(matrix, restatement, tmp_path, field):
    g = graph_of(matrix)
    result = matrix.computeCellGraphColors("G", "byMetaData", metaDataName=field)
    values = [matrix.getCellMetaDataValue(c, field) for c in g["vertexCellIds"].tolist()]
    groups, group_colors, table, could_not = db.python_category(values)
    assert (result["groups"].tolist(), result["groupColors"], result["frequencyTable"], result["couldNotColor"]) == \
        (groups, group_colors, table, could_not)
    assert len(table) >= 2 and sum(count for count, _ in table) == g["vertexCount"]
    rgb = rgb_of_strings([group_colors[group] for group in groups])
    # discs of a twelfth of the view: many pixels are shared by vertices of two groups
    x, y = g["layout"]
    view = dict(vertexRadius=db.python_default_view(x, y, float(SIZE))[2] / 6.)
    image = check_picture(matrix, restatement, tmp_path, "category-" + field, result, rgb, **view)
    # in vertex order another vertex would be on top somewhere: there the image shows the later GROUP, not the later vertex
    xc, yc, half, _ = db.python_default_view(x, y, float(SIZE))[:4]
    none = np.zeros(0, dtype=np.uint32)
    top, _ = restatement.graph_draw(x, y, none, none, SIZE, xc, yc, half, view["vertexRadius"])
    in_vertex_order = restatement.graph_compose(top, np.zeros_like(top), np.asarray(rgb, dtype=np.uint32), 255)
    differs = np.argwhere((image[..., :3] != in_vertex_order[..., :3]).any(axis=2) & (top > 0))
    edge_free = [(j, i) for j, i in differs.tolist()]
    assert len(edge_free) > 0, "no pixel tells the two orders apart"
    order = np.argsort(np.asarray(groups), kind="stable")
    painter_top, _ = restatement.graph_draw(x[order], y[order], none, none, SIZE, xc, yc, half, view["vertexRadius"])
    j, i = edge_free[0]
    winner, loser = int(order[painter_top[j, i] - 1]), int(top[j, i] - 1)
    assert groups[winner] > groups[loser] and winner < loser
    assert image[j, i, :3].tolist() == [(rgb[winner] >> 16) & 255, (rgb[winner] >> 8) & 255, rgb[winner] & 255]
