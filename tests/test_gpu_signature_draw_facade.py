"""computeSignatureGraphLayout, computeSignatureGraphColors, writeSignatureGraphSvg and drawSignatureGraph of the facade on a
small store with meta data of 3, 15 and 40 values, against tests/native/em2_signature_draw_restatement.cpp and the Python
statements of tests/signature_draw_binding.py, which tests/test_signature_draw_cpu.py holds against one another."""
import numpy as np
import pytest

import draw_binding as db
import signature_draw_binding as sb
import synth
from expressionmatrix2_amd import ExpressionMatrix, capi, files

pytestmark = pytest.mark.gpu

CELLS = 600
KEYS = ("sliceOffsets", "sliceColor", "sliceCells", "sliceFraction")


@pytest.fixture(scope="module")
def restatement():
    return sb.load()


def field_values():
    rng = np.random.default_rng(21)
    forty = np.repeat(np.arange(40), 15)                         # 40 values of 15 cells each over the whole store: many ties
    return {
        "Three": ["abc"[v] for v in rng.choice(3, CELLS, p=[0.6, 0.3, 0.1])],
        "Fifteen": ["type%02d" % v for v in rng.integers(0, 15, CELLS)],
        "Forty": ["v%02d" % v for v in rng.permutation(forty)],
        "Sparse": ["x" if v else None for v in rng.integers(0, 2, CELLS)],        # None: the cell does not have the field
    }


@pytest.fixture(scope="module")
def matrix(tmp_path_factory):
    genes = 200
    toc, g, c = synth.expression_matrix(CELLS, genes, density=0.1, cluster_count=4, seed=11)
    directory = str(tmp_path_factory.mktemp("signature_draw") / "data")
    files.create_directory(directory, genes, toc, capi.make_counts(g, c))
    files.add_cell_set(directory, "Odd", np.arange(1, CELLS, 2, dtype=np.uint32))
    e = ExpressionMatrix(directory)
    e.computeLshSignatures(lshName="All8", lshCount=8)
    e.computeLshSignatures(cellSetName="Odd", lshName="Odd8", lshCount=8)
    for name, values in field_values().items():
        for cell, value in enumerate(values):
            if value is not None:
                e.setCellMetaData(cell, name, value)
    e.setCellMetaData(7, "Sparse", "")                           # a stored "" and a missing field are one value
    e.createSignatureGraph(signatureGraphName="All", lshName="All8", minCellCount=1)
    e.createSignatureGraph(signatureGraphName="Odd", cellSetName="Odd", lshName="Odd8", minCellCount=2)
    for name in ("All", "Odd"):
        e.computeSignatureGraphLayout(name)
    yield e
    e.close()


def vertex_values(e, graph, field):
    """The field's value of every cell of every vertex, in stored order, and the vertices' cell counts."""
    values = field_values().get(field)
    _, counts = e.getSignatureGraphVertices(graph)
    per_vertex = []
    for v in range(len(counts)):
        cells = e.getSignatureGraphCells(graph, v)[1].tolist()
        per_vertex.append([("" if values is None or values[cell] is None or (field == "Sparse" and cell == 7) else values[cell]) for cell in cells])
    return per_vertex, counts


def expected_category(restatement, per_vertex):
    flat = [value for vertex in per_vertex for value in vertex]
    table, rank = restatement.value_table(flat)
    offsets = np.concatenate([[0], np.cumsum([len(v) for v in per_vertex])]).astype(np.uint64)
    colors = np.minimum(np.arange(len(table)), 12).astype(np.uint8)
    return table, restatement.census(offsets, np.arange(len(flat), dtype=np.uint32), rank, colors)


def test_layout(matrix):
    e = matrix
    x, y = e.getSignatureGraphLayout("All")
    v0, v1 = e.getSignatureGraphEdges("All")
    vertices = len(e.getSignatureGraphVertices("All")[1])
    assert vertices >= 40 and len(v0) > 0 and x.dtype == np.float64 and x.shape == y.shape == (vertices,)
    expected = capi.graph_layout(vertices, v0, v1, capi.LayoutParameters(seed=231, maxIterationCount=300, tolerance=0.01, gravity=0.02))
    assert np.array_equal(x, expected[0].astype(np.float64)) and np.array_equal(y, expected[1].astype(np.float64))
    x[0] = 1e9                                                   # a copy
    e.computeSignatureGraphLayout("All", seed=5, repulsion="pyramid", levels="multi")        # computed once: nothing happens
    assert np.array_equal(e.getSignatureGraphLayout("All")[1], y) and e.getSignatureGraphLayout("All")[0][0] != 1e9
    e.createSignatureGraph(signatureGraphName="Other", lshName="All8", minCellCount=1)
    try:
        for call in (lambda: e.getSignatureGraphLayout("Other"), lambda: e.writeSignatureGraphSvg("Other", "unused.svg"),
                     lambda: e.drawSignatureGraph("Other")):
            with pytest.raises(RuntimeError) as error:
                call()
            assert str(error.value) == "Layout for signature graph Other is not available."
        with pytest.raises(ValueError, match="repulsion"):
            e.computeSignatureGraphLayout("Other", repulsion="none")
        with pytest.raises(ValueError, match="levels"):
            e.computeSignatureGraphLayout("Other", levels="two")
        e.computeSignatureGraphLayout("Other", repulsion="pyramid", levels="multi", maxIterationCount=20)
        assert np.isfinite(e.getSignatureGraphLayout("Other")[0]).all()
    finally:
        e.removeSignatureGraph("Other")
    for call in (lambda: e.computeSignatureGraphLayout("Missing"), lambda: e.getSignatureGraphLayout("Missing"),
                 lambda: e.computeSignatureGraphColors("Missing"), lambda: e.writeSignatureGraphSvg("Missing", "unused.svg"),
                 lambda: e.drawSignatureGraph("Missing")):
        with pytest.raises(RuntimeError) as error:
            call()
        assert str(error.value) == "Signature graph Missing does not exists."


@pytest.mark.parametrize("graph,field", [("All", "Three"), ("All", "Fifteen"), ("Odd", "Fifteen"), ("All", "Forty"), ("Odd", "Forty"),
                                         ("All", "Sparse"), ("Odd", "No such field")])
def test_category_colours(restatement, matrix, graph, field):
    e = matrix
    per_vertex, counts = vertex_values(e, graph, field)
    table, census = expected_category(restatement, per_vertex)
    result = e.computeSignatureGraphColors(graph, "byMetaData", field)
    for key in KEYS:
        assert result[key].tobytes() == census[key].tobytes(), key
    palette = sb.PALETTE
    assert result["valueTable"] == [(value, cells, palette[min(rank, 12)]) for rank, (value, cells) in enumerate(table)]
    assert result["colors"] == sb.slice_strings(census["sliceColor"])
    assert np.array_equal(np.add.reduceat(result["sliceCells"], result["sliceOffsets"][:-1].astype(np.int64)), counts.astype(np.uint32))
    if field == "Three":
        assert [value for value, _, _ in result["valueTable"]] == ["a", "b", "c"] and (np.diff(result["sliceOffsets"]) > 1).any()
    if field == "Forty" and graph == "All":
        assert len(table) == 40 and sum(1 for _, _, colour in result["valueTable"] if colour == "black") == 28
        cells = [n for _, n in table]
        assert len(set(cells)) < len(cells)                      # ties, in std::sort's order
    if field == "Sparse":
        assert sorted(value for value, _, _ in result["valueTable"]) == ["", "x"]
    if field == "No such field":
        assert result["valueTable"] == [("", int(counts.sum()), "#00ff00")] and set(result["colors"]) == {"#00ff00"}


def test_random_and_black_colours_and_the_two_that_are_not_implemented(restatement, matrix):
    e = matrix
    _, counts = e.getSignatureGraphVertices("All")
    n = len(counts)
    result = e.computeSignatureGraphColors("All")
    assert result["colors"] == capi.color_strings(restatement.random_colors(n)[0]) and result["colors"][0] == "#9a3c22"
    assert np.array_equal(result["sliceOffsets"], np.arange(n + 1)) and np.array_equal(result["sliceCells"], counts)
    assert (result["sliceFraction"] == 1.).all() and result["sliceColor"] is None and result["valueTable"] == []
    assert e.computeSignatureGraphColors("All", "noColoring")["colors"] == ["black"] * n
    for meaning, text in (("color", "Signature graph coloring by meta data interpreted as color is not implemented."),
                          ("number", "Signature graph coloring by meta data interpreted as number is not implemented.")):
        with pytest.raises(RuntimeError) as error:
            e.computeSignatureGraphColors("All", "byMetaData", "Three", meaning)
        assert str(error.value) == text
    with pytest.raises(TypeError):
        e.computeSignatureGraphColors("All", "byMetaData")


def svg_arguments(e, graph):
    x, y = e.getSignatureGraphLayout(graph)
    v0, v1 = e.getSignatureGraphEdges(graph)
    return x, y, e.getSignatureGraphVertices(graph)[1], v0, v1


def test_svg(restatement, matrix, tmp_path):
    e = matrix
    arrays = svg_arguments(e, "All")
    counts = arrays[2]
    assert len(counts) >= 40 and len(set(counts.tolist())) < len(counts)          # repeated cell counts: std::sort's tie order
    e.createSignatureGraph(signatureGraphName="Plain", lshName="All8", minCellCount=1)
    e.computeSignatureGraphLayout("Plain")
    try:
        parameters = e.writeSignatureGraphSvg("Plain", str(tmp_path / "plain.svg"))
        theirs, their_parameters = restatement.svg(str(tmp_path / "r.svg"), *arrays)
        mine = (tmp_path / "plain.svg").read_bytes()
        assert mine == theirs and mine.count(b"<circle") == len(counts) == mine.count(b"fill='black'") and b"<path" not in mine
        assert tuple(parameters[k] for k in ("xCenter", "yCenter", "halfViewBoxSize", "pixelSize")) == their_parameters
        image = e.drawSignatureGraph("Plain", sizePixels=64, hideEdges=True)          # before any colouring: black on white
        assert set(np.unique(image[..., :3]).tolist()) == {0, 255} and (image[..., 3] == 255).all()
    finally:
        e.removeSignatureGraph("Plain")
    for option, field in (("byMetaData", "Three"), ("byMetaData", "Fifteen"), ("random", None)):
        coloring = e.computeSignatureGraphColors("All", option, field)
        pies = dict(slice_offsets=coloring["sliceOffsets"], slice_colors=coloring["colors"], slice_fraction=coloring["sliceFraction"])
        for options, mine_options in ((dict(), dict()),
                                      (dict(hide_edges=True, size=830., x_shift=0.5, y_shift=-1.25, zoom=2., vertex_size=0.7, edge_thickness=3.),
                                       dict(hideEdges=True, svgSizePixels=830., xShift=0.5, yShift=-1.25, zoomFactor=2., vertexSizeFactor=0.7,
                                            edgeThicknessFactor=3.))):
            theirs, their_parameters = restatement.svg(str(tmp_path / "r.svg"), *arrays, **dict(pies, **options))
            parameters = e.writeSignatureGraphSvg("All", str(tmp_path / "l.svg"), **mine_options)
            assert (tmp_path / "l.svg").read_bytes() == theirs, (option, field)
            assert tuple(parameters[k] for k in ("xCenter", "yCenter", "halfViewBoxSize", "pixelSize")) == their_parameters
        assert (b"<path" in theirs) == (option == "byMetaData")


def expected_image(restatement, e, graph, coloring, size, shade, hide=False, x_shift=0., y_shift=0., zoom=1., vertex_size=1.):
    x, y, counts, v0, v1 = svg_arguments(e, graph)
    xc, yc, half, _, box = sb.python_signature_view(x, y, counts, size, x_shift, y_shift, zoom)
    radius = np.asarray([vertex_size * (0.03 * box * np.sqrt(float(n) / float(counts.max()))) for n in counts.tolist()])
    order = restatement.order_by_count(counts).astype(np.int64)
    position = np.empty(len(order), dtype=np.uint32)
    position[order] = np.arange(len(order), dtype=np.uint32)
    offsets = coloring["sliceOffsets"].astype(np.int64)
    pick = np.concatenate([np.arange(offsets[v], offsets[v + 1]) for v in order])
    new_offsets = np.concatenate([[0], np.cumsum(np.diff(offsets)[order])]).astype(np.uint64)
    bx, by, arc = restatement.pie_boundaries(new_offsets, coloring["sliceFraction"][pick])
    layers = restatement.graph_draw_pies(x[order], y[order], radius[order], position[v0], position[v1], size, xc, yc, half, new_offsets,
                                         bx, by, arc, hide)
    rgb = np.asarray([0 if s == "black" else int(s[1:], 16) for s in coloring["colors"]], dtype=np.uint32)[pick]
    return db.python_compose(layers[1], layers[2], rgb, shade)


def test_image_and_png(restatement, matrix, tmp_path):
    e = matrix
    coloring = e.computeSignatureGraphColors("All", "byMetaData", "Fifteen")
    image = e.drawSignatureGraph("All", str(tmp_path / "a.png"), sizePixels=200)
    assert image.shape == (200, 200, 4) and image.dtype == np.uint8
    assert np.array_equal(image, expected_image(restatement, e, "All", coloring, 200, 255))
    assert np.array_equal(db.read_png(str(tmp_path / "a.png")), image)
    seen = {tuple(p) for p in image.reshape(-1, 4)[:, :3].tolist()}
    assert len(seen & {tuple(int(s[i:i + 2], 16) for i in (1, 3, 5)) for s in sb.PALETTE[:12]}) >= 3      # pies of several colours
    image = e.drawSignatureGraph("All", sizePixels=97, edgeShade=60, hideEdges=False, xShift=0.5, yShift=-0.75, zoomFactor=2.5, vertexSizeFactor=3.)
    assert np.array_equal(image, expected_image(restatement, e, "All", coloring, 97, 60, False, 0.5, -0.75, 2.5, 3.))
    coloring = e.computeSignatureGraphColors("Odd", "random")
    image = e.drawSignatureGraph("Odd", sizePixels=64, hideEdges=True)
    assert np.array_equal(image, expected_image(restatement, e, "Odd", coloring, 64, 255, True))
    stored = e._signatureGraphs["Odd"]["coloring"]["colors"]
    kept, stored[0] = stored[0], "red"
    try:
        with pytest.raises(ValueError, match="'red'"):
            e.drawSignatureGraph("Odd", sizePixels=64)
    finally:
        stored[0] = kept
    with pytest.raises(RuntimeError, match="sizePixels"):
        e.drawSignatureGraph("Odd", sizePixels=0)
