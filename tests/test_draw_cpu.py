"""The restatement of the drawing entries (tests/native/em2_draw_restatement.cpp) against an independent numpy / Python statement
of the same definitions (tests/draw_binding.py): a set of covered pixels per vertex, a Python loop over k per edge, float64
numpy for the colours, '%g' for the SVG's numbers.  The GPU tests then hold the kernels against the restatement.  Also what
of the feature is host code: the SVG writer of the library, the number a meta data value stands for, the categories' order
and palette, the reference's coordinate range, and the PNG."""
import os

import numpy as np
import pytest

import draw_binding as db
import fsp0_binding
from expressionmatrix2_amd import ExpressionMatrix, capi, expression_matrix, files


@pytest.fixture(scope="module")
def restatement():
    return db.load()


def raster_cases():
    """name -> (x, y, v0, v1, S, xc, yc, half, radius).  The view is [0, 8) x [0, 8) at 16 pixels unless said: a pixel is 0.5."""
    rng = np.random.default_rng(3)
    cases = {}
    x = np.array([0.25, 1.0, 8.0, -1.0, 9.5, 4.0, 4.0, 1e30, -1e30])
    y = np.array([0.25, 2.0, 8.0, -1.0, 3.0, 4.0, 4.0, 1.0, 1.0])
    edges = np.array([[0, 1], [1, 0], [0, 2], [3, 4], [5, 6], [1, 7], [8, 4], [2, 3], [0, 5], [5, 0]], dtype=np.uint32)
    for name, radius in (("radius-0", 0.), ("radius-1.5px", 0.75), ("radius-5px", 2.5), ("radius-40px", 20.)):
        cases[name] = (x, y, edges[:, 0], edges[:, 1], 16, 4., 4., 4., radius)
    n = 40
    cases["random"] = (rng.random(n) * 12. - 2., rng.random(n) * 12. - 2., rng.integers(0, n, 90).astype(np.uint32),
                       rng.integers(0, n, 90).astype(np.uint32), 33, 4., 4., 4., 0.4)
    cases["one-pixel"] = (np.array([0.1, 0.9, 3.]), np.array([0.5, 0.2, 0.5]), np.array([0, 0], dtype=np.uint32),
                          np.array([1, 2], dtype=np.uint32), 1, 0.5, 0.5, 0.5, 0.1)
    cases["off-centre"] = (rng.random(n) * 3., rng.random(n) * 3., rng.integers(0, n, 60).astype(np.uint32),
                           rng.integers(0, n, 60).astype(np.uint32), 21, 1.7, 0.9, 1.3, 0.11)
    return cases


@pytest.mark.parametrize("name", sorted(raster_cases()))
def test_raster_restatement_equals_the_python_statement(restatement, name):
    x, y, v0, v1, size, xc, yc, half, radius = raster_cases()[name]
    for hide in (False, True):
        mine = restatement.graph_draw(x, y, v0, v1, size, xc, yc, half, radius, hide)
        theirs = db.python_raster(x, y, v0, v1, size, xc, yc, half, radius, hide)
        assert np.array_equal(mine[0], theirs[0]) and np.array_equal(mine[1], theirs[1]), (name, hide)
        assert not hide or not mine[1].any()
    assert mine[0].any() or name == "one-pixel" or radius == 0.


def test_raster_restatement_refuses_what_the_entry_refuses(restatement):
    x, y = np.array([1., 2.]), np.array([1., 2.])
    none = np.zeros(0, dtype=np.uint32)
    assert restatement.graph_draw(x, y, none, none, 16, 4., 4., 4., 0.5) is not None
    assert restatement.graph_draw(np.array([1., np.nan]), y, none, none, 16, 4., 4., 4., 0.5) is None
    assert restatement.graph_draw(x, np.array([np.inf, 1.]), none, none, 16, 4., 4., 4., 0.5) is None
    assert restatement.graph_draw(x, y, none, none, 16, 4., 4., 0., 0.5) is None
    assert restatement.graph_draw(x, y, none, none, 16, 4., 4., 4., 128.5) is None          # 257 pixels
    assert restatement.graph_draw(x, y, none, none, 16, 4., 4., 4., 128.) is not None        # 256 pixels
    assert restatement.graph_draw(x, y, np.array([0], dtype=np.uint32), np.array([2], dtype=np.uint32), 16, 4., 4., 4., 0.5) is None


def test_compose_restatement_equals_the_python_statement(restatement):
    top = np.array([[0, 0, 1, 2], [0, 3, 3, 0], [0, 0, 0, 0], [2, 1, 0, 0]], dtype=np.uint32)
    hits = np.array([[0, 1, 0, 5], [2, 0, 7, 3], [255, 256, 1000, 0], [0, 1, 1, 0]], dtype=np.uint32)
    rgb = np.array([0x123456, db.COLOR_NONE, db.COLOR_BLACK | 0], dtype=np.uint32)
    for shade in (1, 100, 255):
        mine = restatement.graph_compose(top, hits, rgb, shade)
        assert np.array_equal(mine, db.python_compose(top, hits, rgb, shade)), shade
        assert mine[0, 0].tolist() == [255] * 4 and mine[0, 2].tolist() == [0x12, 0x34, 0x56, 255] and (mine[..., 3] == 255).all()
        assert mine[0, 1].tolist() == [255 - shade] * 3 + [255] and mine[0, 3].tolist() == [0, 0, 0, 255]


def color_cases():
    big = db.NO_VALUE
    just_below = np.nextafter(0.25, 0.)          # value * 2 * 255 just below 127.5's neighbour integers
    cases = {
        "ramp": (np.array([0., 0.25, 0.5, 0.75, 1., 0.1, 0.9, 1. / 510., np.nextafter(1. / 510., 0.), 2. / 510., just_below]), None, None),
        "clips": (np.array([-3., 0., 1., 2., 5., 9.]), 1., 5.),
        "narrow": (np.linspace(-1., 1., 41), -0.5, 0.25),
        "only-min": (np.linspace(0., 10., 23), 4., None),
        "only-max": (np.linspace(0., 10., 23), None, 4.),
        "equal-bounds": (np.array([2.5, 2.5, big, 2.5]), None, None),
        "all-no-value": (np.array([big, big, big]), None, None),
        "no-values": (np.zeros(0), None, None),
        "one-nan": (np.array([1., np.nan, 3., 2., big]), None, None),
        "nan-first": (np.array([np.nan, 1., 3.]), None, None),
        "infinite": (np.array([-np.inf, 0., np.inf]), None, None),
        "equal-colour-bounds": (np.array([1., 2., 3.]), 2., 2.),
        "integers": (np.arange(0, 511) / 510., None, None),
    }
    return cases


@pytest.mark.parametrize("name", sorted(color_cases()))
def test_colour_restatement_equals_the_numpy_statement(restatement, name):
    values, low, high = color_cases()[name]
    rgb, value_range = restatement.spectral_colors(values, low, high)
    expected, expected_range = db.python_colors(values, low, high)
    assert np.array_equal(rgb, expected), name
    assert np.array_equal(value_range, np.asarray(expected_range, dtype=np.float64)), name


def test_colours_that_the_reference_pins(restatement):
    strings = lambda values, *bounds: db.color_strings(restatement.spectral_colors(np.asarray(values, dtype=np.float64), *bounds)[0])
    assert strings([0., 0.5, 1.]) == ["#ff0000", "#ffff00", "#00ff00"]
    assert strings([-3., 9.], 0., 1.) == ["#ff0000", "#00ff00"]
    assert strings([1., np.nan, 3.]) == ["#ff0000", "#00ff00", "#00ff00"]                    # a NaN falls through to green
    assert strings([2.5, db.NO_VALUE, 2.5]) == ["black"] * 3
    assert strings([db.NO_VALUE] * 2) == ["black"] * 2
    assert strings([0., db.NO_VALUE, 1.]) == ["#ff0000", "", "#00ff00"]
    assert strings([0., 0.25, 1.]) == ["#ff0000", "#ff7f00", "#00ff00"]                      # int(0.5 * 255) = 127


def test_values_restatement_on_a_case_done_by_hand(restatement):
    """Two cells over three genes, the middle one outside the gene set: n = 2."""
    toc = np.array([0, 3, 5, 5], dtype=np.uint64)
    data = np.zeros(5, dtype=db.COUNT_DTYPE)
    data["gene"] = [0, 1, 2, 0, 1]
    data["count"] = [1., 5., 3., 2., 7.]
    local = np.array([0, 0xffffffff, 1], dtype=np.uint32)
    s = restatement.cell_similarities(toc, data, 2, 0, [0, 1, 2], local)
    # cell 0 keeps (1, 3): sum0 4, sum00 10; cell 1 keeps (2): sum1 2, sum11 4, sum01 2
    assert s[0] == (2. * 10. - 16.) / np.sqrt((2. * 10. - 16.) * (2. * 10. - 16.))
    assert s[1] == (2. * 2. - 4. * 2.) / np.sqrt((2. * 10. - 16.) * (2. * 4. - 4.))
    assert np.isnan(s[2])
    for method, factor in ((0, np.float32(1.)), (1, np.float32(1. / 4.)), (2, np.float32(1. / np.sqrt(10.)))):
        column = restatement.gene_expression(toc, data, 2, method, [0, 1, 2], local)
        assert column.tolist() == [float(factor * np.float32(3.)), 0., 0.]
    with pytest.raises(RuntimeError):
        restatement.gene_expression(toc, data, 1, 0, [0], local)


def svg_case():
    x = np.array([0.5, -1.25, 3.0000001, 1e-7, 123456.789, 2.5])
    y = np.array([1., 2.125, -7.5e10, 0., 1. / 3., 2.5])
    cells = np.array([7, 0, 4000000000, 12, 13, 99], dtype=np.uint32)
    v0 = np.array([0, 2, 5], dtype=np.uint32)
    v1 = np.array([1, 3, 5], dtype=np.uint32)
    return x, y, cells, v0, v1


@pytest.mark.parametrize("hide", (False, True))
@pytest.mark.parametrize("mode", ("plain", "colors", "groups"))
def test_svg_of_the_library_the_restatement_and_the_python_statement(restatement, tmp_path, mode, hide):
    x, y, cells, v0, v1 = svg_case()
    view = (600., 0.1, -2.5, 1. / 3., 0.0123456789, 1e-5)
    colors = ["#ff0000", "", "black", "red", "#00ff00", ""] if mode == "colors" else None
    groups = [2, 0, 2, 4, 0, 1] if mode == "groups" else None
    group_colors = {0: "#00ff00", 2: "black", 4: "#0000ff", 7: "#123456"} if mode == "groups" else None      # group 1 and 3 have none
    expected = db.python_svg(x, y, cells, v0, v1, hide, *view, "Some Genes", colors, groups, group_colors)
    theirs = restatement.graph_svg(str(tmp_path / "r.svg"), x, y, cells, v0, v1, hide, *view, "Some Genes", colors, groups, group_colors)
    assert theirs == expected
    capi.graph_write_svg(str(tmp_path / "l.svg"), x, y, cells, v0, v1, hide, *view, "Some Genes", vertex_colors=colors,
                         vertex_groups=groups, group_colors=group_colors)
    assert (tmp_path / "l.svg").read_bytes() == expected
    assert (b"<g id=edges>" in expected) == (not hide) and expected.startswith(b"<p><svg id=graphSvg width='600' height='600' viewBox='")
    if mode == "groups":
        assert b"<g id=vertexGroup1 style='fill:black'>" in expected and b"<g id=vertexGroup3 style='fill:black'></g>" in expected
        assert expected.index(b"cellId=0&") < expected.index(b"cellId=13&") < expected.index(b"cellId=99&") < expected.index(b"cellId=7&")


def test_svg_entry_checks(tmp_path):
    x, y, cells, v0, v1 = svg_case()
    with pytest.raises(RuntimeError, match="not below vertexCount"):
        capi.graph_write_svg(str(tmp_path / "a.svg"), x, y, cells, v0, np.array([1, 3, 6], dtype=np.uint32), False, 600., 0., 0., 1.,
                             0.1, 0.1, "G")
    with pytest.raises(RuntimeError, match="cannot open"):
        capi.graph_write_svg(str(tmp_path / "missing" / "a.svg"), x, y, cells, v0, v1, False, 600., 0., 0., 1., 0.1, 0.1, "G")


def test_the_number_of_a_meta_data_value():
    none = db.NO_VALUE
    for text, expected in (("1", 1.), ("-2.5e3", -2500.), ("+7", 7.), (".5", 0.5), ("1e400", np.inf), ("", none), (" 1", none),
                           ("\t1", none), ("1 ", none), ("1x", none), ("abc", none), ("1,5", none), ("--1", none), ("0", 0.)):
        assert capi.meta_data_number(text) == expected, text
    assert capi.meta_data_number(b"1\x002") == none


def category_store(tmp_path, values):
    cells = len(values)
    toc, data = fsp0_binding.clustered(cells, 12, 0.3, seed=5, cluster_count=3, non_integer=True)
    path = str(tmp_path / "store")
    files.create_directory(path, 12, toc, data)
    e = ExpressionMatrix(path)
    for cell, value in enumerate(values):
        if value is not None:
            e.setCellMetaData(cell, "kind", value)
    return e


def with_layout(e, vertices, x, y):
    """A cell graph as createCellGraph and computeCellGraphLayout leave it, without the GPU: what the host code of the colouring
    reads of it."""
    none = np.zeros(0, dtype=np.uint32)
    e._cellGraphs["g"] = {"vertexCellIds": np.asarray(vertices, dtype=np.uint32), "edgeVertices": (none, none), "vertexCount": len(vertices),
                          "layout": (np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)), "similarPairsName": "none"}


def test_two_categories_of_equal_frequency_and_a_vertex_list_shorter_than_the_cells(tmp_path):
    """std::greater<pair<int, string>>: count descending, then value DESCENDING; cell 5 is no vertex and is not counted."""
    values = ["a", "b", "b", "a", "c", "c"]
    e = category_store(tmp_path, values)
    with_layout(e, [0, 1, 2, 3, 4], np.arange(5.), np.arange(5.))
    r = e.computeCellGraphColors("g", "byMetaData", metaDataName="kind")
    assert r["frequencyTable"] == [(2, "b"), (2, "a"), (1, "c")] and r["couldNotColor"] == 0
    assert r["groups"].tolist() == [1, 0, 0, 1, 2] and r["groupColors"] == {0: "#00ff00", 1: "#0000ff", 2: "#ffff00"}
    assert r["colors"] == ["#0000ff", "#00ff00", "#00ff00", "#0000ff", "#ffff00"] and r["values"] is None
    groups, group_colors, table, could_not = db.python_category(values[:5])
    assert (groups, group_colors, table, could_not) == (r["groups"].tolist(), r["groupColors"], r["frequencyTable"], r["couldNotColor"])
    e.close()


def test_fourteen_categories(tmp_path):
    """Twelve colours, "black" from the thirteenth group on, couldNotColor their cells; a cell without the field counts as ""."""
    values = []
    for k in range(14):
        values += ["k%02d" % k] * (15 - k)
    values[-1] = None                               # the last category loses one of its two cells to ""
    e = category_store(tmp_path, values)
    with_layout(e, range(len(values)), np.zeros(len(values)), np.zeros(len(values)))
    r = e.computeCellGraphColors("g", "byMetaData", metaDataName="kind", metaDataMeaning="category")
    assert [value for _, value in r["frequencyTable"]] == ["k%02d" % k for k in range(12)] + ["k12", "k13", ""]
    assert r["couldNotColor"] == 3 + 1 + 1 and len(r["groupColors"]) == 15
    assert [r["groupColors"][g] for g in range(15)] == list(db.PALETTE) + ["black"] * 3
    assert list(db.PALETTE) == list(expression_matrix.CATEGORY_PALETTE)
    assert r["colors"][0] == "#00ff00" and r["colors"][-1] == "black" and r["colors"][-2] == "black"
    plain = [v if v is not None else "" for v in values]
    assert db.python_category(plain)[0] == r["groups"].tolist()
    # "color": the value verbatim; nothing is grouped
    c = e.computeCellGraphColors("g", "byMetaData", metaDataName="kind", metaDataMeaning="color")
    assert c["colors"] == plain and c["groupColors"] == {} and not c["groups"].any()
    # any other meaning, and any other option: no colouring
    for r in (e.computeCellGraphColors("g", "byMetaData", metaDataName="kind", metaDataMeaning="other"), e.computeCellGraphColors("g")):
        assert r["colors"] == [""] * len(values) and r["groupColors"] == {} and r["values"] is None and r["minValue"] is None
    with pytest.raises(NotImplementedError):
        e.computeCellGraphColors("g", "byMetaData", metaDataName="kind", reuseColors=True)
    e.close()


def test_layout_is_asked_for_first(tmp_path):
    e = category_store(tmp_path, ["a"])
    with_layout(e, [0], [0.], [0.])
    del e._cellGraphs["g"]["layout"]
    for call in (lambda: e.computeCellGraphColors("g"), lambda: e.writeCellGraphSvg("g", str(tmp_path / "a.svg")),
                 lambda: e.drawCellGraph("g")):
        with pytest.raises(RuntimeError) as error:
            call()
        assert str(error.value) == "Layout for graph g is not available."
    with pytest.raises(RuntimeError) as error:
        e.computeCellGraphColors("h")
    assert str(error.value) == "Graph h does not exist."
    e.close()


def test_the_coordinate_range_starts_its_maxima_at_the_smallest_positive_double(tmp_path):
    """CellGraph::computeCoordinateRange as written: a layout entirely at negative x and y has xMax = yMax = 2.2e-308."""
    tiny = float(np.finfo(np.float64).tiny)
    x, y = np.array([-5., -3., -4.]), np.array([-2., -1., -1.5])
    assert db.python_coordinate_range(x, y) == (-5., tiny, -2., tiny)
    e = category_store(tmp_path, ["a", "b", "c"])
    with_layout(e, [0, 1, 2], x, y)
    view = e._cell_graph_view(e._cellGraphs["g"], 600, None, None, None, None, None)
    assert view == db.python_default_view(x, y, 600.)
    assert view[0] == (-5. + tiny) / 2. and view[2] == (tiny + 5.) * 1.05 / 2. and view[1] == (-2. + (-2. + (tiny + 5.))) / 2.
    assert view[3] == 1.5 * ((tiny + 5.) * 1.05) / 600. and view[4] == 0.05 * ((tiny + 5.) * 1.05) / 600.
    # what is given is kept
    assert e._cell_graph_view(e._cellGraphs["g"], 600, 1., 2., 3., 4., 5.) == (1., 2., 3., 4., 5.)
    # positive coordinates: the ordinary bounding square
    with_layout(e, [0, 1, 2], -x, -y)
    assert e._cell_graph_view(e._cellGraphs["g"], 100, None, None, None, None, None)[:3] == (4., 2., 1.05)
    e.close()


def test_png_round_trip(tmp_path):
    rng = np.random.default_rng(11)
    for shape in ((1, 1, 4), (5, 7, 4), (64, 64, 4)):
        image = rng.integers(0, 256, shape, dtype=np.uint8)
        path = str(tmp_path / ("%dx%d.png" % shape[:2]))
        expression_matrix.write_png(path, image)
        assert np.array_equal(db.read_png(path), image)
    with pytest.raises(ValueError):
        expression_matrix.write_png(str(tmp_path / "bad.png"), np.zeros((4, 4, 3), dtype=np.uint8))
    with pytest.raises(ValueError, match="'red'"):
        expression_matrix._rgb_of("red")
    assert expression_matrix._rgb_of("#0a0B0c") == 0x0a0b0c and expression_matrix._rgb_of("") == 0
