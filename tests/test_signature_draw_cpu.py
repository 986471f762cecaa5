"""The yardsticks of the signature graph's colourings and pictures against one another, without a GPU:
tests/native/em2_signature_draw_restatement.cpp against the independent Python statement of tests/signature_draw_binding.py, and
the library's host-only entries (the value order, the random colours, the boundary vectors, the SVG text) against both.  The
cases are shared with the GPU tests."""
import numpy as np
import pytest

import signature_draw_binding as sb
from expressionmatrix2_amd import capi

U32 = np.uint32
WAVE_CELLS = 32            # em2_pie_census_wave_cells(), which tests/test_gpu_signature_draw.py checks: cases sit on both sides


@pytest.fixture(scope="module")
def restatement():
    return sb.load()


def census_case(vertex_colors, color_of_value=None, shuffle_seed=None):
    """(cellOffsets, cells, idOfCell, colorOfValue) from the value id of every cell of every vertex, in stored order.  The cell
    ids are a permutation, so that cells[] is a real indirection."""
    sizes = [len(v) for v in vertex_colors]
    offsets = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64)
    flat = np.asarray([c for v in vertex_colors for c in v], dtype=U32)
    n = len(flat)
    cells = np.random.default_rng(0 if shuffle_seed is None else shuffle_seed).permutation(n + 3).astype(U32)[:n]
    id_of_cell = np.zeros(n + 3, dtype=U32)
    id_of_cell[cells] = flat
    if color_of_value is None:
        color_of_value = np.arange(max(int(flat.max(initial=0)) + 1, 1), dtype=np.uint8)
    return offsets, cells, id_of_cell, np.asarray(color_of_value, dtype=np.uint8)


@pytest.fixture(scope="module")
def shared_census_cases():
    return census_cases()


def census_cases():
    rng = np.random.default_rng(3)
    t = WAVE_CELLS
    cases = {
        "no vertex": census_case([]),
        "vertices of one cell": census_case([[0], [5], [12], [5]]),
        "around the threshold": census_case([rng.integers(0, 13, n).tolist() for n in (t - 1, t, t + 1, 1, t + 1, t - 1, t)]),
        "five thousand cells": census_case([[1, 2], rng.integers(0, 13, 5000).tolist(), [3]]),
        "all thirteen in one vertex": census_case([list(range(13)) * 2 + [7], list(range(12, -1, -1)) * 3 + [4] * 9]),
        # values 12, 13, 14 are of rank >= 12: one black slice
        "three values merge into black": census_case([[12, 0, 13, 14, 0, 13, 12], [14] * 20 + [13] * 20 + [1] * 39 + [12] * 2],
                                                     list(range(12)) + [12, 12, 12]),
        # equal counts: the first occurrence decides; lane form (9 cells) and wave form (90 cells)
        "equal counts": census_case([[4, 2, 9, 2, 4, 9, 0, 0, 1], ([6] * 10 + [3] * 10 + [11] * 10) * 3, [8, 5] * 30 + [2] * 30]),
        "one colour": census_case([[6] * 7, [6] * 70]),
        "a vertex without cells": census_case([[1, 2], [], [3]]),
        "random": census_case([rng.integers(0, 13, int(n)).tolist() for n in rng.integers(1, 90, 300)], shuffle_seed=8),
    }
    return cases


@pytest.mark.parametrize("name", sorted(census_cases()))
def test_census_restatement_equals_the_python_statement(restatement, name):
    case = census_cases()[name]
    mine, theirs = restatement.census(*case), sb.python_census(*case)
    for key in ("sliceOffsets", "sliceColor", "sliceCells", "sliceFraction"):
        assert np.array_equal(mine[key], theirs[key]), (name, key)
    assert mine["sliceFraction"].tobytes() == theirs["sliceFraction"].tobytes()


def test_census_done_by_hand(restatement):
    r = restatement.census(*census_case([[4, 2, 9, 2, 4, 9, 0, 0, 1]]))
    assert r["sliceColor"].tolist() == [4, 2, 9, 0, 1] and r["sliceCells"].tolist() == [2, 2, 2, 2, 1]
    assert r["sliceFraction"].tolist() == [2. * (1. / 9.)] * 4 + [1. / 9.]
    black = restatement.census(*census_case([[12, 0, 13, 14, 0, 13, 12]], list(range(12)) + [12, 12, 12]))
    assert black["sliceColor"].tolist() == [12, 0] and black["sliceCells"].tolist() == [5, 2]


def test_census_restatement_refuses_an_id_out_of_range(restatement):
    offsets, cells, ids, colors = census_case([[0, 1], [2]])
    bad = ids.copy()
    bad[cells[2]] = 3
    assert restatement.census(offsets, cells, bad, colors) is None
    assert restatement.census(offsets, cells, ids, np.array([0, 13, 2], dtype=np.uint8)) is None
    far = cells.copy()
    far[0] = len(ids)
    assert restatement.census(offsets, far, ids, colors) is None


def test_random_colours(restatement):
    rgb, draws = restatement.random_colors(500)
    expected, expected_draws = sb.python_random_colors(500)
    # the two doubles g++'s <random> gives first, in the order of two sequenced calls (red, then green): std::mt19937(231)
    # starts 3356491351, 2600961200, 2509159060, 1021729225, and (3356491351 + 2600961200 * 2^32) / 2^64 is the first
    assert draws[0] == 0.60558347049669692 and draws[1] == 0.23788987323274116
    assert sb.python_mt19937(231, 4) == [3356491351, 2600961200, 2509159060, 1021729225]
    assert np.array_equal(draws, expected_draws) and np.array_equal(rgb, expected)
    assert np.array_equal(capi.signature_graph_random_colors(500), expected)
    assert len(capi.signature_graph_random_colors(0)) == 0
    assert capi.color_strings(rgb[:1]) == ["#%02x%02x%02x" % tuple(int(d * 255) for d in draws[:3])]


def value_cases():
    rng = np.random.default_rng(6)
    return {
        "three values": ["b"] * 5 + ["a"] * 9 + ["c"] * 5,
        "sixteen values, equal totals": [str(v) for v in rng.permutation(np.repeat(np.arange(16), [3, 3, 5, 5, 5, 1, 1, 9, 9, 2, 2, 2, 7, 7, 4, 4]))],
        "an empty string among them": ["", "x", "", "y", "x", ""],
        "not ASCII": ["é", "e", "z", "é", "Z"],
    }


# 40 values with many equal totals: above 16 elements std::sort's order of ties is libstdc++'s, and only the restatement states it
FORTY_VALUES = [("value%02d" % v) for v in np.random.default_rng(7).permutation(np.repeat(np.arange(40), np.tile([4, 4, 4, 4, 9, 9, 2, 2], 5)))]


@pytest.mark.parametrize("name", sorted(value_cases()))
def test_value_table_restatement_equals_the_python_statement(restatement, name):
    values = value_cases()[name]
    table, rank = restatement.value_table(values)
    expected, expected_rank = sb.python_value_table(values)
    assert table == expected and np.array_equal(rank, expected_rank)


def test_order_by_count_is_std_sort(restatement):
    rng = np.random.default_rng(2)
    for n in (0, 1, 16, 17, 40, 1000):
        counts = rng.integers(1, 6, n).astype(np.uint64)
        order = capi.order_by_count(counts)
        assert np.array_equal(order, restatement.order_by_count(counts)), n
        assert sorted(order.tolist()) == list(range(n)) and (np.diff(counts[order].astype(np.int64)) <= 0).all()
        if n <= 16:
            assert order.tolist() == sorted(range(n), key=lambda i: -int(counts[i]))
    table, _ = restatement.value_table(FORTY_VALUES)
    in_map_order = sorted(set(FORTY_VALUES))
    counts = np.asarray([FORTY_VALUES.count(v) for v in in_map_order], dtype=np.uint64)
    assert [in_map_order[i] for i in capi.order_by_count(counts)] == [value for value, _ in table]
    assert [value for value, _ in table] != sorted(in_map_order, key=lambda v: -FORTY_VALUES.count(v))      # the sort is not stable here


def boundary_case():
    fractions = [[1.], [0.5, 0.5], [0.75, 0.25], [0.25, 0.75], [1. / 3.] * 3, [2. * (1. / 9.)] * 4 + [1. / 9.], [1. / 13.] * 13,
                 [0.5000000000000001, 0.4999999999999999], np.random.default_rng(1).dirichlet(np.ones(7)).tolist()]
    offsets = np.concatenate([[0], np.cumsum([len(f) for f in fractions])]).astype(np.uint64)
    return offsets, np.asarray([f for v in fractions for f in v], dtype=np.float64)


def test_boundaries_of_the_library_the_restatement_and_numpy(restatement):
    """Against the restatement, which calls the same libm: equal.  Against numpy: two faithfully rounded cosines differ far below
    the half unit llround decides by, so the integers differ only at a near-tie, and then by one."""
    offsets, fraction = boundary_case()
    mine = capi.pie_boundaries(offsets, fraction)
    theirs = restatement.pie_boundaries(offsets, fraction)
    numpy_s = sb.python_pie_boundaries(offsets, fraction)
    for a, b, n in zip(mine, theirs, numpy_s):
        assert np.array_equal(a, b)
        assert np.abs(a.astype(np.int64) - n.astype(np.int64)).max() <= 1
    bx, by, arc = mine
    assert (bx[0], by[0], arc[0]) == (1048576, 0, 1)                               # one slice: the whole turn
    assert (bx[2], by[2]) == (-1048576, 0) and arc[1] == 0 and arc[2] == 0         # two exact halves
    assert arc[3] == 1 and arc[4] == 0 and arc[5] == 0 and arc[6] == 1
    assert arc[-9] == 1 and arc[-8] == 0                                           # just above and just below a half


def pie_slices(fractions_per_vertex):
    offsets = np.concatenate([[0], np.cumsum([len(f) for f in fractions_per_vertex])]).astype(np.uint64)
    fraction = np.asarray([f for v in fractions_per_vertex for f in v], dtype=np.float64)
    return (offsets,) + sb.load().pie_boundaries(offsets, fraction)


def raster_cases():
    """name -> (x, y, radius, v0, v1, size, xc, yc, half, sliceOffsets, bx, by, arc); a unit is a pixel where the view says so."""
    rng = np.random.default_rng(11)
    none = np.zeros(0, dtype=U32)
    wave = 32.                                   # em2_graph_draw_pies_wave_radius(), checked by the GPU test
    cases = {}
    thirteen = [1. / 13.] * 13
    view64 = (64, 32., 32., 32.)
    x = [10.5, 30., 50.2, 20., 40., 12., 60., 33.3]
    y = [10.5, 12., 11.1, 40., 44., 55., 60., 31.]
    fractions = [[0.5, 0.5], [0.75, 0.25], thirteen, [0.2, 0.3, 0.5], [1.], [0.9, 0.1], [0.25, 0.25, 0.25, 0.25], [0.6, 0.4]]
    cases["eight pies"] = (x, y, [6., 7.5, 9., 3.9, 5., 4.1, 8., 0.4], [0, 1, 2], [1, 2, 3]) + view64 + pie_slices(fractions)
    # radii 0, the two sides of both class bounds, and one that covers the whole image; not sorted by radius
    radii = [0., 4., 4.01, wave, wave + 0.01, 300., 3.99, wave - 0.01]
    xs, ys = rng.random(8) * 200., rng.random(8) * 200.
    cases["every radius class, S = 200"] = (xs, ys, radii, [0, 5], [7, 2], 200, 100., 100., 100.) + \
        pie_slices([rng.dirichlet(np.ones(int(m))).tolist() for m in rng.integers(1, 8, 8)])
    cases["the whole image on top"] = (xs, ys, radii[:5] + [3.99, wave - 0.01, 300.], none, none, 200, 100., 100., 100.) + \
        pie_slices([[0.3, 0.7]] * 7 + [[0.55, 0.25, 0.2]])
    cases["half outside"] = ([0., 64., 31.9, -3.], [20., 40., -2., 70.], [9., 12.5, 7., 10.], none, none) + view64 + \
        pie_slices([[0.5, 0.5], [0.4, 0.6], thirteen, [0.3, 0.3, 0.4]])
    cases["overlapping, in painter order"] = ([30., 34., 32., 32.], [30., 31., 35., 32.], [14., 9., 6., 2.], none, none) + view64 + \
        pie_slices([[0.5, 0.5], [0.7, 0.3], [0.1, 0.9], [0.5, 0.25, 0.25]])
    # a slice whose start and end coincide: empty with largeArc 0, the whole disc with 1; slice 0 of the second vertex is asked first
    offsets = np.array([0, 2, 4, 6], dtype=np.uint64)
    bx = np.array([1048576, 1048576, 1048576, 1048576, -1048576, 1048576], dtype=np.int32)
    by = np.zeros(6, dtype=np.int32)
    cases["coincident boundaries"] = ([16., 48., 32.], [16., 16., 48.], [10., 10., 10.], none, none) + view64 + \
        (offsets, bx, by, np.array([0, 0, 1, 0, 0, 0], dtype=np.uint8))
    cases["one pixel"] = ([0.5, 0.2], [0.5, 0.9], [0.3, 5.], [0], [1], 1, 0.5, 0.5, 0.5) + pie_slices([[0.5, 0.5], [0.25, 0.75]])
    # the own pixel with d = (0, 0): the centre on a pixel centre (ux = 256 i + 128), radius 0
    cases["own pixel"] = ([10.5, 20.5], [7.5, 9.5], [0., 0.], none, none) + view64 + pie_slices([[0.1, 0.9], [0.5, 0.5]])
    n = 60
    cases["random, S = 96"] = (rng.random(n) * 110. - 7., rng.random(n) * 110. - 7., rng.random(n) ** 3 * 40., rng.integers(0, n, 80),
                               rng.integers(0, n, 80), 96, 48.3, 47.9, 50.5) + \
        pie_slices([rng.dirichlet(np.ones(int(m))).tolist() for m in rng.integers(1, 14, n)])
    return cases


CPU_RASTER_CASES = ("eight pies", "half outside", "overlapping, in painter order", "coincident boundaries", "one pixel", "own pixel",
                    "random, S = 96")


@pytest.mark.parametrize("name", CPU_RASTER_CASES)
def test_pie_raster_restatement_equals_the_python_statement(restatement, name):
    case = raster_cases()[name]
    mine, theirs = restatement.graph_draw_pies(*case), sb.python_pie_raster(*case)
    assert mine is not None
    for layer, a, b in zip(("vertexTop", "sliceTop", "edgeHits"), mine, theirs):
        assert np.array_equal(a, b), "%s: %s differs at %s" % (name, layer, np.argwhere(a != b)[:5].tolist())


def test_pie_raster_by_hand(restatement):
    """Two exact halves: the boundary (-2^20, 0) puts a pixel centre below the centre into slice 0 (y points down, the angle
    increases with the sweep), one above into slice 1."""
    offsets, bx, by, arc = pie_slices([[0.5, 0.5]])
    assert bx.tolist() == [1048576, -1048576] and by.tolist() == [0, 0]
    top, slices, hits = restatement.graph_draw_pies([32.5], [32.5], [10.], [], [], 64, 32., 32., 32., offsets, bx, by, arc)
    assert slices[32, 32] == 1                                   # d = (0, 0)
    assert slices[36, 32] == 1 and slices[28, 32] == 2           # below: cross(a, d) > 0; above: < 0
    # on the line through both boundaries cross(d, b) = 0, which is not > 0: such a centre is left to the last slice, on both rays
    assert slices[32, 38] == 2 and slices[32, 26] == 2
    assert top[32, 43] == 0 and top[32, 42] == 1 and not hits.any()
    # a slice of three quarters
    offsets, bx, by, arc = pie_slices([[0.75, 0.25]])
    assert arc.tolist() == [1, 0]
    _, slices, _ = restatement.graph_draw_pies([32.5], [32.5], [10.], [], [], 64, 32., 32., 32., offsets, bx, by, arc)
    assert slices[36, 36] == 1 and slices[36, 28] == 1 and slices[28, 28] == 1 and slices[28, 36] == 2


def test_pie_raster_restatement_refuses_what_the_entry_refuses(restatement):
    offsets, bx, by, arc = pie_slices([[0.5, 0.5], [1.]])
    draw = lambda radius, offsets=offsets: restatement.graph_draw_pies([5., 9.], [5., 9.], radius, [], [], 64, 32., 32., 32., offsets, bx, by, arc)
    assert draw([1., 2.]) is not None and draw([1., 8192.]) is not None
    assert draw([np.nan, 1.]) is None and draw([1., np.inf]) is None and draw([-1., 1.]) is None and draw([1., 8193.]) is None
    assert draw([1., 2.], np.array([0, 3, 2], dtype=np.uint64)) is None and draw([1., 2.], np.array([0, 0, 3], dtype=np.uint64)) is None
    assert draw([1., 2.], np.array([1, 2, 3], dtype=np.uint64)) is None and draw([1., 2.], np.array([0, 2, 2], dtype=np.uint64)) is None


def svg_cases():
    rng = np.random.default_rng(13)
    n = 14
    x, y = rng.random(n) * 30. - 12., rng.random(n) * 20. - 3.
    counts = rng.permutation(np.array([1, 1, 2, 2, 2, 5, 9, 9, 40, 40, 1000, 3, 3, 7], dtype=np.uint64))
    v0, v1 = rng.integers(0, n, 20).astype(U32), rng.integers(0, n, 20).astype(U32)
    census = sb.python_census(*census_case([rng.integers(0, 13, int(c) if c < 100 else 100).tolist() for c in counts]))
    pies = dict(slice_offsets=census["sliceOffsets"], slice_colors=sb.slice_strings(census["sliceColor"]),
                slice_fraction=census["sliceFraction"])
    return {
        "uncoloured": ((x, y, counts, v0, v1), {}),
        "pies": ((x, y, counts, v0, v1), pies),
        "pies, no edges, another view": ((x, y, counts, v0, v1), dict(pies, hide_edges=True, size=830., x_shift=1.5, y_shift=-2.25,
                                                                       zoom=3., vertex_size=0.7, edge_thickness=2.)),
        "all at negative x": ((-x - 40., y, counts, v0, v1), dict(pies, edge_thickness=0.3)),
        "one vertex": ((x[:1], y[:1], counts[:1], v0[:0], v1[:0]), {}),
    }


@pytest.mark.parametrize("name", sorted(svg_cases()))
def test_svg_of_the_library_the_restatement_and_the_python_statement(restatement, tmp_path, name):
    arrays, options = svg_cases()[name]
    theirs, their_parameters = restatement.svg(str(tmp_path / "r.svg"), *arrays, **options)
    assert theirs == sb.python_signature_svg(*arrays, **options), name
    names = {"size": "svg_size_pixels", "zoom": "zoom_factor", "vertex_size": "vertex_size_factor", "edge_thickness": "edge_thickness_factor"}
    parameters = capi.signature_graph_write_svg(str(tmp_path / "l.svg"), *arrays, **{names.get(k, k): v for k, v in options.items()})
    assert (tmp_path / "l.svg").read_bytes() == theirs, name
    assert parameters == their_parameters
    expected = sb.python_signature_view(arrays[0], arrays[1], arrays[2], options.get("size", 500.), options.get("x_shift", 0.),
                                        options.get("y_shift", 0.), options.get("zoom", 1.))[:4]
    assert parameters == expected
    if name == "uncoloured":
        assert theirs.count(b"<circle") == 14 and theirs.count(b"fill='black'") == 14 and b"<path" not in theirs
    if name == "pies":
        assert b"<path" in theirs and b" 0 1 1 " in theirs and b" 0 0 1 " in theirs


def test_svg_with_repeated_cell_counts_above_sixteen_vertices(restatement, tmp_path):
    """60 vertices with many equal cell counts: the order of the circles is std::sort's, which only the restatement states."""
    rng = np.random.default_rng(17)
    n = 60
    x, y = rng.random(n) * 9., rng.random(n) * 9.
    counts = rng.integers(1, 5, n).astype(np.uint64)
    none = np.zeros(0, dtype=U32)
    theirs, _ = restatement.svg(str(tmp_path / "r.svg"), x, y, counts, none, none)
    capi.signature_graph_write_svg(str(tmp_path / "l.svg"), x, y, counts, none, none)
    assert (tmp_path / "l.svg").read_bytes() == theirs
    stable = sorted(range(n), key=lambda v: -int(counts[v]))
    assert capi.order_by_count(counts).tolist() != stable


def test_svg_entry_checks(tmp_path):
    x, y, counts = np.array([0., 1.]), np.array([0., 1.]), np.array([1, 2], dtype=np.uint64)
    none = np.zeros(0, dtype=U32)
    with pytest.raises(RuntimeError, match="not below vertexCount"):
        capi.signature_graph_write_svg(str(tmp_path / "a.svg"), x, y, counts, [0], [2])
    with pytest.raises(RuntimeError, match="cannot open"):
        capi.signature_graph_write_svg(str(tmp_path / "missing" / "a.svg"), x, y, counts, none, none)
    with pytest.raises(RuntimeError, match="do not ascend"):
        capi.signature_graph_write_svg(str(tmp_path / "a.svg"), x, y, counts, none, none, slice_offsets=[0, 2, 1], slice_colors=["a"],
                                       slice_fraction=[1.])
