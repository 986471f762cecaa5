"""compareCellGraphs and assignColorsToGroups without a GPU: the one-thread C++ restatement the GPU tests compare against
(tests/native/em2_graph_compare_restatement.cpp) held against an independent Python statement (dicts, np.float32 scalars,
libm's roundf), the float cases of the bin on their own, the colourings, the facade's error texts and what the new C entry
points say about a null pointer and about a machine without a HIP device."""
import ctypes

import numpy as np
import pytest

import graph_compare_binding as gb
from expressionmatrix2_amd import capi
from expressionmatrix2_amd.expression_matrix import ExpressionMatrix

F = np.float32
NEGATIVE_ZERO, POSITIVE_ZERO = 0x80000000, 0


@pytest.fixture(scope="module")
def restatement():
    return gb.load()


def one_bin(restatement, s0, s1):
    """The bin of one common edge: (bits of binDelta, identical count), from the restatement and from Python, which must agree."""
    g0, g1 = gb.pair_of_edges(s0, s1)
    status, r = restatement.compare(g0, g1)
    assert status == gb.OK and r["commonEdgeCount"] == 1 and r["binCount"].tolist() == [1]
    gb.assert_same_comparison(r, gb.python_compare(g0, g1), "%r against %r" % (s0, s1))
    return int(gb.bits(r["binDelta"])[0]), r["commonIdenticalEdgeCount"]


def test_roundf_is_not_numpys_round():
    """std::round is ties away from zero; np.round and Python's round are ties to even."""
    assert gb._libm().roundf(0.5) == 1.0 and gb._libm().roundf(-0.5) == -1.0 and gb._libm().roundf(2.5) == 3.0
    assert np.round(F(0.5)) == 0.0 and round(2.5) == 2


def test_float_cases_of_the_bin(restatement):
    # the zero bin keeps the sign of its product
    assert one_bin(restatement, F(0.5), F(0.5)) == (POSITIVE_ZERO, 1)
    assert one_bin(restatement, F(0.5), F(0.499)) == (NEGATIVE_ZERO, 0)
    assert one_bin(restatement, F(0.5), F(0.501)) == (POSITIVE_ZERO, 0)
    assert float(F(0.499) - F(0.5)) == pytest.approx(-0.000999987, rel=1e-5)
    # a negative denormal difference
    tiny = np.uint32(1).view(np.float32)
    assert one_bin(restatement, tiny, F(0.0)) == (NEGATIVE_ZERO, 0)
    # quotients of exactly +-0.5 go away from zero
    assert F(0.005) / F(0.01) == F(0.5)
    assert one_bin(restatement, F(0.0), F(0.005)) == (int(gb.bits([F(0.01) * F(1.0)])[0]), 0)
    assert one_bin(restatement, F(0.0), F(-0.005)) == (int(gb.bits([F(0.01) * F(-1.0)])[0]), 0)
    assert float(F(0.01) * F(1.0)) == pytest.approx(0.00999999978, rel=1e-8)
    # a quotient just below 0.5
    assert float((F(0.205) - F(0.2)) / F(0.01)) == pytest.approx(0.4999995, rel=1e-6)
    assert one_bin(restatement, F(0.2), F(0.205)) == (POSITIVE_ZERO, 0)
    # a quotient of exactly 1.5
    assert F(0.015) / F(0.01) == F(1.5)
    assert one_bin(restatement, F(0.0), F(0.015)) == (int(gb.bits([F(0.01) * F(2.0)])[0]), 0)
    assert float(F(0.01) * F(2.0)) == pytest.approx(0.0199999996, rel=1e-8)
    # the quotient overflows: the bins +inf and -inf
    assert one_bin(restatement, F(-3e38), F(3e38)) == (0x7f800000, 0)
    assert one_bin(restatement, F(3e38), F(-3e38)) == (0xff800000, 0)
    # the two zeros are identical
    assert one_bin(restatement, F(-0.0), F(0.0)) == (POSITIVE_ZERO, 1)


def test_the_zero_bin_is_keyed_by_its_first_edge(restatement):
    """Edges (i, i + 1) ascend in key order with i: the zero bin takes the sign of the first of them that falls into it."""
    for first, expected in [((0.5, 0.5), POSITIVE_ZERO), ((0.5, 0.499), NEGATIVE_ZERO), ((0.5, 0.501), POSITIVE_ZERO)]:
        others = [(0.5, 0.499), (0.5, 0.501), (0.5, 0.5), (0.5, 0.6)]
        s0 = [F(0.3), F(first[0])] + [F(a) for a, _ in others]
        s1 = [F(0.9), F(first[1])] + [F(b) for _, b in others]
        g0, g1 = gb.path_graph(len(s0), s0), gb.path_graph(len(s1), s1)
        status, r = restatement.compare(g0, g1)
        assert status == gb.OK
        gb.assert_same_comparison(r, gb.python_compare(g0, g1), "first %r" % (first,))
        zero = [int(b) for b, d in zip(gb.bits(r["binDelta"]), r["binDelta"]) if d == 0]
        assert zero == [expected] and r["binCount"][list(r["binDelta"]).index(0)] == 4


def test_the_table_bins_have_distinct_products():
    """Within |r| <= 2048 distinct r give distinct, ascending products 0.01f * r: the bins of the table are bins of the map."""
    products = (np.arange(-2049, 2050, dtype=np.float32) * F(0.01)).astype(np.float32)
    assert (np.diff(products) > 0).all()


def test_restatement_against_python_on_random_graphs(restatement):
    rng = np.random.default_rng(20240607)
    sizes = (0, 1, 2, 7, 63, 64, 65, 300)
    for trial in range(60):
        pool = np.arange(40, dtype=np.uint32) * np.uint32(7) + np.uint32(rng.integers(0, 5))
        n0, n1 = rng.choice(sizes), rng.choice(sizes)
        g0 = gb.random_graph(rng, pool, int(rng.integers(2, 30)), int(n0))
        g1 = gb.similar_graph(rng, g0) if trial % 2 else gb.random_graph(rng, pool, int(rng.integers(2, 30)), int(n1))
        status, r = restatement.compare(g0, g1)
        assert status == gb.OK
        gb.assert_same_comparison(r, gb.python_compare(g0, g1), "trial %d" % trial)


def test_restatement_vertices_duplicates_and_errors(restatement):
    # a multiset intersection: cell 5 twice and three times, cell 7 once and not at all
    g0 = gb.graph([5, 5, 7, 9], [0], [3], [0.5])
    g1 = gb.graph([9, 5, 5, 5], [0], [1], [0.5])
    status, r = restatement.compare(g0, g1)
    assert status == gb.OK and r["commonVertexCount"] == 3 and r["commonEdgeCount"] == 1
    gb.assert_same_comparison(r, gb.python_compare(g0, g1), "repeated ids")
    # the same unordered pair twice, in both orientations: the first stays
    g0 = gb.graph([1, 2], [0, 1], [1, 0], [0.25, 0.75])
    g1 = gb.graph([2, 1], [0, 1], [1, 0], [0.75, 0.25])
    status, r = restatement.compare(g0, g1)
    assert status == gb.OK and (r["edgeCount0"], r["edgeCount1"], r["commonEdgeCount"]) == (1, 1, 1)
    assert r["binDelta"].tolist() == [float(F(0.01) * F(50.0))]
    # errors
    nan = F(np.nan)
    assert restatement.compare(*gb.pair_of_edges(nan, F(0.5)))[0] == gb.NOT_A_NUMBER
    assert restatement.compare(*gb.pair_of_edges(F(np.inf), F(np.inf)))[0] == gb.NOT_A_NUMBER
    assert restatement.compare(gb.graph([1, 2, 3], [0, 1], [1, 2], [0.5, nan]), gb.graph([1, 2], [0], [1], [0.5]))[0] == gb.OK
    assert restatement.compare(gb.graph([4, 4], [0], [1], [0.5]), gb.graph([1, 2], [0], [1], [0.5]))[0] == gb.SELF_LOOP
    assert restatement.compare(gb.graph([1, 2], [0], [2], [0.5]), gb.graph([1, 2], [0], [1], [0.5]))[0] == gb.BAD_INDEX


def group_cases():
    rng = np.random.default_rng(7)
    cases = {}
    cases["one group"] = (np.zeros(6), [0, 1, 2], [1, 2, 3])
    cases["inside groups"] = ([0, 0, 1, 1, 2, 2], [0, 2, 4], [1, 3, 5])
    cases["path of 20"] = (np.arange(20), np.arange(19), np.arange(1, 20))
    clique = [(a, b) for a in range(13) for b in range(a + 1, 13)]
    cases["clique of 13"] = (np.arange(13), [a for a, _ in clique], [b for _, b in clique])
    cases["gaps"] = ([0, 3, 3, 7, 9], [0, 1, 3, 2], [1, 3, 4, 4])
    cases["own groups"] = (rng.permutation(300), rng.integers(0, 300, 900), rng.integers(0, 300, 900))
    cases["high low"] = ([0, 1, 2, 3], [3, 2, 1], [0, 0, 0])
    cases["low high"] = ([0, 1, 2, 3], [0, 0, 0], [3, 2, 1])
    cases["both ways"] = ([0, 1, 2, 3], [0, 3, 1, 2, 0], [3, 0, 2, 1, 3])
    cases["random"] = (rng.integers(0, 25, 200), rng.integers(0, 200, 1500), rng.integers(0, 200, 1500))
    cases["nothing"] = ([], [], [])
    return cases


GROUP_CASES = group_cases()


@pytest.mark.parametrize("name", sorted(GROUP_CASES))
def test_colouring_is_proper_and_the_literal_greedy(restatement, name):
    group, v0, v1 = GROUP_CASES[name]
    status, r = restatement.group_colors(group, v0, v1)
    assert status == gb.OK
    gb.assert_proper(r, name)
    gb.assert_same_group_colors(r, gb.python_group_colors(group, v0, v1), name)
    if name == "path of 20":
        assert r["colorTable"].tolist() == [0, 1] * 10
    if name == "clique of 13":
        assert r["colorTable"].tolist() == list(range(13))
    if name == "gaps":
        assert r["groupCount"] == 10 and len(r["colorTable"]) == 10
    if name in ("one group", "inside groups"):
        assert len(r["pairGroup0"]) == 0 and not r["colorTable"].any()


def test_group_restatement_refuses_an_index_out_of_range(restatement):
    assert restatement.group_colors([0, 1], [0], [2])[0] == gb.BAD_INDEX


# ---- the facade's errors (nothing here reaches the device) ----

def test_facade_error_texts(tmp_path):
    e = ExpressionMatrix.create(str(tmp_path / "store"))
    stub = {"layout": (np.zeros(0), np.zeros(0)), "vertexCount": 0}
    e._cellGraphs["a"] = dict(stub)
    for names in (("a", "b"), ("b", "a"), ("b", "b"), ("b", "c")):
        with pytest.raises(RuntimeError) as error:
            e.compareCellGraphs(*names)
        assert str(error.value) == "Did not find one or both of the cell graphs to be compared."
    with pytest.raises(RuntimeError) as error:
        e.compareCellGraphs("a", "a")
    assert str(error.value) == "Comparison of a cell graph with itself requested. "
    with pytest.raises(RuntimeError) as error:
        e.reuseCellGraphColors("b")
    assert str(error.value) == "Graph b does not exist."
    for coloring in (None, {"coloringOption": "bySimilarity", "frequencyTable": []}, {"coloringOption": "byMetaData", "frequencyTable": []}):
        if coloring is not None:
            e._cellGraphs["a"]["coloring"] = coloring
        with pytest.raises(RuntimeError, match='is not a "category" colouring'):
            e.reuseCellGraphColors("a")
    e.close()


# ---- the entry points' words, through the raw C ABI ----

INVALID, NO_DEVICE = 1, 2
NO_DEVICE_TEXT = ": no HIP device is visible (this library has no CPU path)"
IDS = np.arange(4, dtype=np.uint32)
E0 = np.array([0, 1], dtype=np.uint32)
E1 = np.array([1, 2], dtype=np.uint32)
ES = np.array([0.5, 0.5], dtype=np.float32)
HANDLE = ctypes.c_void_p(None)
OUT = ctypes.byref(HANDLE)

VALID = {
    "em2_cell_graph_compare": (IDS, 4, E0, E1, ES, 2, IDS, 4, E0, E1, ES, 2, 0, OUT),
    "em2_dev_cell_graph_compare": (IDS, 4, E0, E1, ES, 2, IDS, 4, E0, E1, ES, 2, 0, OUT),
    "em2_graph_comparison_sizes": (None, None, None, None, None, None, None, None),
    "em2_graph_comparison_get": (None, None, None),
    "em2_graph_group_colors": (IDS, 4, E0, E1, 2, 0, OUT),
    "em2_dev_graph_group_colors": (IDS, 4, E0, E1, 2, 0, OUT),
    "em2_group_colors_sizes": (None, None, None, None),
    "em2_group_colors_get": (None, None, None, None, None),
}

# (entry point, the argument that is null): every pointer the entry needs
NULL_CASES = [(name, index) for name in ("em2_cell_graph_compare", "em2_dev_cell_graph_compare") for index in (0, 2, 3, 4, 6, 8, 9, 10, 13)]
NULL_CASES += [(name, index) for name in ("em2_graph_group_colors", "em2_dev_graph_group_colors") for index in (0, 2, 3, 6)]
NULL_CASES += [(name, 0) for name in ("em2_graph_comparison_sizes", "em2_graph_comparison_get", "em2_group_colors_sizes", "em2_group_colors_get")]


def call(name, arguments):
    lib = capi.load()
    rc = getattr(lib, name)(*[a.ctypes.data if isinstance(a, np.ndarray) else a for a in arguments])
    return rc, lib.em2_last_error().decode()


@pytest.mark.parametrize("name,index", NULL_CASES, ids=["%s-%d" % case for case in NULL_CASES])
def test_a_null_pointer(name, index):
    arguments = list(VALID[name])
    arguments[index] = None
    assert call(name, arguments) == (INVALID, name + ": null pointer")


def test_arguments_are_checked_before_the_device_is_looked_for():
    arguments = list(VALID["em2_cell_graph_compare"])
    arguments[12] = 2
    rc, text = call("em2_cell_graph_compare", arguments)
    assert rc == INVALID and text.startswith("em2_cell_graph_compare: path must be 0 ")
    arguments = list(VALID["em2_graph_group_colors"])
    arguments[5] = 3
    assert call("em2_graph_group_colors", arguments) == (INVALID, "em2_graph_group_colors: path must be 0 (automatic), 1 (LDS) or 2 (sort)")
    # no edges and no vertices need no pointers
    if capi.device_count() == 0:
        assert call("em2_cell_graph_compare", (None, 0, None, None, None, 0, None, 0, None, None, None, 0, 0, OUT))[0] == NO_DEVICE


@pytest.mark.skipif(capi.device_count() > 0, reason="a HIP device is visible")
@pytest.mark.parametrize("name", ["em2_cell_graph_compare", "em2_dev_cell_graph_compare", "em2_graph_group_colors",
                                  "em2_dev_graph_group_colors"])
def test_no_device(name):
    assert call(name, VALID[name]) == (NO_DEVICE, name + NO_DEVICE_TEXT)
    assert HANDLE.value is None
    wrapper = {"em2_cell_graph_compare": lambda: capi.cell_graph_compare((IDS, E0, E1, ES), (IDS, E0, E1, ES)),
               "em2_graph_group_colors": lambda: capi.graph_group_colors(IDS, E0, E1)}.get(name)
    if wrapper:
        with pytest.raises(RuntimeError, match="no HIP device"):
            wrapper()


def test_wrappers_check_their_arguments():
    with pytest.raises(ValueError):
        capi.cell_graph_compare((IDS, E0, E1[:1], ES), (IDS, E0, E1, ES))
    with pytest.raises(ValueError):
        capi.graph_group_colors(IDS, E0, E1[:1])
