"""em2_graph_layout on the GPU (csrc/em2_layout.hip) against tests/native/em2_layout_restatement.cpp, which
tests/test_layout_cpu.py holds against a float64 numpy statement of the model and against closed forms.  The order of every
rounding is part of the contract: positions, iteration count, final step and final energy equal the
restatement's bit for bit."""
import ctypes

import numpy as np
import pytest

import layout_binding as lb
import synth
from expressionmatrix2_amd import CellGraphVertexInfo, ExpressionMatrix, capi, files

pytestmark = pytest.mark.gpu

INVALID = 1
DEFAULT = lb.DEFAULTS["maxIterationCount"]
# The restatement needs 3 ns a pair on one thread: the default 300 iterations (about 150 until the step is below the
# tolerance) of 4100 vertices would take it 8 s.  That size runs 0, 1, 2 and 25 iterations; every other one the default too.
ITERATIONS = {name: (0, 1, 2, DEFAULT) for name in lb.CASES}
ITERATIONS["random-4100"] = (0, 1, 2, 25)


def _parameters(**changes):
    p = dict(lb.DEFAULTS)
    p.update(changes)
    return capi.LayoutParameters(**p)


@pytest.mark.parametrize("name", lb.CASES)
def test_run_equals_the_restatement(name):
    """N = 1, 2, 63, 64, 65 (the wave); 255, 256, 257 (the workgroup's vertices and the chunk of the energy tree); 2032, 2048,
    2049 (slices of 127, 128, 129 against the tile of 128); 4100 (slices of two whole tiles and a ragged one); no edge at all;
    a star of 600 leaves; a ring; isolated vertices; self-loops and a repeated edge; the two cliques."""
    n, edges = lb.case(name)
    for iterations in ITERATIONS[name]:
        mine = capi.graph_layout(n, edges[0], edges[1], _parameters(maxIterationCount=iterations))
        theirs = lb.reference(name, iterations)
        lb.assert_same_run(mine, theirs, "%s after %d iterations" % (name, iterations))
        assert mine[2] == iterations or iterations == DEFAULT


def test_the_default_run_ends_on_the_tolerance_not_on_the_count():
    """(so the runs above covered the stop rule; not a statement about the quality of the picture)"""
    x, y, iterations, step, energy = capi.graph_layout(*_flat(lb.case("ring-70")))
    assert 0 < iterations < DEFAULT and step < lb.DEFAULTS["tolerance"] and np.isfinite(energy)
    assert np.all(np.isfinite(x)) and np.all(np.isfinite(y))


def _flat(graph):
    return graph[0], graph[1][0], graph[1][1]


@pytest.mark.parametrize("gravity,tolerance,step,seed", [(0., 0.01, 1., 231), (0.5, 0.05, 3., 7), (0.02, 0.3, 0.25, 0)])
def test_other_parameters_equal_the_restatement(gravity, tolerance, step, seed):
    for name in ("random-257", "isolated", "loops-and-repeats"):
        n, edges = lb.case(name)
        changes = dict(gravity=gravity, tolerance=tolerance, initialStep=step, seed=seed, maxIterationCount=60)
        mine = capi.graph_layout(n, edges[0], edges[1], _parameters(**changes))
        lb.assert_same_run(mine, lb.load().layout(n, edges, **changes), name)


def _positions(n, seed, coincident):
    rng = np.random.default_rng(seed)
    x = (rng.random(n, dtype=np.float32) - np.float32(0.5)) * np.float32(np.sqrt(n))
    y = (rng.random(n, dtype=np.float32) - np.float32(0.5)) * np.float32(np.sqrt(n))
    if coincident and n >= 4:
        x[3], y[3] = x[1], y[1]                               # two pairs of coincident vertices
        x[n - 1], y[n - 1] = x[0], y[0]
    return x, y


@pytest.mark.parametrize("name,gravity", [("random-2", 0.), ("random-65", 0.), ("random-257", 0.02), ("random-2049", 0.5),
                                          ("star-600", 0.02), ("loops-and-repeats", 0.02), ("isolated", 0.), ("no-edges", 1.)])
def test_forces_against_the_float64_statement_and_the_restatement(name, gravity):
    """The check that shares no code with the kernel's author: every component of em2_graph_layout_forces within
    (N + 8) 2^-24 sum|terms| of the numpy statement (the bound of tests/test_layout_cpu.py).  Then the restatement, bit for bit,
    with coincident start positions among them."""
    n, edges = lb.case(name)
    x, y = _positions(n, 17, coincident=True)
    fx, fy, energy = capi.graph_layout_forces(n, edges[0], edges[1], gravity, x, y)
    f, absolute = lb.numpy_forces(n, edges, gravity, x, y)
    error = np.abs(np.stack([fx, fy], axis=1).astype(np.float64) - f)
    assert np.all(error <= lb.force_bound(n, absolute))
    rx, ry, renergy = lb.load().forces(n, edges, gravity, x, y)
    assert np.array_equal(lb.bits(fx), lb.bits(rx)) and np.array_equal(lb.bits(fy), lb.bits(ry))
    assert np.float64(energy).tobytes() == np.float64(renergy).tobytes()


def test_coincident_vertices_add_an_exact_zero():
    x = np.array([1.5, 1.5, 1.5, -4.], dtype=np.float32)
    y = np.array([-2., -2., -2., 0.25], dtype=np.float32)
    fx, fy, _ = capi.graph_layout_forces(4, [0], [0], 0., x, y)
    assert lb.bits(fx[:3]).tolist() == [lb.bits(fx[:1])[0]] * 3 and lb.bits(fy[:3]).tolist() == [lb.bits(fy[:1])[0]] * 3
    fx, fy, energy = capi.graph_layout_forces(3, [0], [0], 0., x[:3], y[:3])
    assert lb.bits(fx).tolist() == [0, 0, 0] and lb.bits(fy).tolist() == [0, 0, 0] and energy == 0.


@pytest.mark.parametrize("name", ["random-1", "random-65", "random-2049", "no-edges", "star-600", "loops-and-repeats"])
def test_device_entry_equals_the_host_entry_and_a_call_repeats_itself(name):
    n, edges = lb.case(name)
    parameters = _parameters(maxIterationCount=20)
    first = capi.graph_layout(n, edges[0], edges[1], parameters)
    second = capi.graph_layout(n, edges[0], edges[1], parameters)
    device = capi.dev_graph_layout(n, edges[0], edges[1], parameters)
    lb.assert_same_run(second, first, name + ", again")
    lb.assert_same_run(device, first, name + ", device entry")


def test_the_scratch_cache_is_only_a_cache():
    for name in ("random-4100", "random-2", "random-257"):
        n, edges = lb.case(name)
        lb.assert_same_run(capi.graph_layout(n, edges[0], edges[1], _parameters(maxIterationCount=2)), lb.reference(name, 2), name)
    capi.load().em2_dev_release_scratch()
    n, edges = lb.case("random-257")
    lb.assert_same_run(capi.graph_layout(n, edges[0], edges[1], _parameters(maxIterationCount=2)), lb.reference("random-257", 2),
                       "after the release")


# ---- the error returns ----

def _raw(entry, n, v0, v1, edge_count, parameters, x, y, result=None):
    lib = capi.load()
    rc = getattr(lib, entry)(n, v0, v1, edge_count, parameters, x, y, result)
    return rc, lib.em2_last_error().decode()


def test_error_returns_and_texts():
    v0, v1 = np.array([0, 1, 2], dtype=np.uint32), np.array([1, 2, 0], dtype=np.uint32)
    x, y = np.full(3, 77., dtype=np.float32), np.full(3, 77., dtype=np.float32)
    p = _parameters(maxIterationCount=3)
    ok = (capi._ptr(v0), capi._ptr(v1), 3, ctypes.byref(p), capi._ptr(x), capi._ptr(y))
    entry = "em2_graph_layout"
    assert _raw(entry, 3, *ok)[0] == 0 and not np.any(x == 77.)
    # null pointers
    for position in (0, 1, 3, 4, 5):
        arguments = list(ok)
        arguments[position] = None
        assert _raw(entry, 3, *arguments) == (INVALID, entry + ": null pointer")
    assert _raw(entry, 3, None, None, 0, *ok[3:])[0] == 0                    # no edges: the arrays may be missing
    # an edge end outside the graph: refused before anything indexes with it, nothing written
    for bad in (3, 4, 0xffffffff):
        for array in (v0, v1):
            broken = array.copy()
            broken[1] = bad
            x[:] = 77.
            arguments = (capi._ptr(broken), capi._ptr(v1)) if array is v0 else (capi._ptr(v0), capi._ptr(broken))
            assert _raw(entry, 3, *arguments, *ok[2:]) == (INVALID, entry + ": an edge names a vertex outside the graph")
            assert np.all(x == 77.)
    # no vertex: EM2_OK, nothing written, also without the arrays
    x[:] = 77.
    result = capi.LayoutResult()
    assert _raw(entry, 0, None, None, 0, ctypes.byref(p), capi._ptr(x), capi._ptr(y), ctypes.byref(result))[0] == 0
    assert _raw(entry, 0, None, None, 0, ctypes.byref(p), None, None)[0] == 0
    assert np.all(x == 77.) and result.iterationCount == 0
    assert _raw(entry, 0, *ok) == (INVALID, entry + ": an edge names a vertex outside the graph")
    # negative and NaN parameters
    for field in ("tolerance", "gravity", "initialStep"):
        for value in (-1e-9, float("nan"), -float("inf")):
            broken = _parameters(**{field: value})
            assert _raw(entry, 3, *ok[:3], ctypes.byref(broken), *ok[4:]) == (INVALID, "%s: %s must not be negative" % (entry, field))
    zero = _parameters(tolerance=0., gravity=0., maxIterationCount=2)
    assert _raw(entry, 3, *ok[:3], ctypes.byref(zero), *ok[4:])[0] == 0
    # the forces entry
    entry = "em2_graph_layout_forces"
    lib = capi.load()
    fx, fy = np.zeros(3, dtype=np.float32), np.zeros(3, dtype=np.float32)
    energy = ctypes.c_double(0.)
    good = [3, capi._ptr(v0), capi._ptr(v1), 3, 0.02, capi._ptr(x), capi._ptr(y), capi._ptr(fx), capi._ptr(fy), ctypes.byref(energy)]
    assert lib.em2_graph_layout_forces(*good) == 0
    for position in (1, 2, 5, 6, 7, 8):
        arguments = list(good)
        arguments[position] = None
        assert (lib.em2_graph_layout_forces(*arguments), lib.em2_last_error().decode()) == (INVALID, entry + ": null pointer")
    broken = v1.copy()
    broken[2] = 3
    arguments = list(good)
    arguments[2] = capi._ptr(broken)
    assert (lib.em2_graph_layout_forces(*arguments), lib.em2_last_error().decode()) == (
        INVALID, entry + ": an edge names a vertex outside the graph")
    arguments = list(good)
    arguments[4] = float("nan")
    assert (lib.em2_graph_layout_forces(*arguments), lib.em2_last_error().decode()) == (INVALID, entry + ": gravity must not be negative")


def test_device_entry_refuses_an_edge_outside_the_graph():
    import torch
    d_v0 = torch.tensor([0, 1, 5], dtype=torch.int32, device="cuda")
    d_v1 = torch.tensor([1, 2, 0], dtype=torch.int32, device="cuda")
    d_x = torch.full((3,), 77., dtype=torch.float32, device="cuda")
    d_y = torch.full((3,), 77., dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    p = _parameters()
    assert _raw("em2_dev_graph_layout", 3, d_v0.data_ptr(), d_v1.data_ptr(), 3, ctypes.byref(p), d_x.data_ptr(), d_y.data_ptr()) == (
        INVALID, "em2_dev_graph_layout: an edge names a vertex outside the graph")
    assert d_x.cpu().tolist() == [77.] * 3


# ---- end to end through ExpressionMatrix ----

@pytest.fixture(scope="module")
def matrix(tmp_path_factory):
    cells, genes = 300, 120
    toc, g, c = synth.expression_matrix(cells, genes, density=0.2, cluster_count=3, seed=9)
    directory = str(tmp_path_factory.mktemp("layout") / "data")
    files.create_directory(directory, genes, toc, capi.make_counts(g, c))
    e = ExpressionMatrix(directory)
    e.findSimilarPairs0(similarPairsName="Exact", k=10, similarityThreshold=0.1)
    yield e
    e.close()


@pytest.mark.parametrize("keep", [False, True])
def test_facade(matrix, keep):
    e = matrix
    name = "Graph-%s" % keep
    e.createCellGraph(graphName=name, similarPairsName="Exact", similarityThreshold=0.3, k=4, keepIsolatedVertices=keep)
    with pytest.raises(RuntimeError) as error:
        e.getCellGraphVertices(name)
    assert str(error.value) == "Layout for graph %s is not available." % name
    g = e._cell_graph(name)
    v0, v1 = g["edgeVertices"]
    assert g["vertexCount"] > 10 and g["edgeCount"] > 10
    e.computeCellGraphLayout(name, seed=5, maxIterationCount=30, tolerance=0.02, gravity=0.1)
    vertices = e.getCellGraphVertices(name)
    x, y, iterations, _, _ = capi.graph_layout(g["vertexCount"], v0, v1, _parameters(seed=5, maxIterationCount=30, tolerance=0.02, gravity=0.1))
    assert iterations > 0 and len(vertices) == g["vertexCount"]
    assert [v.cellId for v in vertices] == g["vertexCellIds"].tolist()
    assert [v.x() for v in vertices] == x.astype(np.float64).tolist() and [v.y() for v in vertices] == y.astype(np.float64).tolist()
    assert all(type(v) is CellGraphVertexInfo and type(v.cellId) is int and type(v.x()) is float for v in vertices)
    # the second call is a no-op, whatever its arguments
    e.computeCellGraphLayout(name, seed=6, maxIterationCount=1)
    again = e.getCellGraphVertices(name)
    assert again == vertices and not (again[0] != vertices[0])
    # the equality of src/CellGraph.hpp:151-154: the cell id and the position
    assert CellGraphVertexInfo(3, (1., 2.)) == CellGraphVertexInfo(3, (1., 2.))
    assert CellGraphVertexInfo(3, (1., 2.)) != CellGraphVertexInfo(4, (1., 2.))
    assert CellGraphVertexInfo(3, (1., 2.)) != CellGraphVertexInfo(3, (1., 2.5))


def test_facade_default_arguments_and_unknown_graphs(matrix):
    e = matrix
    e.createCellGraph(graphName="Defaults", similarPairsName="Exact", similarityThreshold=0.3, k=4)
    e.computeCellGraphLayout("Defaults")
    g = e._cell_graph("Defaults")
    x, y, _, _, _ = capi.graph_layout(g["vertexCount"], *g["edgeVertices"])
    assert [v.x() for v in e.getCellGraphVertices("Defaults")] == x.astype(np.float64).tolist()
    for call in (lambda: e.computeCellGraphLayout("Missing"), lambda: e.getCellGraphVertices("Missing")):
        with pytest.raises(RuntimeError) as error:
            call()
        assert str(error.value) == "Graph Missing does not exist."
