"""The pyramid entries of the layout on the GPU (csrc/em2_layout.hip) against
tests/native/em2_layout_pyramid_restatement.cpp, which tests/test_layout_pyramid_cpu.py holds against a float64 numpy statement
of the approximation and against the exact model.  The order of every rounding is part of the contract: positions, iteration
count, final step and final energy equal the restatement's bit for bit."""
import ctypes

import numpy as np
import pytest

import layout_binding as lb
import layout_pyramid_binding as pb
import synth
from expressionmatrix2_amd import ExpressionMatrix, capi, files

pytestmark = pytest.mark.gpu

INVALID = 1
DEFAULT = lb.DEFAULTS["maxIterationCount"]


def _parameters(**changes):
    p = dict(lb.DEFAULTS)
    p.update(changes)
    return capi.LayoutParameters(**p)


@pytest.mark.parametrize("name", lb.CASES)
def test_run_equals_the_restatement(name):
    """At the automatic depth.  N = 63, 64, 65 hold the wave; 255, 256, 257 the energy chunk in vertex order against the walk in
    sorted order; 2 049 and 4 100 have depth 5 (depth 6 is forced below).  The restatement is cheap, so every size runs the default too."""
    n, edges = lb.case(name)
    for iterations in (0, 1, 2, 25, DEFAULT):
        mine = capi.graph_layout_pyramid(n, edges[0], edges[1], _parameters(maxIterationCount=iterations))
        lb.assert_same_run(mine, pb.reference(name, iterations), "%s after %d iterations" % (name, iterations))
        assert mine[2] == iterations or iterations == DEFAULT


def test_the_depths_of_the_cases_and_depth_6():
    """2 049 and 4 100 vertices both have the automatic depth 5 (8 * 4^5 = 8 192); depth 6 is forced here."""
    assert [pb.automatic_depth(n) for n in (1, 9, 65, 257, 2048, 2049, 4100)] == [0, 1, 2, 3, 4, 5, 5]
    n, edges = lb.case("random-4100")
    mine = capi.graph_layout_pyramid(n, edges[0], edges[1], _parameters(maxIterationCount=3), depth=6)
    lb.assert_same_run(mine, pb.reference("random-4100", 3, 6), "random-4100 at depth 6")


@pytest.mark.parametrize("depth", [0, 1, 2, 3, 10])
@pytest.mark.parametrize("n", [9, 65, 257])
def test_forced_depths(n, depth):
    """Depths 0 and 1 have no far field, 2 is the first level with one, 10 is a pyramid almost wholly empty."""
    name = "random-%d" % n
    n, edges = lb.case(name)
    for iterations in (1, 20):
        mine = capi.graph_layout_pyramid(n, edges[0], edges[1], _parameters(maxIterationCount=iterations), depth=depth)
        lb.assert_same_run(mine, pb.reference(name, iterations, depth), "%s at depth %d after %d iterations" % (name, depth, iterations))


def test_depth_0_differs_from_the_exact_entry_only_in_the_order_of_the_sum():
    n, edges = lb.case("random-65")
    x, y = pb._cloud(n, 3)
    fx, fy, _ = capi.graph_layout_forces_pyramid(n, edges[0], edges[1], 0.02, x, y, depth=0)
    f, absolute = lb.numpy_forces(n, edges, 0.02, x, y)
    assert np.all(np.abs(np.stack([fx, fy], axis=1).astype(np.float64) - f) <= lb.force_bound(n, absolute))


@pytest.mark.parametrize("name", pb.POSITION_SETS)
def test_forces_at_set_positions(name):
    """One vertex; two coincident; all coincident (S = 0); a vertical line (one extent zero); a vertex at xmax and one at ymax
    (u = 1, the clamp to the last cell); positions on exact cell boundaries; coincident pairs in a cloud; 2 000 vertices in
    one leaf with 48 spread over the box (a wave with near-field lists of 2 000 and of 1).  Bit for bit against the
    restatement, and within the bound of tests/test_layout_pyramid_cpu.py of the numpy statement."""
    x, y, depth = pb.position_set(name)
    n, edges = len(x), pb.position_set_edges(len(x))
    fx, fy, energy = capi.graph_layout_forces_pyramid(n, edges[0], edges[1], 0.02, x, y, depth=depth)
    rx, ry, renergy, _ = pb.load().forces(n, edges, 0.02, x, y, depth)
    assert np.array_equal(lb.bits(fx), lb.bits(rx)) and np.array_equal(lb.bits(fy), lb.bits(ry))
    assert np.float64(energy).tobytes() == np.float64(renergy).tobytes()
    pb.check_against_numpy((fx, fy), n, edges, 0.02, x, y, depth, name)


@pytest.mark.parametrize("name,gravity", [("random-257", 0.02), ("random-2049", 0.5), ("star-600", 0.)])
def test_forces_at_the_automatic_depth(name, gravity):
    n, edges = lb.case(name)
    x, y = pb._cloud(n, 17)
    fx, fy, energy = capi.graph_layout_forces_pyramid(n, edges[0], edges[1], gravity, x, y)
    rx, ry, renergy, _ = pb.load().forces(n, edges, gravity, x, y)
    assert np.array_equal(lb.bits(fx), lb.bits(rx)) and np.array_equal(lb.bits(fy), lb.bits(ry))
    assert np.float64(energy).tobytes() == np.float64(renergy).tobytes()
    pb.check_against_numpy((fx, fy), n, edges, gravity, x, y, pb.automatic_depth(n), name)


@pytest.mark.parametrize("gravity,tolerance,step,seed", [(0., 0.01, 1., 231), (0.5, 0.05, 3., 7), (0.02, 0.3, 0.25, 0)])
def test_other_parameters_equal_the_restatement(gravity, tolerance, step, seed):
    for name in ("random-257", "isolated", "loops-and-repeats"):
        n, edges = lb.case(name)
        changes = dict(gravity=gravity, tolerance=tolerance, initialStep=step, seed=seed, maxIterationCount=60)
        mine = capi.graph_layout_pyramid(n, edges[0], edges[1], _parameters(**changes))
        lb.assert_same_run(mine, pb.load().layout(n, edges, **changes), name)


@pytest.mark.parametrize("name", ["random-1", "random-65", "random-2049", "no-edges", "star-600", "loops-and-repeats"])
def test_device_entry_equals_the_host_entry_and_a_call_repeats_itself(name):
    n, edges = lb.case(name)
    parameters = _parameters(maxIterationCount=20)
    first = capi.graph_layout_pyramid(n, edges[0], edges[1], parameters)
    second = capi.graph_layout_pyramid(n, edges[0], edges[1], parameters)
    device = capi.dev_graph_layout_pyramid(n, edges[0], edges[1], parameters)
    forced = capi.dev_graph_layout_pyramid(n, edges[0], edges[1], parameters, depth=pb.automatic_depth(n))
    lb.assert_same_run(second, first, name + ", again")
    lb.assert_same_run(device, first, name + ", device entry")
    lb.assert_same_run(forced, first, name + ", device entry at the forced depth")
    lb.assert_same_run(first, pb.reference(name, 20), name)


def test_the_exact_entry_is_untouched_by_a_pyramid_call_before_it():
    """(the two share their scratch and everything but the repulsion)"""
    n, edges = lb.case("random-257")
    capi.graph_layout_pyramid(n, edges[0], edges[1], _parameters(maxIterationCount=3), depth=10)
    lb.assert_same_run(capi.graph_layout(n, edges[0], edges[1], _parameters(maxIterationCount=3)), lb.reference("random-257", 3), "exact")
    lb.assert_same_run(capi.graph_layout_pyramid(n, edges[0], edges[1], _parameters(maxIterationCount=3)), pb.reference("random-257", 3),
                       "pyramid")


# ---- the error returns ----

def _raw(entry, *arguments):
    lib = capi.load()
    rc = getattr(lib, entry)(*arguments)
    return rc, lib.em2_last_error().decode()


def test_error_returns_leave_the_outputs_untouched():
    v0, v1 = np.array([0, 1, 2], dtype=np.uint32), np.array([1, 2, 0], dtype=np.uint32)
    x, y = np.full(3, 77., dtype=np.float32), np.full(3, 77., dtype=np.float32)
    p = _parameters(maxIterationCount=3)
    entry = "em2_graph_layout_pyramid"
    ok = [3, capi._ptr(v0), capi._ptr(v1), 3, ctypes.byref(p), pb.DEPTH_AUTO, capi._ptr(x), capi._ptr(y), None]
    for bad in (3, 0xffffffff):
        for position, array in ((1, v0), (2, v1)):
            broken = array.copy()
            broken[1] = bad
            arguments = list(ok)
            arguments[position] = capi._ptr(broken)
            assert _raw(entry, *arguments) == (INVALID, entry + ": an edge names a vertex outside the graph")
            assert np.all(x == 77.) and np.all(y == 77.)
    arguments = list(ok)
    arguments[5] = 11
    assert _raw(entry, *arguments) == (INVALID, entry + ": depth must be at most 10 or the automatic depth")
    assert np.all(x == 77.) and np.all(y == 77.)
    assert _raw(entry, 0, None, None, 0, ctypes.byref(p), pb.DEPTH_AUTO, None, None, None)[0] == 0
    assert _raw(entry, *ok)[0] == 0 and not np.any(x == 77.)
    # the forces entry
    entry = "em2_graph_layout_forces_pyramid"
    fx, fy = np.full(3, 77., dtype=np.float32), np.full(3, 77., dtype=np.float32)
    good = [3, capi._ptr(v0), capi._ptr(v1), 3, 0.02, 2, capi._ptr(x), capi._ptr(y), capi._ptr(fx), capi._ptr(fy), None]
    broken = v1.copy()
    broken[2] = 3
    arguments = list(good)
    arguments[2] = capi._ptr(broken)
    assert _raw(entry, *arguments) == (INVALID, entry + ": an edge names a vertex outside the graph")
    arguments = list(good)
    arguments[5] = 11
    assert _raw(entry, *arguments) == (INVALID, entry + ": depth must be at most 10 or the automatic depth")
    assert np.all(fx == 77.) and np.all(fy == 77.)
    assert _raw(entry, 0, None, None, 0, 0.02, 2, None, None, None, None, None)[0] == 0
    assert _raw(entry, *good)[0] == 0 and not np.any(fx == 77.)


def test_device_entry_refuses_an_edge_outside_the_graph_and_a_depth_of_11():
    import torch
    d_v0 = torch.tensor([0, 1, 5], dtype=torch.int32, device="cuda")
    d_v1 = torch.tensor([1, 2, 0], dtype=torch.int32, device="cuda")
    d_x = torch.full((3,), 77., dtype=torch.float32, device="cuda")
    d_y = torch.full((3,), 77., dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    p = _parameters()
    entry = "em2_dev_graph_layout_pyramid"
    assert _raw(entry, 3, d_v0.data_ptr(), d_v1.data_ptr(), 3, ctypes.byref(p), pb.DEPTH_AUTO, d_x.data_ptr(), d_y.data_ptr(), None) == (
        INVALID, entry + ": an edge names a vertex outside the graph")
    assert _raw(entry, 3, d_v1.data_ptr(), d_v1.data_ptr(), 3, ctypes.byref(p), 11, d_x.data_ptr(), d_y.data_ptr(), None) == (
        INVALID, entry + ": depth must be at most 10 or the automatic depth")
    assert d_x.cpu().tolist() == [77.] * 3 and d_y.cpu().tolist() == [77.] * 3


# ---- end to end through ExpressionMatrix ----

@pytest.fixture(scope="module")
def matrix(tmp_path_factory):
    cells, genes = 300, 120
    toc, g, c = synth.expression_matrix(cells, genes, density=0.2, cluster_count=3, seed=9)
    directory = str(tmp_path_factory.mktemp("layout-pyramid") / "data")
    files.create_directory(directory, genes, toc, capi.make_counts(g, c))
    e = ExpressionMatrix(directory)
    e.findSimilarPairs0(similarPairsName="Exact", k=10, similarityThreshold=0.1)
    yield e
    e.close()


def _stored(e, name):
    vertices = e.getCellGraphVertices(name)
    return [v.x() for v in vertices], [v.y() for v in vertices]


def test_facade(matrix):
    e = matrix
    arguments = dict(seed=5, maxIterationCount=30, tolerance=0.02, gravity=0.1)
    for name in ("Pyramid", "Exact", "NoArgument"):
        e.createCellGraph(graphName=name, similarPairsName="Exact", similarityThreshold=0.3, k=4)
    g = e._cell_graph("Pyramid")
    v0, v1 = g["edgeVertices"]
    assert g["vertexCount"] > 10 and g["edgeCount"] > 10
    with pytest.raises(ValueError) as error:
        e.computeCellGraphLayout("Pyramid", repulsion="barnes-hut", **arguments)
    assert '"exact"' in str(error.value) and '"pyramid"' in str(error.value)
    with pytest.raises(ValueError):
        e.computeCellGraphLayout("Missing", repulsion="")                              # (raised before the graph is looked up)
    with pytest.raises(RuntimeError):
        e.getCellGraphVertices("Pyramid")                                              # nothing was computed by the refused call

    e.computeCellGraphLayout("Pyramid", repulsion="pyramid", **arguments)
    x, y, iterations, _, _ = capi.graph_layout_pyramid(g["vertexCount"], v0, v1, _parameters(**arguments))
    assert iterations > 0 and _stored(e, "Pyramid") == (x.astype(np.float64).tolist(), y.astype(np.float64).tolist())
    # a second call is a no-op, whatever it asks for
    before = e.getCellGraphVertices("Pyramid")
    e.computeCellGraphLayout("Pyramid", repulsion="exact", seed=6, maxIterationCount=1)
    assert e.getCellGraphVertices("Pyramid") == before

    ex, ey, _, _, _ = capi.graph_layout(g["vertexCount"], v0, v1, _parameters(**arguments))
    e.computeCellGraphLayout("Exact", repulsion="exact", **arguments)
    e.computeCellGraphLayout("NoArgument", **arguments)
    assert _stored(e, "Exact") == _stored(e, "NoArgument") == (ex.astype(np.float64).tolist(), ey.astype(np.float64).tolist())
    assert not np.array_equal(x, ex)
