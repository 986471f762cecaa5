"""The multilevel entries of the layout on the GPU (csrc/em2_layout.hip) against
tests/native/em2_layout_multilevel_restatement.cpp, which tests/test_layout_multilevel_cpu.py holds against a Python greedy
matching, a float64 numpy statement of the weighted force and the single-level restatements.  Everything about the levels is
integer arithmetic and every rounding of the forces is part of the contract: mates, maps, masses, edges, rounds, positions,
iteration counts, final step and final energy equal the restatement's exactly."""
import ctypes

import numpy as np
import pytest

import layout_binding as lb
import layout_multilevel_binding as mb
import layout_pyramid_binding as pb
import synth
from expressionmatrix2_amd import ExpressionMatrix, capi, files

pytestmark = pytest.mark.gpu

INVALID = 1
SEED = lb.DEFAULTS["seed"]
EXACT, AUTO = mb.DEPTH_EXACT, mb.DEPTH_AUTO
# the restatement's exact sum over 2 049 or more vertices costs seconds at the default budget of every level
SHORT = 25


def _parameters(**changes):
    p = dict(lb.DEFAULTS)
    p.update(changes)
    return capi.LayoutParameters(**p)


def _same_step(mine, theirs, what):
    for key in ("mate", "coarseOf", "coarseMass"):
        assert np.array_equal(mine[key], theirs[key]), "%s: %s" % (what, key)
    assert (mine["coarseCount"], mine["rounds"]) == (theirs["coarseCount"], theirs["rounds"]), what
    for k in range(3):
        assert np.array_equal(mine["coarseEdges"][k], theirs["coarseEdges"][k]), "%s: coarse edges" % what


# ---- em2_graph_layout_coarsen ----

@pytest.mark.parametrize("name", mb.COARSEN_CASES)
def test_one_coarsening_step_equals_the_restatement(name):
    """n = 1; one edge; a path of 3; a star (one pair, 599 vertices left over); a ring; two cliques; no edge at all; loops (ignored)
    and repeats (weight 3 and the first edge taken); random graphs over one and many workgroups; the path whose weights ascend
    (20 rounds, one pair each); 256 and 257 vertices, the edge of a workgroup."""
    n, edges = mb.case(name)
    for level in (0, 3):
        mine = capi.graph_layout_coarsen(n, edges[0], edges[1], SEED, level)
        _same_step(mine, mb.load().coarsen(n, edges, SEED, level), "%s at level %d" % (name, level))
    mb.check_contraction(n, edges, mine)


def test_the_ascending_path_takes_20_rounds_and_is_still_the_greedy_matching():
    n, edges = mb.case("ascending-path-40")
    mine = capi.graph_layout_coarsen(n, edges[0], edges[1], SEED, 0)
    assert mine["rounds"] == 20
    assert np.array_equal(mine["mate"], mb.python_greedy(n, mb.merged_edges(edges), SEED, 0))


def test_loops_are_ignored_and_repeats_become_a_weight():
    n, edges = lb.case("loops-and-repeats")
    mine = capi.graph_layout_coarsen(n, edges[0], edges[1], SEED, 0)
    assert mine["mate"][1] == 2 and mine["mate"][2] == 1                              # (1, 2) is there three times
    # as weights on the merged edges the same graph gives the same step
    merged = mb.merged_edges(edges)
    a, b = np.array([e[0] for e in merged], np.uint32), np.array([e[1] for e in merged], np.uint32)
    again = capi.graph_layout_coarsen(n, a, b, SEED, 0, edge_weight=np.array(list(merged.values()), np.uint32))
    _same_step(again, mine, "merged by hand")


@pytest.mark.parametrize("name", ["random-257", "random-2049"])
def test_a_second_level_on_weighted_input_with_masses(name):
    n, edges = lb.case(name)
    first = mb.load().coarsen(n, edges, SEED, 0)
    n1, mass, (a, b, w) = first["coarseCount"], first["coarseMass"], first["coarseEdges"]
    assert mass.max() == 2 and w.max() >= 2
    mine = capi.graph_layout_coarsen(n1, a, b, SEED, 1, mass=mass, edge_weight=w)
    _same_step(mine, mb.load().coarsen(n1, (a, b), SEED, 1, mass, w), name + ", level 1")
    mb.check_contraction(n1, (a, b), mine, mass, w)
    assert np.array_equal(mine["mate"], mb.python_greedy(n1, mb.merged_edges((a, b), w), SEED, 1))
    assert mine["coarseMass"].max() > 2


# ---- em2_graph_layout_forces_weighted ----

@pytest.mark.parametrize("exact", [True, False])
@pytest.mark.parametrize("name", pb.POSITION_SETS)
def test_weighted_forces_at_set_positions(name, exact):
    """The position sets of the pyramid's tests with masses 1 ... 7 and weights 1 ... 3, at the exact repulsion and at each
    set's own depth: bit for bit against the restatement, and within the bound of the numpy statement."""
    x, y, depth = pb.position_set(name)
    depth = EXACT if exact else depth
    n, edges = len(x), pb.position_set_edges(len(x))
    mass, weights = mb.position_set_weights(n)
    fx, fy, energy = capi.graph_layout_forces_weighted(n, edges[0], edges[1], 0.02, x, y, depth, mass, weights)
    rx, ry, renergy, _ = mb.load().forces_weighted(n, edges, 0.02, x, y, depth, mass, weights)
    assert np.array_equal(lb.bits(fx), lb.bits(rx)) and np.array_equal(lb.bits(fy), lb.bits(ry))
    assert np.float64(energy).tobytes() == np.float64(renergy).tobytes()
    mb.check_weighted_against_numpy((fx, fy), n, edges, 0.02, x, y, depth, mass, weights, name)


@pytest.mark.parametrize("name", pb.POSITION_SETS + ["random-257", "random-2049"])
def test_unit_masses_and_weights_give_the_bits_of_the_unweighted_entries(name):
    if name in pb.POSITION_SETS:
        x, y, depth = pb.position_set(name)
        n, edges = len(x), pb.position_set_edges(len(x))
    else:
        n, edges = lb.case(name)
        (x, y), depth = pb._cloud(n, 12), pb.automatic_depth(n)
    exact = capi.graph_layout_forces(n, edges[0], edges[1], 0.02, x, y)
    pyramid = capi.graph_layout_forces_pyramid(n, edges[0], edges[1], 0.02, x, y, depth=depth)
    for mass, weights in ((None, None), (np.ones(n, np.uint32), np.ones(len(edges[0]), np.uint32))):
        for theirs, d in ((exact, EXACT), (pyramid, depth)):
            mine = capi.graph_layout_forces_weighted(n, edges[0], edges[1], 0.02, x, y, d, mass, weights)
            assert np.array_equal(lb.bits(mine[0]), lb.bits(theirs[0])) and np.array_equal(lb.bits(mine[1]), lb.bits(theirs[1]))
            assert np.float64(mine[2]).tobytes() == np.float64(theirs[2]).tobytes()


def test_weighted_forces_of_a_coarse_level_over_many_workgroups():
    """Level 1 of random-2049 (1 166 vertices: five workgroups, slices of 73) at the exact repulsion, depth 3 and the automatic depth."""
    n, edges = lb.case("random-2049")
    first = mb.load().coarsen(n, edges, SEED, 0)
    n1, mass, (a, b, w) = first["coarseCount"], first["coarseMass"], first["coarseEdges"]
    x, y = pb._cloud(n1, 31)
    for depth in (EXACT, 3, AUTO):
        fx, fy, energy = capi.graph_layout_forces_weighted(n1, a, b, 0.5, x, y, depth, mass, w)
        rx, ry, renergy, _ = mb.load().forces_weighted(n1, (a, b), 0.5, x, y, depth, mass, w)
        assert np.array_equal(lb.bits(fx), lb.bits(rx)) and np.array_equal(lb.bits(fy), lb.bits(ry))
        assert np.float64(energy).tobytes() == np.float64(renergy).tobytes()


# ---- whole runs ----

def _budget(name):
    n = lb.case(name)[0]
    return SHORT if n >= 2000 else lb.DEFAULTS["maxIterationCount"]


@pytest.mark.parametrize("depth", [EXACT, AUTO])
@pytest.mark.parametrize("name", lb.CASES)
def test_run_equals_the_restatement(name, depth):
    """Positions, total and per-level iterations, level sizes, rounds, step and energy."""
    n, edges = lb.case(name)
    for iterations in sorted({0, 2, _budget(name)}):
        mine = capi.graph_layout_multilevel(n, edges[0], edges[1], _parameters(maxIterationCount=iterations), depth)
        mb.assert_same_multilevel_run(mine, mb.reference(name, iterations, depth), "%s, %d iterations a level" % (name, iterations))
        assert mine[2] == sum(level[3] for level in mine[5])


@pytest.mark.parametrize("depth", [0, 3])
def test_forced_depths_on_every_level(depth):
    n, edges = lb.case("random-2049")
    mine = capi.graph_layout_multilevel(n, edges[0], edges[1], _parameters(maxIterationCount=SHORT), depth)
    mb.assert_same_multilevel_run(mine, mb.reference("random-2049", SHORT, depth), "random-2049 at depth %d" % depth)
    assert len(mine[5]) > 4


@pytest.mark.parametrize("gravity,tolerance,step,seed", [(0., 0.01, 1., 231), (0.5, 0.05, 3., 7), (0.02, 0.3, 0.25, 0)])
def test_other_parameters_equal_the_restatement(gravity, tolerance, step, seed):
    for name in ("random-257", "isolated", "ring-70"):
        n, edges = lb.case(name)
        changes = dict(gravity=gravity, tolerance=tolerance, initialStep=step, seed=seed, maxIterationCount=60)
        mine = capi.graph_layout_multilevel(n, edges[0], edges[1], _parameters(**changes), EXACT)
        mb.assert_same_multilevel_run(mine, mb.load().layout(n, edges, depth=EXACT, **changes), name)


@pytest.mark.parametrize("name", mb.ONE_LEVEL_CASES)
def test_a_graph_of_one_level_equals_the_single_level_entries(name):
    n, edges = lb.case(name)
    parameters = _parameters(maxIterationCount=40)
    exact = capi.graph_layout_multilevel(n, edges[0], edges[1], parameters, EXACT)
    assert len(exact[5]) == 1 and exact[5][0][0] == n and exact[5][0][2:] == (0, exact[2])
    lb.assert_same_run(exact[:5], capi.graph_layout(n, edges[0], edges[1], parameters), name + ", exact")
    for depth in (AUTO, 2):
        mine = capi.graph_layout_multilevel(n, edges[0], edges[1], parameters, depth)
        lb.assert_same_run(mine[:5], capi.graph_layout_pyramid(n, edges[0], edges[1], parameters, depth), "%s at depth %#x" % (name, depth))


@pytest.mark.parametrize("name", ["random-1", "random-65", "random-2049", "no-edges", "ring-70", "loops-and-repeats"])
def test_device_entry_equals_the_host_entry_and_a_call_repeats_itself(name):
    n, edges = lb.case(name)
    parameters = _parameters(maxIterationCount=20)
    for depth in (EXACT, AUTO):
        first = capi.graph_layout_multilevel(n, edges[0], edges[1], parameters, depth)
        second = capi.graph_layout_multilevel(n, edges[0], edges[1], parameters, depth)
        device = capi.dev_graph_layout_multilevel(n, edges[0], edges[1], parameters, depth)
        mb.assert_same_multilevel_run(second, first, name + ", again")
        mb.assert_same_multilevel_run(device, first, name + ", device entry")


def test_the_single_level_entries_are_untouched_by_a_multilevel_call_before_them():
    """(they share their scratch and all their kernels)"""
    n, edges = lb.case("random-257")
    capi.graph_layout_multilevel(n, edges[0], edges[1], _parameters(maxIterationCount=3), 4)
    lb.assert_same_run(capi.graph_layout(n, edges[0], edges[1], _parameters(maxIterationCount=3)), lb.reference("random-257", 3), "exact")
    lb.assert_same_run(capi.graph_layout_pyramid(n, edges[0], edges[1], _parameters(maxIterationCount=3)), pb.reference("random-257", 3),
                       "pyramid")


# ---- what the levels are for ----

def test_the_multilevel_layout_of_the_grid_has_the_lower_stress():
    """The 48 x 48 grid with the default parameters, every level exact: below the threshold tests/layout_multilevel_binding.py
    states (the geometric mean of the two stresses measured on a CPU), and below the single-level stress of this process."""
    n, edges = mb.case("grid-48")
    single = capi.graph_layout(n, edges[0], edges[1], _parameters())
    multi = capi.graph_layout_multilevel(n, edges[0], edges[1], _parameters(), EXACT)
    stress_single = mb.stress(single[0], single[1], mb.grid_distance(48))
    stress_multi = mb.stress(multi[0], multi[1], mb.grid_distance(48))
    print("grid-48: single level %.6f, multilevel %.6f, threshold %.6f; levels %r" % (stress_single, stress_multi, mb.GRID_STRESS_THRESHOLD,
                                                                                       multi[5]))
    assert stress_multi < mb.GRID_STRESS_THRESHOLD
    assert stress_multi < stress_single


# ---- the error returns ----

def _raw(entry, *arguments):
    lib = capi.load()
    rc = getattr(lib, entry)(*arguments)
    return rc, lib.em2_last_error().decode()


def test_error_returns_leave_the_outputs_untouched():
    v0, v1 = np.array([0, 1, 2], dtype=np.uint32), np.array([1, 2, 0], dtype=np.uint32)
    x, y = np.full(3, 77., dtype=np.float32), np.full(3, 77., dtype=np.float32)
    p = _parameters(maxIterationCount=3)
    result, levels = capi.LayoutResult(), capi.LayoutLevels()
    result.iterationCount, levels.levelCount = 77, 77
    entry = "em2_graph_layout_multilevel"
    ok = [3, capi._ptr(v0), capi._ptr(v1), 3, ctypes.byref(p), AUTO, capi._ptr(x), capi._ptr(y), ctypes.byref(result), ctypes.byref(levels)]

    def untouched():
        return np.all(x == 77.) and np.all(y == 77.) and result.iterationCount == 77 and levels.levelCount == 77

    for bad in (3, 0xffffffff):
        for position, array in ((1, v0), (2, v1)):
            broken = array.copy()
            broken[1] = bad
            arguments = list(ok)
            arguments[position] = capi._ptr(broken)
            assert _raw(entry, *arguments) == (INVALID, entry + ": an edge names a vertex outside the graph")
            assert untouched()
    arguments = list(ok)
    arguments[5] = 11
    assert _raw(entry, *arguments) == (INVALID, entry + ": depth must be at most 10 or the automatic depth")
    assert untouched()
    nan = _parameters(tolerance=float("nan"))
    arguments = list(ok)
    arguments[4] = ctypes.byref(nan)
    assert _raw(entry, *arguments) == (INVALID, entry + ": tolerance must not be negative")
    assert untouched()
    assert _raw(entry, *ok)[0] == 0 and not np.any(x == 77.) and result.iterationCount == 3 and levels.levelCount == 1


def test_device_entry_refuses_an_edge_outside_the_graph_and_leaves_the_positions():
    import torch
    d_v0 = torch.tensor([0, 1, 5], dtype=torch.int32, device="cuda")
    d_v1 = torch.tensor([1, 2, 0], dtype=torch.int32, device="cuda")
    d_x = torch.full((3,), 77., dtype=torch.float32, device="cuda")
    d_y = torch.full((3,), 77., dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    p = _parameters()
    entry = "em2_dev_graph_layout_multilevel"
    assert _raw(entry, 3, d_v0.data_ptr(), d_v1.data_ptr(), 3, ctypes.byref(p), EXACT, d_x.data_ptr(), d_y.data_ptr(), None, None) == (
        INVALID, entry + ": an edge names a vertex outside the graph")
    assert _raw(entry, 3, d_v1.data_ptr(), d_v1.data_ptr(), 3, ctypes.byref(p), 11, d_x.data_ptr(), d_y.data_ptr(), None, None) == (
        INVALID, entry + ": depth must be at most 10 or the automatic depth")
    assert d_x.cpu().tolist() == [77.] * 3 and d_y.cpu().tolist() == [77.] * 3


def test_the_test_entries_refuse_an_edge_outside_the_graph():
    v0, v1 = np.array([0, 1], dtype=np.uint32), np.array([1, 3], dtype=np.uint32)
    with pytest.raises(Exception) as error:
        capi.graph_layout_coarsen(3, v0, v1, SEED, 0)
    assert "an edge names a vertex outside the graph" in str(error.value)
    with pytest.raises(Exception) as error:
        capi.graph_layout_forces_weighted(3, v0, v1, 0.02, np.zeros(3, np.float32), np.zeros(3, np.float32))
    assert "an edge names a vertex outside the graph" in str(error.value)


# ---- end to end through ExpressionMatrix ----

@pytest.fixture(scope="module")
def matrix(tmp_path_factory):
    cells, genes = 300, 120
    toc, g, c = synth.expression_matrix(cells, genes, density=0.2, cluster_count=3, seed=9)
    directory = str(tmp_path_factory.mktemp("layout-multilevel") / "data")
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
    for name in ("Multi", "MultiPyramid", "Default", "Single"):
        e.createCellGraph(graphName=name, similarPairsName="Exact", similarityThreshold=0.3, k=4)
    g = e._cell_graph("Multi")
    v0, v1 = g["edgeVertices"]
    assert g["vertexCount"] > 64 and g["edgeCount"] > 10
    with pytest.raises(ValueError) as error:
        e.computeCellGraphLayout("Multi", levels="bogus", **arguments)
    assert '"single"' in str(error.value) and '"multi"' in str(error.value)
    with pytest.raises(RuntimeError):
        e.getCellGraphVertices("Multi")                                                # nothing was computed by the refused call

    e.computeCellGraphLayout("Multi", levels="multi", **arguments)
    run = capi.graph_layout_multilevel(g["vertexCount"], v0, v1, _parameters(**arguments), EXACT)
    assert len(run[5]) > 1 and _stored(e, "Multi") == (run[0].astype(np.float64).tolist(), run[1].astype(np.float64).tolist())
    e.computeCellGraphLayout("MultiPyramid", levels="multi", repulsion="pyramid", **arguments)
    run = capi.graph_layout_multilevel(g["vertexCount"], v0, v1, _parameters(**arguments), AUTO)
    assert _stored(e, "MultiPyramid") == (run[0].astype(np.float64).tolist(), run[1].astype(np.float64).tolist())

    # the default call and levels="single" give what they gave before there were levels
    ex, ey, _, _, _ = capi.graph_layout(g["vertexCount"], v0, v1, _parameters(**arguments))
    e.computeCellGraphLayout("Default", **arguments)
    e.computeCellGraphLayout("Single", levels="single", **arguments)
    assert _stored(e, "Default") == _stored(e, "Single") == (ex.astype(np.float64).tolist(), ey.astype(np.float64).tolist())
    assert _stored(e, "Multi") != _stored(e, "Default")
