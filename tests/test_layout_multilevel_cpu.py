"""tests/native/em2_layout_multilevel_restatement.cpp -- what the multilevel entries of csrc/em2_layout.hip must equal bit for
bit (tests/test_gpu_layout_multilevel.py) -- against an independent Python greedy matching and the rounds of locally dominant
edges, for the invariants of the contraction, against a float64 numpy statement of the weighted force, against the single-level
restatements where the two must coincide, and for the quality the levels are there for.  Then the argument
checks that need no device.  No GPU."""
import ctypes

import numpy as np
import pytest

import layout_binding as lb
import layout_multilevel_binding as mb
import layout_pyramid_binding as pb
from expressionmatrix2_amd import capi

INVALID, UNSUPPORTED = 1, 6
SEED = lb.DEFAULTS["seed"]


@pytest.fixture(scope="module")
def restatement():
    return mb.load()


# ---- coarsening ----

@pytest.mark.parametrize("name", ["ring-70", "ring-2000", "star-600", "grid-48", "random-257", "random-2049", "cliques",
                                  "loops-and-repeats", "ascending-path-40", "isolated"])
def test_matching_equals_the_python_greedy_and_the_rounds_on_every_level(restatement, name):
    """Level by level until the stop rule: the restatement's mates are those of the greedy matching stated in Python and those
    of the rounds of locally dominant edges; its round count is the rounds'; the contraction keeps its invariants."""
    n, edges = mb.case(name)
    mass, weights = None, None
    ratios = []
    for level in range(mb.MAX_LEVELS):
        out = restatement.coarsen(n, edges, SEED, level, mass, weights)
        merged = mb.merged_edges(edges, weights)
        greedy = mb.python_greedy(n, merged, SEED, level)
        by_rounds, rounds = mb.python_rounds(n, merged, SEED, level)
        assert np.array_equal(out["mate"], greedy), "%s level %d" % (name, level)
        assert np.array_equal(by_rounds, greedy) and out["rounds"] == rounds, "%s level %d" % (name, level)
        # maximal: no edge between two unmatched vertices
        assert not any(greedy[a] == mb.NONE and greedy[b] == mb.NONE for a, b in merged)
        mb.check_contraction(n, edges, out, mass, weights)
        if n <= mb.COARSEST or 4 * out["coarseCount"] > 3 * n:
            break
        ratios.append(out["coarseCount"] / n)
        n, mass = out["coarseCount"], out["coarseMass"]
        edges, weights = (out["coarseEdges"][0], out["coarseEdges"][1]), out["coarseEdges"][2]
    print(name, "ratios", ["%.2f" % r for r in ratios])


def test_the_ascending_path_takes_20_rounds(restatement):
    n, edges = mb.case("ascending-path-40")
    out = restatement.coarsen(n, edges, SEED, 0)
    assert out["rounds"] == 20 and out["coarseCount"] == 20
    assert out["mate"].tolist() == [i ^ 1 for i in range(40)]
    assert out["coarseEdges"][2].tolist() == [2 * i + 2 for i in range(19)]          # the edges between the pairs keep their weights


def test_loops_are_ignored_and_repeats_add_up(restatement):
    n, edges = lb.case("loops-and-repeats")
    out = restatement.coarsen(n, edges, SEED, 0)
    merged = mb.merged_edges(edges)
    assert merged[(1, 2)] == 3 and (0, 0) not in merged and (5, 5) not in merged and len(merged) == 8
    assert out["mate"][1] == 2 and out["mate"][2] == 1                                # the heaviest edge is taken first


def test_the_levels_of_a_run(restatement):
    """The stop rule and the report: level sizes fall by at least a quarter, the last is small or did not coarsen further."""
    for name, iterations in (("random-2049", 2), ("grid-48", 1), ("ring-70", 3)):
        n, edges = mb.case(name)
        levels = mb.reference(name, iterations, mb.DEPTH_EXACT)[5]
        assert levels[0][0] == n and levels[0][1] == len(mb.merged_edges(edges)) and levels[0][2] == 0
        assert len(levels) > 1
        for fine, coarse in zip(levels, levels[1:]):
            assert 4 * coarse[0] <= 3 * fine[0] and coarse[1] <= fine[1] and coarse[2] >= 1
        assert all(level[3] == iterations for level in levels)
        assert mb.reference(name, iterations, mb.DEPTH_EXACT)[2] == iterations * len(levels)


# ---- the weighted force ----

@pytest.mark.parametrize("exact", [True, False])
@pytest.mark.parametrize("name", pb.POSITION_SETS)
def test_weighted_force_against_the_float64_statement(restatement, name, exact):
    x, y, depth = pb.position_set(name)
    depth = mb.DEPTH_EXACT if exact else depth
    n, edges = len(x), pb.position_set_edges(len(x))
    mass, weights = mb.position_set_weights(n)
    out = restatement.forces_weighted(n, edges, 0.02, x, y, depth, mass, weights)
    mb.check_weighted_against_numpy(out, n, edges, 0.02, x, y, depth, mass, weights, name)
    assert out[2] == pytest.approx(float((np.stack(out[:2], axis=1).astype(np.float64) ** 2).sum()), rel=1e-12)


@pytest.mark.parametrize("depth", [mb.DEPTH_EXACT, 3, 5])
def test_weighted_force_of_a_coarse_level_against_the_float64_statement(restatement, depth):
    """The second level of random-2049 with its own masses and weights, at spread positions."""
    n, edges = lb.case("random-2049")
    out = restatement.coarsen(n, edges, SEED, 0)
    n1, mass, (a, b, w) = out["coarseCount"], out["coarseMass"], out["coarseEdges"]
    assert mass.max() == 2 and w.max() >= 2
    x, y = pb._cloud(n1, 31)
    forces = restatement.forces_weighted(n1, (a, b), 0.02, x, y, depth, mass, w)
    mb.check_weighted_against_numpy(forces, n1, (a, b), 0.02, x, y, depth, mass, w, "level 1 of random-2049")


@pytest.mark.parametrize("name", pb.POSITION_SETS + ["random-257", "loops-and-repeats"])
def test_unit_masses_and_weights_give_the_bits_of_the_unweighted_restatements(restatement, name):
    if name in pb.POSITION_SETS:
        x, y, depth = pb.position_set(name)
        n, edges = len(x), pb.position_set_edges(len(x))
    else:
        n, edges = lb.case(name)
        (x, y), depth = pb._cloud(n, 12), 3
    ones = np.ones(n, np.uint32), np.ones(len(edges[0]), np.uint32)
    exact = lb.load().forces(n, edges, 0.02, x, y)
    pyramid = pb.load().forces(n, edges, 0.02, x, y, depth)
    for mass, weights in ((None, None), ones):
        mine = restatement.forces_weighted(n, edges, 0.02, x, y, mb.DEPTH_EXACT, mass, weights)
        assert np.array_equal(lb.bits(mine[0]), lb.bits(exact[0])) and np.array_equal(lb.bits(mine[1]), lb.bits(exact[1]))
        assert np.float64(mine[2]).tobytes() == np.float64(exact[2]).tobytes()
        mine = restatement.forces_weighted(n, edges, 0.02, x, y, depth, mass, weights)
        assert np.array_equal(lb.bits(mine[0]), lb.bits(pyramid[0])) and np.array_equal(lb.bits(mine[1]), lb.bits(pyramid[1]))
        assert np.float64(mine[2]).tobytes() == np.float64(pyramid[2]).tobytes()
        assert np.array_equal(mine[3], pyramid[3])


# ---- whole runs ----

@pytest.mark.parametrize("name", mb.ONE_LEVEL_CASES + ["random-2", "loops-and-repeats"])
def test_a_graph_of_one_level_is_the_single_level_run(restatement, name):
    n, edges = lb.case(name)
    for iterations in (0, 3, 40):
        exact = restatement.layout(n, edges, depth=mb.DEPTH_EXACT, maxIterationCount=iterations)
        assert exact[5] == [(n, len(mb.merged_edges(edges)), 0, exact[2])]
        lb.assert_same_run(exact[:5], lb.reference(name, iterations), name)
        for depth in (mb.DEPTH_AUTO, 2):
            mine = restatement.layout(n, edges, depth=depth, maxIterationCount=iterations)
            lb.assert_same_run(mine[:5], pb.reference(name, iterations, depth), "%s at depth %#x" % (name, depth))


def test_without_an_iteration_the_run_is_the_prolongation_of_the_start(restatement):
    """maxIterationCount 0: vertex i of the coarsest level starts where vertex i of the input does (the square is the input's),
    and every level below copies its groups' positions, the second member of a pair displaced by its hashed offset."""
    for name in ("ring-70", "random-257", "grid-48"):
        n, edges = mb.case(name)
        run = restatement.layout(n, edges, depth=mb.DEPTH_EXACT, maxIterationCount=0)
        assert run[2] == 0 and run[3] == 1. and run[4] == np.inf and len(run[5]) > 1
        steps, mass, weights, size = [], None, None, n
        for level in range(len(run[5]) - 1):
            out = restatement.coarsen(size, edges, SEED, level, mass, weights)
            steps.append(out)
            size, mass = out["coarseCount"], out["coarseMass"]
            edges, weights = (out["coarseEdges"][0], out["coarseEdges"][1]), out["coarseEdges"][2]
            assert (size, len(weights), out["rounds"]) == run[5][level + 1][:3]
        x, y = lb.load().initial(n, SEED)
        x, y = x[:size].copy(), y[:size].copy()
        for level in range(len(steps) - 1, -1, -1):
            out = steps[level]
            x, y = x[out["coarseOf"]], y[out["coarseOf"]]
            for v in np.flatnonzero((out["mate"] != mb.NONE) & (out["mate"] < np.arange(len(x)))):
                z = mb.level_hash(SEED, level, int(v))
                x[v] += np.float32((z >> 40) * 2. ** -24 - 0.5)
                y[v] += np.float32(((z >> 16) & 0xffffff) * 2. ** -24 - 0.5)
        assert np.array_equal(lb.bits(x), lb.bits(run[0])) and np.array_equal(lb.bits(y), lb.bits(run[1]))


# ---- what the levels are for ----

def test_the_multilevel_layout_of_the_grid_has_the_lower_stress():
    """The 48 x 48 grid, default parameters, every level exact.  Measured with the two restatements (layout_multilevel_binding):
    single level 0.27015, multilevel 0.016152; the gate is their geometric mean, 0.06606, a factor 4.09 from either."""
    x, y = mb.reference("grid-48", lb.DEFAULTS["maxIterationCount"], mb.DEPTH_EXACT)[:2]
    stress = mb.stress(x, y, mb.grid_distance(48))
    print("grid-48: multilevel stress %.6f, threshold %.6f" % (stress, mb.GRID_STRESS_THRESHOLD))
    assert mb.GRID_STRESS_THRESHOLD == pytest.approx(0.06606, rel=1e-3)
    assert stress < mb.GRID_STRESS_THRESHOLD
    assert stress == pytest.approx(mb.GRID_STRESS_MULTI, rel=1e-3)


def test_the_stress_of_a_perfect_and_of_a_folded_grid():
    """The measure itself: 0 for the grid drawn as a grid under the Manhattan metric's best scale is not reached by a Euclidean
    drawing, but it is small; a grid folded onto a line is far worse."""
    side = 48
    v = np.arange(side * side)
    drawn = mb.stress((v % side).astype(np.float32), (v // side).astype(np.float32), mb.grid_distance(side))
    folded = mb.stress((v % side).astype(np.float32), np.zeros(side * side, np.float32), mb.grid_distance(side))
    assert drawn < 0.02 < 0.1 < folded


# ---- the argument checks that need no device ----

E0 = np.array([0, 1], dtype=np.uint32)
E1 = np.array([1, 2], dtype=np.uint32)
F32 = np.zeros(4, dtype=np.float32)
U32 = np.zeros(4, dtype=np.uint32)


def _raw(entry, *arguments):
    lib = capi.load()
    rc = getattr(lib, entry)(*arguments)
    return rc, lib.em2_last_error().decode()


def _layout_arguments(**changes):
    p = capi.LayoutParameters(**changes)
    return p, [4, capi._ptr(E0), capi._ptr(E1), 2, ctypes.byref(p), mb.DEPTH_EXACT, capi._ptr(F32), capi._ptr(F32), None, None]


@pytest.mark.parametrize("entry", ["em2_graph_layout_multilevel", "em2_dev_graph_layout_multilevel"])
def test_argument_checks_of_the_layout_entries(entry):
    keep, good = _layout_arguments()
    for position in (1, 2, 4, 6, 7):
        arguments = list(good)
        arguments[position] = None
        assert _raw(entry, *arguments) == (INVALID, entry + ": null pointer")
    for field in ("tolerance", "gravity", "initialStep"):
        for value in (-1e-9, float("nan")):
            keep, arguments = _layout_arguments(**{field: value})
            assert _raw(entry, *arguments) == (INVALID, "%s: %s must not be negative" % (entry, field))
    keep, good = _layout_arguments()
    for depth in (11, 12, 0xfffffffd, 0x80000000):
        arguments = list(good)
        arguments[5] = depth
        assert _raw(entry, *arguments) == (INVALID, entry + ": depth must be at most 10 or the automatic depth")
    arguments = list(good)
    arguments[0] = 2 ** 30 + 1
    assert _raw(entry, *arguments) == (UNSUPPORTED, entry + ": vertexCount is above 2^30")
    arguments = list(good)
    arguments[3] = 2 ** 32
    assert _raw(entry, *arguments) == (UNSUPPORTED, entry + ": edgeCount is 2^32 or more")
    # no vertex: EM2_OK without the arrays, at every depth; no level; with an edge, the edge is outside the graph
    result, levels = capi.LayoutResult(), capi.LayoutLevels()
    for depth in (mb.DEPTH_EXACT, mb.DEPTH_AUTO, 0, 10):
        levels.levelCount = 9
        assert _raw(entry, 0, None, None, 0, ctypes.byref(keep), depth, None, None, ctypes.byref(result), ctypes.byref(levels))[0] == 0
        assert result.iterationCount == 0 and result.step == 1. and result.energy == np.inf and levels.levelCount == 0
    result.iterationCount, levels.levelCount = 77, 9
    assert _raw(entry, 0, capi._ptr(E0), capi._ptr(E1), 2, ctypes.byref(keep), mb.DEPTH_AUTO, None, None, ctypes.byref(result),
                ctypes.byref(levels)) == (INVALID, entry + ": an edge names a vertex outside the graph")
    assert result.iterationCount == 77 and levels.levelCount == 9


def test_argument_checks_of_the_test_entries():
    entry = "em2_graph_layout_forces_weighted"
    energy = ctypes.c_double(5.)
    e0, e1, f, u = capi._ptr(E0), capi._ptr(E1), capi._ptr(F32), capi._ptr(U32)
    good = [4, None, e0, e1, None, 2, 0.5, mb.DEPTH_EXACT, f, f, f, f, ctypes.byref(energy)]
    for position in (2, 3, 8, 9, 10, 11):
        arguments = list(good)
        arguments[position] = None
        assert _raw(entry, *arguments) == (INVALID, entry + ": null pointer")
    arguments = list(good)
    arguments[7] = 11
    assert _raw(entry, *arguments) == (INVALID, entry + ": depth must be at most 10 or the automatic depth")
    arguments = list(good)
    arguments[1] = u                                                                  # masses of 0
    assert _raw(entry, *arguments) == (INVALID, entry + ": a mass is 0")
    heavy = np.full(4, 2 ** 29, dtype=np.uint32)
    arguments[1] = capi._ptr(heavy)
    assert _raw(entry, *arguments) == (UNSUPPORTED, entry + ": the masses sum to more than 2^30")
    arguments = list(good)
    weights = np.full(2, 2 ** 31, dtype=np.uint32)
    arguments[4] = capi._ptr(weights)
    assert _raw(entry, *arguments) == (UNSUPPORTED, entry + ": the edge weights sum to 2^32 or more")
    assert energy.value == 5.
    assert _raw(entry, 0, None, None, None, None, 0, 0.5, 3, None, None, None, None, ctypes.byref(energy))[0] == 0 and energy.value == 0.

    entry = "em2_graph_layout_coarsen"
    count, rounds, edge_count = ctypes.c_uint32(7), ctypes.c_uint32(7), ctypes.c_uint64(7)
    good = [4, None, e0, e1, None, 2, 231, 0, u, u, ctypes.byref(count), ctypes.byref(rounds), u, u, u, u, ctypes.byref(edge_count)]
    for position in (2, 3, 8, 9, 10, 11, 12, 13, 14, 15, 16):
        arguments = list(good)
        arguments[position] = None
        assert _raw(entry, *arguments) == (INVALID, entry + ": null pointer")
    arguments = list(good)
    arguments[0] = 0
    assert _raw(entry, *arguments) == (INVALID, entry + ": vertexCount must not be 0")
    assert (count.value, rounds.value, edge_count.value) == (7, 7, 7)


def test_the_facade_refuses_other_levels_before_anything_else():
    """(before the graph is looked up: the graph named here does not exist, and no store is open)"""
    from expressionmatrix2_amd import ExpressionMatrix
    with pytest.raises(ValueError) as error:
        ExpressionMatrix.computeCellGraphLayout(None, "Missing", levels="bogus")
    assert '"single"' in str(error.value) and '"multi"' in str(error.value)
