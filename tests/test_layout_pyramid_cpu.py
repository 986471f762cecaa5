"""tests/native/em2_layout_pyramid_restatement.cpp -- what the pyramid entries of csrc/em2_layout.hip must equal bit for bit
(tests/test_gpu_layout_pyramid.py) -- against an independent float64 numpy statement of the approximation, against the exact
model, for the integer invariants of its pyramid, and for the accuracy DESIGN.md 3.20 records.  Then the argument checks of the
three entries that need no device.  No GPU."""
import ctypes

import numpy as np
import pytest

import layout_binding as lb
import layout_pyramid_binding as pb
from expressionmatrix2_amd import capi

INVALID, UNSUPPORTED = 1, 6


@pytest.fixture(scope="module")
def restatement():
    return pb.load()


def _spread(n, seed):
    x, y = pb._cloud(n, seed)
    if n >= 4:
        x[3], y[3] = x[1], y[1]
        x[n - 1], y[n - 1] = x[0], y[0]
    return x, y


def _clustered(n, seed):
    """Eight Gaussian clusters of width 2 on the square of the start positions."""
    rng = np.random.default_rng(seed)
    centres = (rng.random((8, 2)) - 0.5) * np.sqrt(n)
    p = centres[rng.integers(0, 8, n)] + rng.normal(0., 2., (n, 2))
    return p[:, 0].astype(np.float32), p[:, 1].astype(np.float32)


@pytest.mark.parametrize("name,gravity,depth", [("random-65", 0., 2), ("random-257", 0.02, 3), ("random-2049", 0.5, 5),
                                                ("random-4100", 0.02, 6), ("random-257", 0., 10), ("star-600", 0.02, 4),
                                                ("loops-and-repeats", 0.02, 2), ("isolated", 0., 3), ("no-edges", 1., 3)])
def test_forces_against_the_float64_statement(restatement, name, gravity, depth):
    n, edges = lb.case(name)
    x, y = _spread(n, 17)
    out = restatement.forces(n, edges, gravity, x, y, depth)
    terms = pb.check_against_numpy(out, n, edges, gravity, x, y, depth, "%s at depth %d" % (name, depth))
    assert np.array_equal(terms, out[3])                     # the two statements visit the same cells and vertices
    assert out[2] == pytest.approx(float((np.stack(out[:2], axis=1).astype(np.float64) ** 2).sum()), rel=1e-12)


@pytest.mark.parametrize("name", pb.POSITION_SETS)
def test_position_sets_against_the_float64_statement(restatement, name):
    x, y, depth = pb.position_set(name)
    n, edges = len(x), pb.position_set_edges(len(x))
    out = restatement.forces(n, edges, 0.02, x, y, depth)
    terms = pb.check_against_numpy(out, n, edges, 0.02, x, y, depth, name)
    assert np.array_equal(terms, out[3])


def test_coincident_vertices_and_the_vertex_itself_add_an_exact_zero(restatement):
    x, y, depth = pb.position_set("all-coincident")
    fx, fy, energy, terms = restatement.forces(len(x), ([], []), 0., x, y, depth)
    assert not lb.bits(fx).any() and not lb.bits(fy).any() and energy == 0. and np.all(terms == len(x))


@pytest.mark.parametrize("name,gravity", [("random-65", 0.), ("random-257", 0.02), ("star-600", 0.02), ("loops-and-repeats", 0.02)])
def test_depth_0_is_the_exact_model(restatement, name, gravity):
    """One leaf is the whole near field: the forces are within DESIGN.md 3.19's bound of the exact float64 model."""
    n, edges = lb.case(name)
    x, y = _spread(n, 17)
    fx, fy, _, terms = restatement.forces(n, edges, gravity, x, y, 0)
    f, absolute = lb.numpy_forces(n, edges, gravity, x, y)
    assert np.all(terms == n)
    assert np.all(np.abs(np.stack([fx, fy], axis=1).astype(np.float64) - f) <= lb.force_bound(n, absolute))


@pytest.mark.parametrize("name", ["cloud-1000-depth-4", "cloud-300-depth-10", "one-dense-leaf", "all-coincident", "cell-boundaries",
                                  "at-xmax-and-ymax", "vertical-line"])
def test_integer_invariants_of_the_pyramid(restatement, name):
    if name.startswith("cloud"):
        x, y = _spread(int(name.split("-")[1]), 4)
        depth = int(name.split("-")[3])
    else:
        x, y, depth = pb.position_set(name)
    n = len(x)
    p = restatement.pyramid(x, y, depth)
    xmin, ymin, side = (float(v) for v in p["box"])
    assert xmin == x.min() and ymin == y.min() and side == max(np.float32(x.max() - x.min()), np.float32(y.max() - y.min()))
    assert p["qx"].max() <= 2 ** 31 and p["qy"].max() <= 2 ** 31
    for level in range(depth + 1):
        width = 2 ** level
        begin = pb.level_begin(level)
        count = p["count"][begin:begin + width * width].reshape(width, width).astype(np.int64)
        sums = [p[k][begin:begin + width * width].reshape(width, width) for k in ("sumX", "sumY")]
        assert count.sum() == n                                                           # every level holds every vertex
        assert int(sums[0].sum()) == int(p["qx"].astype(np.uint64).sum()) and int(sums[1].sum()) == int(p["qy"].astype(np.uint64).sum())
        if level < depth:                                                                 # a parent is its four children
            below = pb.level_begin(level + 1)
            for k, mine in (("count", count), ("sumX", sums[0]), ("sumY", sums[1])):
                children = p[k][below:below + 4 * width * width].reshape(width, 2, width, 2).astype(np.uint64)
                assert np.array_equal(children.sum(axis=(1, 3)), mine.astype(np.uint64))
        # the centroid of a cell that is not empty lies in the cell's quantised bounds: mean(q) in [b, b + 1) 2^(31 - l), the
        # last cell closed at 2^31; as a position, within the float32 rounding of the centroid
        by, bx = np.nonzero(count)
        for axis, q_sum, b, lo, m in ((0, sums[0], bx, xmin, p["mx"]), (1, sums[1], by, ymin, p["my"])):
            mean = q_sum[by, bx].astype(np.float64) / count[by, bx]
            cell = 2. ** (31 - level)
            assert np.all(mean >= b * cell) and np.all((mean < (b + 1) * cell) | ((b == width - 1) & (mean <= 2. ** 31)))
            position = m[begin:begin + width * width].reshape(width, width)[by, bx].astype(np.float64)
            slack = 2. ** -23 * np.maximum(np.abs(position), abs(lo))
            assert np.all(position >= lo + side * b / width - slack) and np.all(position <= lo + side * (b + 1) / width + slack)


@pytest.mark.parametrize("n,depth", [(1, 0), (8, 0), (9, 1), (32, 1), (33, 2), (8 * 4 ** 9, 9), (8 * 4 ** 9 + 1, 10), (8 * 4 ** 10 + 1, 10),
                                     (2 ** 30, 10)])
def test_the_automatic_depth(restatement, n, depth):
    """The smallest D with LEAF_TARGET 4^D >= N, capped at 10: the restatement, the statement in Python, and (where a run is
    small enough to make) a run at the automatic depth against a run at that depth forced."""
    assert pb.LEAF_TARGET == capi.LAYOUT_LEAF_TARGET == 8
    assert restatement.automatic_depth(n) == depth == pb.automatic_depth(n)
    if n <= 33:
        edges = lb.ring(n)[1]
        lb.assert_same_run(restatement.layout(n, edges, maxIterationCount=3), restatement.layout(n, edges, depth=depth, maxIterationCount=3),
                           "automatic depth at %d vertices" % n)
        other = restatement.layout(n, edges, depth=depth + 2, maxIterationCount=3)
        assert n < 9 or not np.array_equal(other[0], restatement.layout(n, edges, maxIterationCount=3)[0])


# ---- the accuracy of the approximation: measured against the exact restatement, recorded in DESIGN.md 3.20 ----
# (median relative error, 99th percentile, ratio of the energies) as measured; the assertions allow twice each (for the ratio:
# twice its distance from 1).
MEASURED = {
    "start positions": (1.749e-3, 1.878e-2, 1.00063),        # depth 5, 108.9 interactions per vertex of 4 096
    "clustered": (2.656e-3, 3.631e-2, 1.00190),              # depth 5, 325.6
}


@pytest.mark.parametrize("name", ["start positions", "clustered"])
def test_accuracy_against_the_exact_restatement(restatement, name):
    n = 4096
    x, y = lb.load().initial(n, 231) if name == "start positions" else _clustered(n, 12)
    depth = pb.automatic_depth(n)
    ex, ey, exact_energy = lb.load().forces(n, ([], []), 0., x, y)
    fx, fy, energy, terms = restatement.forces(n, ([], []), 0., x, y)
    exact = np.stack([ex, ey], axis=1).astype(np.float64)
    error = np.linalg.norm(np.stack([fx, fy], axis=1).astype(np.float64) - exact, axis=1) / np.linalg.norm(exact, axis=1)
    median, high, ratio = float(np.median(error)), float(np.percentile(error, 99)), energy / exact_energy
    print("%s, %d vertices, depth %d: %.1f interactions per vertex, median relative error %.3e, 99th percentile %.3e, energy ratio %.5f"
          % (name, n, depth, terms.mean(), median, high, ratio))
    measured = MEASURED[name]
    assert median <= 2. * measured[0] and high <= 2. * measured[1] and abs(ratio - 1.) <= 2. * abs(measured[2] - 1.)


# ---- the argument checks that answer before a device is looked for ----

def _raw(entry, *arguments):
    lib = capi.load()
    rc = getattr(lib, entry)(*[a.ctypes.data if isinstance(a, np.ndarray) else a for a in arguments])
    return rc, lib.em2_last_error().decode()


E0, E1 = np.array([0, 1], dtype=np.uint32), np.array([1, 2], dtype=np.uint32)
F32 = np.zeros(16, dtype=np.float32)
AUTO = pb.DEPTH_AUTO


def _layout_arguments(**changes):
    p = capi.LayoutParameters(**changes)
    return p, [4, E0, E1, 2, ctypes.byref(p), AUTO, F32, F32, None]


@pytest.mark.parametrize("entry", ["em2_graph_layout_pyramid", "em2_dev_graph_layout_pyramid"])
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
    for depth in (11, 12, 0xfffffffe, 0x80000000):
        arguments = list(good)
        arguments[5] = depth
        assert _raw(entry, *arguments) == (INVALID, entry + ": depth must be at most 10 or the automatic depth")
    arguments = list(good)
    arguments[0] = 2 ** 30 + 1
    assert _raw(entry, *arguments) == (UNSUPPORTED, entry + ": vertexCount is above 2^30")
    # no vertex: EM2_OK without the arrays, at every valid depth; with an edge, the edge is outside the graph
    result = capi.LayoutResult()
    for depth in (AUTO, 0, 10):
        assert _raw(entry, 0, None, None, 0, ctypes.byref(keep), depth, None, None, ctypes.byref(result))[0] == 0
        assert result.iterationCount == 0 and result.step == 1. and result.energy == np.inf
    assert _raw(entry, 0, E0, E1, 2, ctypes.byref(keep), AUTO, None, None, None) == (
        INVALID, entry + ": an edge names a vertex outside the graph")


def test_argument_checks_of_the_forces_entry():
    entry = "em2_graph_layout_forces_pyramid"
    energy = ctypes.c_double(5.)
    good = [4, E0, E1, 2, 0.5, AUTO, F32, F32, F32, F32, ctypes.byref(energy)]
    for position in (1, 2, 6, 7, 8, 9):
        arguments = list(good)
        arguments[position] = None
        assert _raw(entry, *arguments) == (INVALID, entry + ": null pointer")
    for gravity in (-1., float("nan")):
        arguments = list(good)
        arguments[4] = gravity
        assert _raw(entry, *arguments) == (INVALID, entry + ": gravity must not be negative")
    for depth in (11, 0xfffffffe):
        arguments = list(good)
        arguments[5] = depth
        assert _raw(entry, *arguments) == (INVALID, entry + ": depth must be at most 10 or the automatic depth")
    assert _raw(entry, 0, None, None, 0, 0.5, 3, None, None, None, None, ctypes.byref(energy))[0] == 0 and energy.value == 0.
    assert _raw(entry, 0, E0, E1, 2, 0.5, 3, None, None, None, None, None) == (INVALID, entry + ": an edge names a vertex outside the graph")


needs_no_device = pytest.mark.skipif(capi.device_count() > 0, reason="a HIP device is visible")


@needs_no_device
def test_no_device():
    text = ": no HIP device is visible (this library has no CPU path)"
    keep, good = _layout_arguments()
    for entry in ("em2_graph_layout_pyramid", "em2_dev_graph_layout_pyramid"):
        assert _raw(entry, *good) == (2, entry + text)
    assert _raw("em2_graph_layout_forces_pyramid", 4, E0, E1, 2, 0.5, 3, F32, F32, F32, F32, None) == (
        2, "em2_graph_layout_forces_pyramid" + text)


def test_the_facade_refuses_another_repulsion_before_anything_else():
    """(before the graph is looked up: the graph named here does not exist, and no store is open)"""
    from expressionmatrix2_amd import ExpressionMatrix
    with pytest.raises(ValueError) as error:
        ExpressionMatrix.computeCellGraphLayout(None, "Missing", repulsion="barnes-hut")
    assert '"exact"' in str(error.value) and '"pyramid"' in str(error.value)
