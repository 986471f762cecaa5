"""tests/native/em2_layout_restatement.cpp -- what csrc/em2_layout.hip must equal bit for bit (tests/test_gpu_layout.py) --
against an independent float64 numpy statement of the model, against closed forms, and for the properties and the determinism
DESIGN.md 3.19 states.  No GPU."""
import numpy as np
import pytest

import layout_binding as lb

EQUILIBRIUM = lb.C ** (1. / 3.) * lb.K                     # C K^2 / d = d^2 / K


@pytest.fixture(scope="module")
def restatement():
    return lb.load()


def _spread(n, seed, coincident=False):
    rng = np.random.default_rng(seed)
    x = (rng.random(n, dtype=np.float32) - np.float32(0.5)) * np.float32(np.sqrt(n))
    y = (rng.random(n, dtype=np.float32) - np.float32(0.5)) * np.float32(np.sqrt(n))
    if coincident and n >= 4:
        x[3], y[3] = x[1], y[1]
        x[n - 1], y[n - 1] = x[0], y[0]
    return x, y


@pytest.mark.parametrize("name,gravity", [("random-65", 0.), ("random-257", 0.02), ("random-2049", 0.5), ("star-600", 0.02),
                                          ("loops-and-repeats", 0.02), ("isolated", 0.), ("no-edges", 1.)])
def test_forces_against_the_float64_statement(restatement, name, gravity):
    """Every force component within (N + 8) 2^-24 sum|terms|: the rounding bound of an N-term float32 sum (N - 1 additions of
    relative error 2^-24 each, whatever their order) with room for the few roundings inside a term (the differences, d^2, the
    division, the fmaf: 8 more units).  sum|terms| is the float64 sum of the absolute values of that component's addends."""
    n, edges = lb.case(name)
    x, y = _spread(n, 17, coincident=True)
    fx, fy, energy = restatement.forces(n, edges, gravity, x, y)
    f, absolute = lb.numpy_forces(n, edges, gravity, x, y)
    bound = lb.force_bound(n, absolute)
    error = np.abs(np.stack([fx, fy], axis=1).astype(np.float64) - f)
    worst = float((error / np.maximum(bound, 1e-300)).max())
    print("%s: worst error / bound %.4f" % (name, worst))
    assert np.all(error <= bound)
    assert energy == pytest.approx(float((np.stack([fx, fy], axis=1).astype(np.float64) ** 2).sum()), rel=1e-12)


def test_coincident_vertices_and_the_vertex_itself_add_an_exact_zero(restatement):
    x = np.array([1.5, 1.5, 1.5], dtype=np.float32)
    y = np.array([-2., -2., -2.], dtype=np.float32)
    fx, fy, energy = restatement.forces(3, ([0], [0]), 0., x, y)       # a self-loop too
    assert lb.bits(fx).tolist() == [0, 0, 0] and lb.bits(fy).tolist() == [0, 0, 0] and energy == 0.
    # ... and a run from there moves nothing (|f| = 0)
    fx, fy, _ = restatement.forces(1, ([], []), 0.02, x[:1], y[:1])
    assert fx[0] == np.float32(-0.02) * np.float32(1.5) and fy[0] == np.float32(0.02) * np.float32(2.)


def _final_step_bound(step):
    """The run ended because the step fell below the tolerance, so its last update was a shrink: the energy of the last
    evaluation did not fall.  For the pair every move changes the distance d by exactly 2 s (both ends move by s along the
    line), and |f| is monotone in d on either side of the equilibrium d*: a move that does not cross d* lowers the energy.  So
    the last but one move, of step s' >= s_K, crossed d*, which leaves |d - d*| < 2 s', and the last move, of step s_K = final
    step / t, changed d by 2 s_K towards or across d* without lowering |f|: |d - d*| <= 2 s_K after it.  (The issue's estimate
    was 4 tolerance K; 2 / t = 2.23 is what the step rule gives, and the restatement stays below half of it.)  A triangle that
    has become equilateral moves radially, its sides change by sqrt(3) s per move, and the same argument gives sqrt(3) s_K."""
    return 2. * step / lb.T


@pytest.mark.parametrize("tolerance", [0.1, 0.01, 0.001])
@pytest.mark.parametrize("seed", [0, 1, 231])
def test_closed_forms_without_gravity(restatement, seed, tolerance):
    for n, edges in ((2, ([0], [1])), (3, ([0, 1, 2], [1, 2, 0]))):
        x, y, iterations, step, _ = restatement.layout(n, edges, seed=seed, gravity=0., tolerance=tolerance, maxIterationCount=10000)
        assert iterations < 10000 and step < tolerance * lb.K and step / lb.T >= tolerance * lb.K
        x, y = x.astype(np.float64), y.astype(np.float64)
        for a, b in zip(*edges):
            d = float(np.hypot(x[a] - x[b], y[a] - y[b]))
            print("n %d seed %d tolerance %g: |d - d*| = %.3g, bound %.3g" % (n, seed, tolerance, abs(d - EQUILIBRIUM), _final_step_bound(step)))
            assert abs(d - EQUILIBRIUM) <= _final_step_bound(step) + 1e-6
            assert abs(d - EQUILIBRIUM) < 4. * tolerance * lb.K


@pytest.mark.parametrize("name", ["ring-70", "cliques", "random-257", "star-600"])
def test_the_energy_falls(restatement, name):
    n, edges = lb.case(name)
    _, _, initial = restatement.forces(n, edges, lb.DEFAULTS["gravity"], *restatement.initial(n, lb.DEFAULTS["seed"]))
    _, _, iterations, _, energy = lb.reference(name, lb.DEFAULTS["maxIterationCount"])
    assert iterations > 0 and energy < initial


def test_two_cliques_are_two_groups(restatement):
    n, edges = lb.case("cliques")
    x, y, _, _, _ = lb.reference("cliques", lb.DEFAULTS["maxIterationCount"])
    p = np.stack([x, y], axis=1).astype(np.float64)
    inside = [np.linalg.norm(p[a] - p[b]) for o in (0, 8) for a in range(o, o + 8) for b in range(a + 1, o + 8)]
    between = np.linalg.norm(p[:8].mean(axis=0) - p[8:].mean(axis=0))
    assert np.mean(inside) < between


def test_isolated_vertices_without_gravity_stay_finite(restatement):
    n, edges = lb.case("isolated")
    x, y, iterations, step, energy = restatement.layout(n, edges, gravity=0.)
    assert iterations > 0 and np.all(np.isfinite(x)) and np.all(np.isfinite(y)) and np.isfinite(step) and np.isfinite(energy)


def test_no_iteration_returns_the_initial_positions(restatement):
    n, edges = lb.case("ring-70")
    x, y, iterations, step, energy = restatement.layout(n, edges, maxIterationCount=0)
    x0, y0 = restatement.initial(n, lb.DEFAULTS["seed"])
    assert iterations == 0 and step == lb.DEFAULTS["initialStep"] and energy == np.inf
    assert np.array_equal(lb.bits(x), lb.bits(x0)) and np.array_equal(lb.bits(y), lb.bits(y0))
    # an initial step below the tolerance: nothing runs either
    assert restatement.layout(n, edges, initialStep=0.001)[2] == 0


def test_determinism(restatement):
    n, edges = lb.case("random-257")
    first = restatement.layout(n, edges, seed=5, maxIterationCount=40)
    second = restatement.layout(n, edges, seed=5, maxIterationCount=40)
    lb.assert_same_run(first, second, "the same seed")
    other = restatement.layout(n, edges, seed=6, maxIterationCount=40)
    assert not np.array_equal(first[0], other[0]) and not np.array_equal(first[1], other[1])


def test_initial_positions(restatement):
    """A pure function of (seed, vertex): u in [-0.5, 0.5) on a grid of 2^-24 from the hash, times sqrtf(N) K.  Between two
    vertex counts the positions of a vertex differ by that factor only."""
    x64, y64 = restatement.initial(64, 231)                      # side 8: x = 8 u exactly
    ux, uy = x64 / np.float32(8.), y64 / np.float32(8.)
    u = np.concatenate([ux, uy]).astype(np.float64)
    assert np.all(u >= -0.5) and np.all(u < 0.5) and np.all(u * 2 ** 24 == np.round(u * 2 ** 24))
    for n in (1, 4, 7, 100, 4100):
        x, y = restatement.initial(n, 231)
        side = np.sqrt(np.float32(n))
        assert np.array_equal(x[:64], ux[:n] * side) and np.array_equal(y[:64], uy[:n] * side)
    x100, _ = restatement.initial(100, 231)
    big_x, big_y = restatement.initial(100000, 231)
    side = float(np.sqrt(np.float32(100000.)))
    assert abs(big_x.mean()) < 0.01 * side and abs(big_y.mean()) < 0.01 * side             # centred: the mean of 10^5 uniforms
    assert big_x.min() < -0.49 * side and big_x.max() > 0.49 * side
    assert abs(np.corrcoef(big_x, big_y)[0, 1]) < 0.02
    other_x, _ = restatement.initial(100, 232)
    assert not np.array_equal(other_x, x100)
