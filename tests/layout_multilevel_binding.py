"""ctypes binding of tests/native/em2_layout_multilevel_restatement.cpp (the multilevel layout of DESIGN.md 3.21 on one thread
in plain loops), an independent Python greedy matching, a float64 numpy statement of the weighted force, the graphs the
multilevel tests share and the stress of a layout.  Compiled with g++ at first use.  Test infrastructure only."""
import ctypes
import functools
import os
import subprocess

import numpy as np

import layout_binding as lb
import layout_pyramid_binding as lpb

SOURCE = os.path.join(lb.NATIVE_DIR, "em2_layout_multilevel_restatement.cpp")

# the constants of include/em2_lsh.h
DEPTH_AUTO = 0xffffffff
DEPTH_EXACT = 0xfffffffe
COARSEST = 32
MAX_LEVELS = 32
EXACT_LIMIT = 4096
NONE = 0xffffffff

c = ctypes
P = c.c_void_p
_ptr = lb._ptr


def _optional(a):
    return None if a is None else _ptr(a)


def _u32(a):
    return None if a is None else np.ascontiguousarray(a, dtype=np.uint32)


class MultilevelRestatement:
    def __init__(self, lib):
        self.lib = lib
        lib.em2rm_coarsen.argtypes = [c.c_uint32, P, P, P, P, c.c_uint64, c.c_uint32, c.c_uint32] + [P] * 7
        lib.em2rm_coarsen.restype = None
        lib.em2rm_forces_weighted.argtypes = [c.c_uint32, P, P, P, P, c.c_uint64, c.c_double, c.c_uint32] + [P] * 6
        lib.em2rm_forces_weighted.restype = None
        lib.em2rm_layout.argtypes = [c.c_uint32, P, P, c.c_uint64, c.c_uint32, c.c_uint32, c.c_double, c.c_double, c.c_double, c.c_uint32] + [P] * 8
        lib.em2rm_layout.restype = None

    def coarsen(self, n, edges, seed, level, mass=None, weights=None):
        """-> dict: mate, coarseOf [n], coarseCount, rounds, coarseMass [coarseCount], coarseEdges (a, b, w), each ascending."""
        v0, v1 = lb._edges(edges)
        mass, weights = _u32(mass), _u32(weights)
        mate, coarse_of, coarse_mass = (np.zeros(n, np.uint32) for _ in range(3))
        a, b, w = (np.zeros(len(v0), np.uint32) for _ in range(3))
        counts = np.zeros(3, np.uint64)
        self.lib.em2rm_coarsen(n, _optional(mass), _ptr(v0), _ptr(v1), _optional(weights), len(v0), seed, level, _ptr(mate), _ptr(coarse_of),
                               _ptr(coarse_mass), _ptr(a), _ptr(b), _ptr(w), _ptr(counts))
        count, edge_count = int(counts[0]), int(counts[2])
        return dict(mate=mate, coarseOf=coarse_of, coarseCount=count, rounds=int(counts[1]), coarseMass=coarse_mass[:count].copy(),
                    coarseEdges=(a[:edge_count].copy(), b[:edge_count].copy(), w[:edge_count].copy()))

    def forces_weighted(self, n, edges, gravity, x, y, depth, mass=None, weights=None):
        """-> (fx, fy, energy, terms)"""
        v0, v1 = lb._edges(edges)
        mass, weights = _u32(mass), _u32(weights)
        x, y = np.ascontiguousarray(x, dtype=np.float32), np.ascontiguousarray(y, dtype=np.float32)
        assert x.shape == y.shape == (n,)
        fx, fy = np.zeros(n, dtype=np.float32), np.zeros(n, dtype=np.float32)
        terms = np.zeros(n, dtype=np.uint32)
        energy = c.c_double(0.)
        self.lib.em2rm_forces_weighted(n, _optional(mass), _ptr(v0), _ptr(v1), _optional(weights), len(v0), gravity, depth, _ptr(x), _ptr(y),
                                       _ptr(fx), _ptr(fy), c.byref(energy), _ptr(terms))
        return fx, fy, energy.value, terms

    def layout(self, n, edges, depth=DEPTH_EXACT, **parameters):
        """-> (x, y, iterations, final step, final energy, levels); levels: a list of (vertexCount, edgeCount, matchingRounds,
        iterationCount), level 0 first.  parameters: the keys of layout_binding.DEFAULTS."""
        p = dict(lb.DEFAULTS)
        p.update(parameters)
        v0, v1 = lb._edges(edges)
        x, y = np.zeros(n, dtype=np.float32), np.zeros(n, dtype=np.float32)
        result = np.zeros(3, dtype=np.float64)
        count = c.c_uint32(0)
        vertices, rounds, iterations = (np.zeros(MAX_LEVELS, np.uint32) for _ in range(3))
        merged = np.zeros(MAX_LEVELS, np.uint64)
        self.lib.em2rm_layout(n, _ptr(v0), _ptr(v1), len(v0), p["seed"], p["maxIterationCount"], p["tolerance"], p["gravity"],
                              p["initialStep"], depth, _ptr(x), _ptr(y), _ptr(result), c.byref(count), _ptr(vertices), _ptr(merged),
                              _ptr(rounds), _ptr(iterations))
        levels = [(int(vertices[l]), int(merged[l]), int(rounds[l]), int(iterations[l])) for l in range(count.value)]
        return x, y, int(result[0]), float(result[1]), float(result[2]), levels


@functools.lru_cache(maxsize=None)
def load():
    build = os.path.join(lb.NATIVE_DIR, "build")
    os.makedirs(build, exist_ok=True)
    path = os.path.join(build, "libem2layoutmultilevelrestatement.so")
    if not os.path.exists(path) or os.path.getmtime(path) < os.path.getmtime(SOURCE):
        tmp = path + ".%d.tmp" % os.getpid()
        cmd = ["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-o", tmp, SOURCE]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError("layout multilevel restatement build failed: " + r.stderr)
        os.replace(tmp, path)
    return MultilevelRestatement(ctypes.CDLL(path))


@functools.lru_cache(maxsize=None)
def reference(name, iterations, depth):
    """The restatement's run of a named graph with the default parameters but `iterations` as maxIterationCount; computed once
    and shared (the arrays are read-only)."""
    n, edges = case(name)
    out = load().layout(n, edges, depth=depth, maxIterationCount=iterations)
    out[0].setflags(write=False)
    out[1].setflags(write=False)
    return out


def assert_same_multilevel_run(mine, theirs, what):
    """(x, y, iterations, step, energy, levels) twice: everything exactly."""
    assert mine[5] == theirs[5], "%s: levels %r, not %r" % (what, mine[5], theirs[5])
    lb.assert_same_run(mine[:5], theirs[:5], what)


# ---- the matching, stated independently: Python integers, the edges sorted by their key, taken greedily ----

_M = 2 ** 64 - 1


def mix(z):
    """The finaliser of splitmix64 after its increment, as include/em2_lsh.h writes it out."""
    z = (z + 0x9E3779B97F4A7C15) & _M
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M
    return z ^ (z >> 31)


def level_hash(seed, level, what):
    return mix(mix(seed << 32 | level) ^ what)


def merged_edges(edges, weights=None):
    """{(a, b): weight} with a < b: self-loops dropped, repeats added."""
    merged = {}
    w = np.ones(len(edges[0]), np.int64) if weights is None else weights
    for a, b, weight in zip(np.asarray(edges[0]).tolist(), np.asarray(edges[1]).tolist(), np.asarray(w).tolist()):
        if a != b:
            key = (min(a, b), max(a, b))
            merged[key] = merged.get(key, 0) + weight
    return merged


def python_greedy(n, merged, seed, level):
    """mate [n] (NONE where unmatched) of the greedy maximal matching over `merged` in descending (weight, hash, a, b)."""
    order = sorted(merged, key=lambda e: (merged[e], level_hash(seed, level, e[0] << 32 | e[1]), e[0], e[1]), reverse=True)
    mate = [NONE] * n
    for a, b in order:
        if mate[a] == NONE and mate[b] == NONE:
            mate[a], mate[b] = b, a
    return np.array(mate, dtype=np.uint32)


def python_rounds(n, merged, seed, level):
    """(mate, rounds) by the rounds of locally dominant edges, as the device runs them: every unmatched vertex points along its
    best live edge, two vertices that point at each other are matched, until no live edge is left."""
    key = {e: (w, level_hash(seed, level, e[0] << 32 | e[1]), e[0], e[1]) for e, w in merged.items()}
    incident = [[] for _ in range(n)]
    for (a, b) in merged:
        incident[a].append((key[(a, b)], b))
        incident[b].append((key[(a, b)], a))
    mate = [NONE] * n
    rounds = 0
    while True:
        pointer = [NONE] * n
        for v in range(n):
            if mate[v] == NONE:
                live = [entry for entry in incident[v] if mate[entry[1]] == NONE]
                if live:
                    pointer[v] = max(live)[1]
        if all(p == NONE for p in pointer):
            return np.array(mate, dtype=np.uint32), rounds
        for v in range(n):
            if pointer[v] != NONE and pointer[pointer[v]] == v:
                mate[v] = pointer[v]
        rounds += 1


def check_contraction(n, edges, out, mass=None, weights=None):
    """The invariants of one coarsening step `out` (a dict as coarsen() returns it) of the graph."""
    mass = np.ones(n, np.int64) if mass is None else np.asarray(mass, np.int64)
    mate, coarse_of = out["mate"].astype(np.int64), out["coarseOf"].astype(np.int64)
    matched = mate != NONE
    v = np.arange(n)
    assert np.all(mate[mate[matched]] == v[matched]) and np.all(mate[matched] != v[matched])
    representative = np.where(matched, np.minimum(v, np.where(matched, mate, v)), v)
    # ids ascend with the representative, without a gap
    is_representative = representative == v
    assert out["coarseCount"] == int(is_representative.sum())
    assert np.array_equal(coarse_of[is_representative], np.arange(out["coarseCount"]))
    assert np.array_equal(coarse_of, coarse_of[representative])
    # the masses of the groups, and their sum
    assert np.array_equal(out["coarseMass"].astype(np.int64), np.bincount(coarse_of, weights=mass, minlength=out["coarseCount"]).astype(np.int64))
    assert int(out["coarseMass"].sum()) == int(mass.sum())
    # the weights: what is not a loop and not inside a group
    merged = merged_edges(edges, weights)
    kept = sum(w for (a, b), w in merged.items() if coarse_of[a] != coarse_of[b])
    a, b, w = out["coarseEdges"]
    assert int(w.astype(np.int64).sum()) == kept
    assert np.all(a < b) and np.all(b < out["coarseCount"])
    keys = a.astype(np.int64) << 32 | b.astype(np.int64)
    assert np.all(np.diff(keys) > 0)
    expected = merged_edges((coarse_of[[e[0] for e in merged]], coarse_of[[e[1] for e in merged]]), list(merged.values())) if merged else {}
    assert expected == {(int(p), int(q)): int(r) for p, q, r in zip(a, b, w)}


# ---- the weighted force in float64 numpy ----

def numpy_weighted_forces(n, edges, gravity, x, y, depth, mass, weights):
    """The weighted force of include/em2_lsh.h in float64, vectorised -> (f, absolute, terms, slack) as
    layout_pyramid_binding.numpy_pyramid_forces gives them (slack 0 for the exact repulsion, depth DEPTH_EXACT)."""
    p = np.stack([np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)], axis=1)
    m = np.asarray(mass, dtype=np.float64)
    f, absolute, slack = np.zeros((n, 2)), np.zeros((n, 2)), np.zeros((n, 2))
    terms = np.zeros(n, dtype=np.int64)
    if depth == DEPTH_EXACT:
        near_all = True
    else:
        near_all = False
        qx, qy, xmin, ymin, side = lpb.numpy_cells(x, y, depth)
        for level in range(2, depth + 1):
            width = 2 ** level
            ax, ay = np.minimum(width - 1, qx >> (31 - level)), np.minimum(width - 1, qy >> (31 - level))
            cell = ay * width + ax
            count = np.bincount(cell, weights=m, minlength=width * width)
            with np.errstate(invalid="ignore"):
                centroid = np.stack([np.bincount(cell, weights=m * p[:, k], minlength=width * width) / count for k in (0, 1)], axis=1)
            delta = lpb.centroid_slack(float(side), centroid)
            for oy in range(6):
                for ox in range(6):
                    bx, by = 2 * ((ax >> 1) - 1) + ox, 2 * ((ay >> 1) - 1) + oy
                    keep = (bx >= 0) & (by >= 0) & (bx < width) & (by < width) & (np.maximum(np.abs(bx - ax), np.abs(by - ay)) > 1)
                    other = np.where(keep, by * width + bx, 0)
                    keep &= count[other] > 0
                    d = p[keep] - centroid[other[keep]]
                    w = lb.C * count[other[keep]] / np.maximum((d ** 2).sum(axis=1), lb.FLOOR)
                    f[keep] += d * w[:, None]
                    absolute[keep] += np.abs(d * w[:, None])
                    slack[keep] += (w * delta[other[keep]])[:, None]
                    terms[keep] += 1
        width = 2 ** depth
        ax, ay = np.minimum(width - 1, qx >> (31 - depth)), np.minimum(width - 1, qy >> (31 - depth))
    for begin in range(0, n, 512):
        rows = slice(begin, begin + 512)
        d = p[rows, None, :] - p[None, :, :]
        w = lb.C * m[None, :] / np.maximum((d ** 2).sum(axis=2), lb.FLOOR)
        if not near_all:
            near = (np.abs(ax[rows, None] - ax[None, :]) <= 1) & (np.abs(ay[rows, None] - ay[None, :]) <= 1)
            w = np.where(near, w, 0.)
            terms[rows] += near.sum(axis=1)
        else:
            terms[rows] += n
        f[rows] += (d * w[:, :, None]).sum(axis=1)
        absolute[rows] += np.abs(d * w[:, :, None]).sum(axis=1)
    v0, v1 = (np.asarray(e, dtype=np.int64) for e in edges)
    wt = np.asarray(weights, dtype=np.float64)
    for a, b in ((v0, v1), (v1, v0)):
        d = p[a] - p[b]
        t = -d * (wt * np.sqrt((d ** 2).sum(axis=1)) / m[a])[:, None]
        np.add.at(f, a, t)
        np.add.at(absolute, a, np.abs(t))
    f -= gravity * p
    absolute += np.abs(gravity * p)
    return f, absolute, terms, slack


def check_weighted_against_numpy(forces, n, edges, gravity, x, y, depth, mass, weights, what):
    """Every component within (T + 8) 2^-24 sum|terms| of the numpy statement (DESIGN.md 3.19's bound, T the addends of the
    vertex's repulsion sums), plus the centroid slack of layout_pyramid_binding where a pyramid is used."""
    f, absolute, terms, slack = numpy_weighted_forces(n, edges, gravity, x, y, depth, mass, weights)
    bound = lpb.pyramid_force_bound(terms, absolute, slack)
    error = np.abs(np.stack([forces[0], forces[1]], axis=1).astype(np.float64) - f)
    worst = float((error / np.maximum(bound, 1e-300)).max())
    print("%s: worst error / bound %.4f, terms %d ... %d" % (what, worst, terms.min(), terms.max()))
    assert np.all(error <= bound), what


def position_set_weights(n):
    """Masses 1 ... 7 and, for layout_pyramid_binding.position_set_edges(n), weights 1 ... 3."""
    edges = lpb.position_set_edges(n)
    return (np.arange(n, dtype=np.uint32) * 5 + 2) % 7 + 1, (np.arange(len(edges[0]), dtype=np.uint32) * 2 + 1) % 3 + 1


# ---- graphs ----

def grid(side):
    """The side x side grid graph, vertex y * side + x."""
    pairs = [(y * side + x, y * side + x + 1) for y in range(side) for x in range(side - 1)]
    pairs += [(y * side + x, (y + 1) * side + x) for y in range(side - 1) for x in range(side)]
    return lb._graph(side * side, pairs)


def ascending_path(n=40):
    """A path of n vertices whose edge i is there i + 1 times: the weights ascend strictly, so a round of locally dominant edges
    matches only the last live edge."""
    return lb._graph(n, [(i, i + 1) for i in range(n - 1) for _ in range(i + 1)])


@functools.lru_cache(maxsize=None)
def case(name):
    if name == "one-vertex":
        return lb._graph(1, [])
    if name == "one-edge":
        return lb._graph(2, [(0, 1)])
    if name == "path-3":
        return lb._graph(3, [(0, 1), (1, 2)])
    if name == "ascending-path-40":
        return ascending_path()
    if name == "grid-48":
        return grid(48)
    if name == "ring-2000":
        return lb.ring(2000)
    if name.startswith("sparse-"):                           # random, degree 6: n = 256 and 257, the workgroup's edge
        n = int(name.split("-")[1])
        return lb.random_graph(n, 6, 7 + n)
    return lb.case(name)


COARSEN_CASES = ["one-vertex", "one-edge", "path-3", "star-600", "ring-70", "cliques", "no-edges", "loops-and-repeats", "random-257",
                 "random-2049", "ascending-path-40", "sparse-256", "sparse-257"]
ONE_LEVEL_CASES = ["star-600", "no-edges", "cliques", "random-1"]


# ---- the quality of a layout ----

STRESS_PAIRS = 20000
STRESS_SEED = 20


def _sample(n):
    rng = np.random.default_rng(STRESS_SEED)
    i, j = rng.integers(0, n, STRESS_PAIRS), rng.integers(0, n, STRESS_PAIRS)
    keep = i != j
    return i[keep], j[keep]


def stress(x, y, graph_distance):
    """min over s of mean((s |p_i - p_j| - g_ij)^2 / g_ij^2) over a fixed sample of pairs; graph_distance(i, j) -> g.  With
    a = |p_i - p_j| / g the minimum is at s = sum(a) / sum(a^2)."""
    i, j = _sample(len(x))
    g = graph_distance(i, j).astype(np.float64)
    d = np.hypot(np.asarray(x, np.float64)[i] - np.asarray(x, np.float64)[j], np.asarray(y, np.float64)[i] - np.asarray(y, np.float64)[j])
    a = d / g
    s = a.sum() / (a * a).sum()
    return float(np.mean((s * a - 1.) ** 2))


def grid_distance(side):
    return lambda i, j: np.abs(i % side - j % side) + np.abs(i // side - j // side)


def ring_distance(n):
    return lambda i, j: np.minimum(np.abs(i - j), n - np.abs(i - j))


# The stress of the 48 x 48 grid with the default parameters, measured with the two restatements on a CPU (one run each; the
# results are functions of the input alone): single level / multilevel at EM2_LAYOUT_DEPTH_EXACT, and their geometric mean,
# below which the multilevel layout has to stay.
GRID_STRESS_SINGLE = 0.27015                                # 220 iterations
GRID_STRESS_MULTI = 0.016152                                # 9 levels, 1 484 iterations over all of them
GRID_STRESS_THRESHOLD = (GRID_STRESS_SINGLE * GRID_STRESS_MULTI) ** 0.5      # 0.06606: a factor 4.09 from either
