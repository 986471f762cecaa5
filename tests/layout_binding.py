"""ctypes binding of tests/native/em2_layout_restatement.cpp (the spring-electrical layout of DESIGN.md 3.19 on one thread, in
plain loops), an independent float64 numpy statement of the model's forces, and the graphs the layout tests share.  Compiled
with g++ at first use.  Test infrastructure only."""
import ctypes
import functools
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE_DIR = os.path.join(ROOT, "tests", "native")
SOURCE = os.path.join(NATIVE_DIR, "em2_layout_restatement.cpp")

# the constants of the model (Hu 2005) and the defaults of include/em2_lsh.h
C = 0.2
K = 1.0
FLOOR = 1e-30
T = 0.9
DEFAULTS = dict(seed=231, maxIterationCount=300, tolerance=0.01, gravity=0.02, initialStep=1.0)
# the shapes of csrc/em2_layout.hip
SLICE_COUNT = 16
TILE = 128
BLOCK_VERTICES = 256

c = ctypes
P = c.c_void_p


def _ptr(a):
    return a.ctypes.data_as(c.c_void_p)


def _edges(edges):
    v0 = np.ascontiguousarray(edges[0], dtype=np.uint32)
    v1 = np.ascontiguousarray(edges[1], dtype=np.uint32)
    assert v0.shape == v1.shape and v0.ndim == 1
    return v0, v1


class LayoutRestatement:
    def __init__(self, lib):
        self.lib = lib
        lib.em2r_layout_initial.argtypes = [c.c_uint32, c.c_uint32, P, P]
        lib.em2r_layout_initial.restype = None
        lib.em2r_layout_forces.argtypes = [c.c_uint32, P, P, c.c_uint64, c.c_double, P, P, P, P, P]
        lib.em2r_layout_forces.restype = None
        lib.em2r_layout.argtypes = [c.c_uint32, P, P, c.c_uint64, c.c_uint32, c.c_uint32, c.c_double, c.c_double, c.c_double, P, P, P]
        lib.em2r_layout.restype = None

    def initial(self, n, seed):
        x, y = np.zeros(n, dtype=np.float32), np.zeros(n, dtype=np.float32)
        self.lib.em2r_layout_initial(n, seed, _ptr(x), _ptr(y))
        return x, y

    def forces(self, n, edges, gravity, x, y):
        """-> (fx, fy, energy)"""
        v0, v1 = _edges(edges)
        x, y = np.ascontiguousarray(x, dtype=np.float32), np.ascontiguousarray(y, dtype=np.float32)
        assert x.shape == y.shape == (n,)
        fx, fy = np.zeros(n, dtype=np.float32), np.zeros(n, dtype=np.float32)
        energy = c.c_double(0.)
        self.lib.em2r_layout_forces(n, _ptr(v0), _ptr(v1), len(v0), gravity, _ptr(x), _ptr(y), _ptr(fx), _ptr(fy), c.byref(energy))
        return fx, fy, energy.value

    def layout(self, n, edges, **parameters):
        """-> (x, y, iterations, final step, final energy); parameters: the keys of DEFAULTS."""
        p = dict(DEFAULTS)
        p.update(parameters)
        v0, v1 = _edges(edges)
        x, y = np.zeros(n, dtype=np.float32), np.zeros(n, dtype=np.float32)
        result = np.zeros(3, dtype=np.float64)
        self.lib.em2r_layout(n, _ptr(v0), _ptr(v1), len(v0), p["seed"], p["maxIterationCount"], p["tolerance"], p["gravity"],
                             p["initialStep"], _ptr(x), _ptr(y), _ptr(result))
        return x, y, int(result[0]), float(result[1]), float(result[2])


@functools.lru_cache(maxsize=None)
def load():
    build = os.path.join(NATIVE_DIR, "build")
    os.makedirs(build, exist_ok=True)
    path = os.path.join(build, "libem2layoutrestatement.so")
    if not os.path.exists(path) or os.path.getmtime(path) < os.path.getmtime(SOURCE):
        tmp = path + ".%d.tmp" % os.getpid()
        cmd = ["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-o", tmp, SOURCE]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError("layout restatement build failed: " + r.stderr)
        os.replace(tmp, path)
    return LayoutRestatement(ctypes.CDLL(path))


def bits(a):
    """A float32 array as uint32: NaN compares equal to itself, -0.0 differs from 0.0."""
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def assert_same_run(mine, theirs, what):
    """(x, y, iterations, step, energy) twice: the positions bit for bit, the three scalars exactly."""
    assert mine[2] == theirs[2], "%s: %d iterations, not %d" % (what, mine[2], theirs[2])
    assert np.float64(mine[3]).tobytes() == np.float64(theirs[3]).tobytes(), "%s: final step %r, not %r" % (what, mine[3], theirs[3])
    assert np.float64(mine[4]).tobytes() == np.float64(theirs[4]).tobytes(), "%s: final energy %r, not %r" % (what, mine[4], theirs[4])
    for axis, a, b in (("x", mine[0], theirs[0]), ("y", mine[1], theirs[1])):
        assert a.shape == b.shape and a.dtype == b.dtype == np.float32, "%s: %s has another size" % (what, axis)
        different = np.flatnonzero(bits(a) != bits(b))
        assert len(different) == 0, "%s: %s differs at %d vertices, first %d: %r != %r" % (
            what, axis, len(different), different[0], a[different[0]], b[different[0]])


# ---- the independent statement: float64, numpy, straight from the formulas of the model ----

def numpy_forces(n, edges, gravity, x, y):
    """-> (f [n, 2] float64, absolute [n, 2] float64: the sum of the absolute values of each component's addends).  The
    positions are taken as given (float32 values in float64); nothing here follows the summation shapes of the kernel."""
    p = np.stack([np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)], axis=1)
    f = np.zeros((n, 2))
    absolute = np.zeros((n, 2))
    for begin in range(0, n, 512):                                           # rows in blocks: [512, n, 2] at a time
        delta = p[begin:begin + 512, None, :] - p[None, :, :]
        d2 = np.maximum((delta ** 2).sum(axis=2), FLOOR)
        terms = delta * (C * K * K / d2)[:, :, None]
        f[begin:begin + 512] += terms.sum(axis=1)
        absolute[begin:begin + 512] += np.abs(terms).sum(axis=1)
    v0, v1 = (np.asarray(e, dtype=np.int64) for e in edges)
    for a, b in ((v0, v1), (v1, v0)):                                          # both directions of every edge
        delta = p[a] - p[b]
        terms = -delta * (np.sqrt((delta ** 2).sum(axis=1)) / K)[:, None]
        np.add.at(f, a, terms)
        np.add.at(absolute, a, np.abs(terms))
    f -= gravity * p
    absolute += np.abs(gravity * p)
    return f, absolute


def force_bound(n, absolute):
    """The rounding bound of an n-term float32 sum whose addends are themselves rounded a few times: (n + 8) 2^-24 sum |terms|."""
    return (n + 8) * 2.0 ** -24 * absolute


# ---- graphs ----
# A graph is (n, (v0, v1)) with uint32 arrays.

def _graph(n, pairs):
    pairs = np.asarray(pairs, dtype=np.uint32).reshape(-1, 2)
    v0, v1 = pairs[:, 0].copy(), pairs[:, 1].copy()
    v0.setflags(write=False)
    v1.setflags(write=False)
    return n, (v0, v1)


def random_graph(n, degree, seed):
    """About degree * n / 2 random edges; repeated edges and self-loops are possible."""
    rng = np.random.default_rng(seed)
    count = degree * n // 2 if n > 1 else 0
    return _graph(n, rng.integers(0, n, size=(count, 2)))


def ring(n):
    return _graph(n, [(i, (i + 1) % n) for i in range(n)])


def star(leaves):
    return _graph(leaves + 1, [(0, i) for i in range(1, leaves + 1)])


def cliques(size=8):
    """Two cliques of `size` vertices joined by one edge (0, size)."""
    pairs = [(a + o, b + o) for o in (0, size) for a in range(size) for b in range(a + 1, size)]
    return _graph(2 * size, pairs + [(0, size)])


def with_isolated(n=70):
    """A path over the first half of the vertices; the others have no edge."""
    return _graph(n, [(i, i + 1) for i in range(n // 2 - 1)])


def loops_and_repeats():
    """A self-loop at 0 and at 5, the edge (1, 2) three times (once reversed), the rest a path."""
    return _graph(9, [(0, 0), (0, 1), (1, 2), (2, 1), (1, 2), (2, 3), (3, 4), (4, 5), (5, 5), (5, 6), (6, 7), (7, 8)])


# N: 1, 2, the wave edge, the workgroup's vertex count (256) and the 16 slices * the tile of 128 (slice length 127, 128, 129),
# and 4100: slices of 257 = two whole tiles and a ragged one.
SIZES = (1, 2, 63, 64, 65, BLOCK_VERTICES - 1, BLOCK_VERTICES, BLOCK_VERTICES + 1,
         SLICE_COUNT * TILE - SLICE_COUNT, SLICE_COUNT * TILE, SLICE_COUNT * TILE + 1, 4100)


@functools.lru_cache(maxsize=None)
def case(name):
    """A named graph; built once, never modified."""
    if name.startswith("random-"):
        n = int(name.split("-")[1])
        return random_graph(n, 6, 100 + n)
    return {
        "no-edges": lambda: _graph(300, []),
        "star-600": lambda: star(600),
        "ring-70": lambda: ring(70),
        "isolated": with_isolated,
        "loops-and-repeats": loops_and_repeats,
        "cliques": cliques,
    }[name]()


CASES = ["random-%d" % n for n in SIZES] + ["no-edges", "star-600", "ring-70", "isolated", "loops-and-repeats", "cliques"]


@functools.lru_cache(maxsize=None)
def reference(name, iterations):
    """The restatement's run of a named case with the default parameters but `iterations` as maxIterationCount; computed once
    and shared (the arrays are read-only)."""
    n, edges = case(name)
    out = load().layout(n, edges, maxIterationCount=iterations)
    out[0].setflags(write=False)
    out[1].setflags(write=False)
    return out
