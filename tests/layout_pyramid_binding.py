"""ctypes binding of tests/native/em2_layout_pyramid_restatement.cpp (the layout with the pyramid's far field, DESIGN.md 3.20,
on one thread in plain loops), an independent float64 numpy statement of the approximation, and the position sets the pyramid
tests share.  Compiled with g++ at first use.  Test infrastructure only."""
import ctypes
import functools
import os
import subprocess

import numpy as np

import layout_binding as lb

SOURCE = os.path.join(lb.NATIVE_DIR, "em2_layout_pyramid_restatement.cpp")

# the constants of include/em2_lsh.h
DEPTH_AUTO = 0xffffffff
MAX_DEPTH = 10
LEAF_TARGET = 8

c = ctypes
P = c.c_void_p
_ptr = lb._ptr


def level_begin(level):
    """Where level l begins in an array over the cells of all levels; level l is row-major, cell (bx, by) at by * 2^l + bx."""
    return (4 ** level - 1) // 3


def automatic_depth(n):
    """The smallest D in 0 ... 10 with LEAF_TARGET * 4^D >= n, else 10 (stated on its own, not through the library)."""
    for depth in range(MAX_DEPTH):
        if LEAF_TARGET * 4 ** depth >= n:
            return depth
    return MAX_DEPTH


class PyramidRestatement:
    def __init__(self, lib):
        self.lib = lib
        lib.em2rp_automatic_depth.argtypes = [c.c_uint32]
        lib.em2rp_automatic_depth.restype = c.c_uint32
        lib.em2rp_pyramid.argtypes = [c.c_uint32, c.c_uint32] + [P] * 10
        lib.em2rp_pyramid.restype = None
        lib.em2rp_layout_forces.argtypes = [c.c_uint32, P, P, c.c_uint64, c.c_double, c.c_uint32, P, P, P, P, P, P]
        lib.em2rp_layout_forces.restype = None
        lib.em2rp_layout.argtypes = [c.c_uint32, P, P, c.c_uint64, c.c_uint32, c.c_uint32, c.c_double, c.c_double, c.c_double, c.c_uint32,
                                     P, P, P]
        lib.em2rp_layout.restype = None

    def automatic_depth(self, n):
        return int(self.lib.em2rp_automatic_depth(n))

    def pyramid(self, x, y, depth):
        """-> dict: box (xmin, ymin, S), qx, qy [n], count, sumX, sumY, mx, my over the cells of all levels (level_begin)."""
        x, y = np.ascontiguousarray(x, dtype=np.float32), np.ascontiguousarray(y, dtype=np.float32)
        n, cells = len(x), level_begin(depth + 1)
        out = dict(box=np.zeros(3, np.float32), qx=np.zeros(n, np.uint32), qy=np.zeros(n, np.uint32), count=np.zeros(cells, np.uint32),
                   sumX=np.zeros(cells, np.uint64), sumY=np.zeros(cells, np.uint64), mx=np.zeros(cells, np.float32),
                   my=np.zeros(cells, np.float32))
        self.lib.em2rp_pyramid(n, depth, _ptr(x), _ptr(y), *[_ptr(out[k]) for k in ("box", "qx", "qy", "count", "sumX", "sumY", "mx", "my")])
        return out

    def forces(self, n, edges, gravity, x, y, depth=DEPTH_AUTO):
        """-> (fx, fy, energy, terms): terms [n] = the addends of each vertex's two repulsion sums."""
        v0, v1 = lb._edges(edges)
        x, y = np.ascontiguousarray(x, dtype=np.float32), np.ascontiguousarray(y, dtype=np.float32)
        assert x.shape == y.shape == (n,)
        fx, fy = np.zeros(n, dtype=np.float32), np.zeros(n, dtype=np.float32)
        terms = np.zeros(n, dtype=np.uint32)
        energy = c.c_double(0.)
        self.lib.em2rp_layout_forces(n, _ptr(v0), _ptr(v1), len(v0), gravity, depth, _ptr(x), _ptr(y), _ptr(fx), _ptr(fy), c.byref(energy),
                                     _ptr(terms))
        return fx, fy, energy.value, terms

    def layout(self, n, edges, depth=DEPTH_AUTO, **parameters):
        """-> (x, y, iterations, final step, final energy); parameters: the keys of layout_binding.DEFAULTS."""
        p = dict(lb.DEFAULTS)
        p.update(parameters)
        v0, v1 = lb._edges(edges)
        x, y = np.zeros(n, dtype=np.float32), np.zeros(n, dtype=np.float32)
        result = np.zeros(3, dtype=np.float64)
        self.lib.em2rp_layout(n, _ptr(v0), _ptr(v1), len(v0), p["seed"], p["maxIterationCount"], p["tolerance"], p["gravity"],
                              p["initialStep"], depth, _ptr(x), _ptr(y), _ptr(result))
        return x, y, int(result[0]), float(result[1]), float(result[2])


@functools.lru_cache(maxsize=None)
def load():
    build = os.path.join(lb.NATIVE_DIR, "build")
    os.makedirs(build, exist_ok=True)
    path = os.path.join(build, "libem2layoutpyramidrestatement.so")
    if not os.path.exists(path) or os.path.getmtime(path) < os.path.getmtime(SOURCE):
        tmp = path + ".%d.tmp" % os.getpid()
        cmd = ["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-o", tmp, SOURCE]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError("layout pyramid restatement build failed: " + r.stderr)
        os.replace(tmp, path)
    return PyramidRestatement(ctypes.CDLL(path))


@functools.lru_cache(maxsize=None)
def reference(name, iterations, depth=DEPTH_AUTO):
    """The restatement's run of a case of layout_binding with the default parameters but `iterations` as maxIterationCount;
    computed once and shared (the arrays are read-only)."""
    n, edges = lb.case(name)
    out = load().layout(n, edges, depth=depth, maxIterationCount=iterations)
    out[0].setflags(write=False)
    out[1].setflags(write=False)
    return out


# ---- the independent statement: float64, numpy ----

def numpy_cells(x, y, depth):
    """The quantised coordinates of the float32 positions (the same float32 operations: one subtraction, one correctly rounded
    division, a scaling by 2^31, a truncation) -> (qx, qy int64 [n], xmin, ymin, S as float32)."""
    x, y = np.asarray(x, dtype=np.float32), np.asarray(y, dtype=np.float32)
    xmin, ymin = x.min(), y.min()
    side = np.maximum(x.max() - xmin, y.max() - ymin)
    if side == 0:
        return np.zeros(len(x), np.int64), np.zeros(len(x), np.int64), xmin, ymin, side
    with np.errstate(invalid="ignore"):
        ux = np.minimum(np.maximum((x - xmin) / side, np.float32(0)), np.float32(1))
        uy = np.minimum(np.maximum((y - ymin) / side, np.float32(0)), np.float32(1))
    return (ux * np.float32(2 ** 31)).astype(np.int64), (uy * np.float32(2 ** 31)).astype(np.int64), xmin, ymin, side


def numpy_pyramid_forces(n, edges, gravity, x, y, depth):
    """The approximation in float64 with the same cells and lists and REAL-VALUED centroids (the float64 mean of the positions
    of a cell's vertices, not the quantised one), vectorised over the vertices: no loop, order or code of the kernel.
    -> (f [n, 2], absolute [n, 2]: the sum of the absolute values of each component's addends, terms [n]: the addends of the
    two repulsion sums, slack [n, 2]: what the quantisation of the centroids may change, see centroid_slack)."""
    p = np.stack([np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)], axis=1)
    qx, qy, xmin, ymin, side = numpy_cells(x, y, depth)
    f, absolute, slack = np.zeros((n, 2)), np.zeros((n, 2)), np.zeros((n, 2))
    terms = np.zeros(n, dtype=np.int64)
    for level in range(2, depth + 1):
        width = 2 ** level
        ax, ay = np.minimum(width - 1, qx >> (31 - level)), np.minimum(width - 1, qy >> (31 - level))
        cell = ay * width + ax
        count = np.bincount(cell, minlength=width * width).astype(np.float64)
        with np.errstate(invalid="ignore"):
            centroid = np.stack([np.bincount(cell, weights=p[:, k], minlength=width * width) / count for k in (0, 1)], axis=1)
        delta = centroid_slack(float(side), centroid)
        for oy in range(6):
            for ox in range(6):
                bx, by = 2 * ((ax >> 1) - 1) + ox, 2 * ((ay >> 1) - 1) + oy
                keep = (bx >= 0) & (by >= 0) & (bx < width) & (by < width) & (np.maximum(np.abs(bx - ax), np.abs(by - ay)) > 1)
                other = np.where(keep, by * width + bx, 0)
                keep &= count[other] > 0
                d = p[keep] - centroid[other[keep]]
                w = lb.C * lb.K * lb.K * count[other[keep]] / np.maximum((d ** 2).sum(axis=1), lb.FLOOR)
                f[keep] += d * w[:, None]
                absolute[keep] += np.abs(d * w[:, None])
                slack[keep] += (w * delta[other[keep]])[:, None]
                terms[keep] += 1
    width = 2 ** depth
    ax, ay = np.minimum(width - 1, qx >> (31 - depth)), np.minimum(width - 1, qy >> (31 - depth))
    for begin in range(0, n, 512):
        rows = slice(begin, begin + 512)
        near = (np.abs(ax[rows, None] - ax[None, :]) <= 1) & (np.abs(ay[rows, None] - ay[None, :]) <= 1)
        d = p[rows, None, :] - p[None, :, :]
        w = np.where(near, lb.C * lb.K * lb.K / np.maximum((d ** 2).sum(axis=2), lb.FLOOR), 0.)
        f[rows] += (d * w[:, :, None]).sum(axis=1)
        absolute[rows] += np.abs(d * w[:, :, None]).sum(axis=1)
        terms[rows] += near.sum(axis=1)
    v0, v1 = (np.asarray(e, dtype=np.int64) for e in edges)
    for a, b in ((v0, v1), (v1, v0)):
        d = p[a] - p[b]
        t = -d * (np.sqrt((d ** 2).sum(axis=1)) / lb.K)[:, None]
        np.add.at(f, a, t)
        np.add.at(absolute, a, np.abs(t))
    f -= gravity * p
    absolute += np.abs(gravity * p)
    return f, absolute, terms, slack


def centroid_slack(side, centroid):
    """How far a coordinate of the kernel's centroid may lie from the real-valued one, times 3 (below).
    The kernel's centroid is xmin + S * mean(q) / 2^31 rounded to float32, with q = floor(u * 2^31) and u the float32 value of
    (x - xmin) / S.  Three sources, per coordinate of one vertex and so of the mean:
      * the truncation to q: at most 2^-31 S (the term the quantisation itself contributes);
      * the two float32 roundings in u (the subtraction and the division, 2^-24 relative each on a value <= 1): 2^-23 S;
      * the rounding of the centroid to float32: 2^-24 |m|.
    A far term is g(m) = (p - m) w with w = C count / |p - m|^2; a displacement e of one coordinate of m changes a component of
    g by at most 2 w |e| to first order (|dg_x/dm_x| = w |1 - 2 dx^2 / d^2| <= w, |dg_x/dm_y| = w |2 dx dy / d^2| <= w, and
    both coordinates move), and |e| is below 2^-20 of the distance (a far centroid is a cell side away, a cell side is at least
    2^-10 S): the factor 3 covers the higher orders.  The caller multiplies by w and sums over the far terms."""
    per_coordinate = side * (2. ** -31 + 2. ** -23) + 2. ** -24 * np.abs(np.nan_to_num(centroid)).max(axis=1)
    return 3. * per_coordinate


def pyramid_force_bound(terms, absolute, slack):
    """(T + 8) 2^-24 sum|terms|, DESIGN.md 3.19's bound with the real number of terms T of the vertex's two sums, plus the
    quantisation of the centroids."""
    return (terms[:, None] + 8) * 2.0 ** -24 * absolute + slack


def check_against_numpy(forces, n, edges, gravity, x, y, depth, what):
    """forces: (fx, fy, energy, ...) of the code under test.  Every component within (T + 8) 2^-24 sum|terms| of the numpy
    statement, T the number of addends of the vertex's two repulsion sums (DESIGN.md 3.19's bound with the real term count),
    plus what the quantisation of the centroids contributes: sum over the far terms of 3 w e, with w = C count / d^2 the
    term's weight and e = (2^-31 + 2^-23) S + 2^-24 |m| the distance between a coordinate of the quantised float32 centroid
    and the real-valued one (derived in centroid_slack above)."""
    f, absolute, terms, slack = numpy_pyramid_forces(n, edges, gravity, x, y, depth)
    bound = pyramid_force_bound(terms, absolute, slack)
    error = np.abs(np.stack([forces[0], forces[1]], axis=1).astype(np.float64) - f)
    worst = float((error / np.maximum(bound, 1e-300)).max())
    print("%s: worst error / bound %.4f, terms %d ... %d" % (what, worst, terms.min(), terms.max()))
    assert np.all(error <= bound), what
    return terms


# ---- position sets for the forces entries: name -> (x, y float32, depth) ----

def _cloud(n, seed, side=None):
    rng = np.random.default_rng(seed)
    side = np.float32(np.sqrt(n) if side is None else side)
    return (rng.random(n, dtype=np.float32) - np.float32(0.5)) * side, (rng.random(n, dtype=np.float32) - np.float32(0.5)) * side


def _one_dense_leaf():
    """2 000 vertices inside one leaf of depth 4 and 48 spread over the box, shuffled: a wave of the walk then holds lanes whose
    near field is 2 000 long and lanes whose near field is their own vertex."""
    rng = np.random.default_rng(5)
    x, y = _cloud(48, 6, side=64.)
    x[0], y[0], x[1], y[1] = -32., -32., 32., 32.                        # the box: [-32, 32]^2, leaves of side 4
    dx, dy = rng.random(2000, dtype=np.float32) * np.float32(3.5), rng.random(2000, dtype=np.float32) * np.float32(3.5)
    x, y = np.concatenate([x, np.float32(8.25) + dx]), np.concatenate([y, np.float32(-11.75) + dy])
    order = rng.permutation(len(x))
    return x[order], y[order], 4


def _boundaries():
    """Positions on exact cell boundaries xmin + S k / 2^D: S = 16, D = 3, every (k, k') once and the far corner."""
    k = np.arange(9, dtype=np.float32) * np.float32(2.) - np.float32(5.)
    gx, gy = np.meshgrid(k, k)
    return gx.ravel().copy(), gy.ravel().copy(), 3


def _extremes():
    x, y = _cloud(200, 8)
    x[7], y[7] = np.float32(9.), np.float32(0.25)                        # the only vertex at xmax
    x[11], y[11] = np.float32(-0.5), np.float32(9.)                      # ... and at ymax
    return x, y, 3


def _coincident_pairs():
    x, y = _cloud(300, 9)
    x[3], y[3] = x[1], y[1]
    x[299], y[299] = x[0], y[0]
    return x, y, 3


@functools.lru_cache(maxsize=None)
def position_set(name):
    x, y, depth = {
        "one-vertex": lambda: (np.array([1.5], np.float32), np.array([-2.], np.float32), 2),
        "two-coincident": lambda: (np.array([1.5, 1.5], np.float32), np.array([-2., -2.], np.float32), 2),
        "all-coincident": lambda: (np.full(70, 0.75, np.float32), np.full(70, -3., np.float32), 3),
        "vertical-line": lambda: (np.full(130, 2., np.float32), _cloud(130, 3)[1], 4),
        "at-xmax-and-ymax": _extremes,
        "cell-boundaries": _boundaries,
        "coincident-pairs": _coincident_pairs,
        "one-dense-leaf": _one_dense_leaf,
    }[name]()
    x.setflags(write=False)
    y.setflags(write=False)
    return x, y, depth


POSITION_SETS = ["one-vertex", "two-coincident", "all-coincident", "vertical-line", "at-xmax-and-ymax", "cell-boundaries",
                 "coincident-pairs", "one-dense-leaf"]


def position_set_edges(n):
    """A few edges for a position set: a path over the first vertices and one self-loop."""
    pairs = [(i, i + 1) for i in range(min(n, 40) - 1)] + [(0, 0)]
    return lb._graph(n, pairs)[1]
