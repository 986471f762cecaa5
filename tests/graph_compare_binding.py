"""ctypes binding of tests/native/em2_graph_compare_restatement.cpp (compareCellGraphs with two std::map of edges, a
std::map<float, size_t> histogram and std::set_intersection; assignColorsToGroups with a std::set adjacency), an independent
Python statement of both, and the inputs the graph comparison tests share.  Compiled with g++ at first use.  Test
infrastructure only."""
import ctypes
import ctypes.util
import functools
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE_DIR = os.path.join(ROOT, "tests", "native")
SOURCE = os.path.join(NATIVE_DIR, "em2_graph_compare_restatement.cpp")

OK, BAD_INDEX, SELF_LOOP, NOT_A_NUMBER = 0, 1, 2, 3
COUNT_KEYS = ("commonVertexCount", "edgeCount0", "edgeCount1", "commonEdgeCount", "commonIdenticalEdgeCount")

c = ctypes
P = c.c_void_p
F = np.float32


def _ptr(a):
    return a.ctypes.data_as(c.c_void_p)


def graph(cells, v0, v1, similarity):
    """(vertexCellIds, edgeVertex0, edgeVertex1, edgeSimilarity) as the arrays the entries take."""
    return (np.ascontiguousarray(cells, dtype=np.uint32), np.ascontiguousarray(v0, dtype=np.uint32),
            np.ascontiguousarray(v1, dtype=np.uint32), np.ascontiguousarray(similarity, dtype=np.float32))


class GraphCompareRestatement:
    def __init__(self, lib):
        self.lib = lib
        lib.em2r_gc_compare.argtypes = [P, c.c_uint32, P, P, P, c.c_uint64] * 2 + [P, P, P, c.POINTER(c.c_uint64)]
        lib.em2r_gc_compare.restype = c.c_int
        lib.em2r_gc_group_colors.argtypes = [P, c.c_uint32, P, P, c.c_uint64, c.POINTER(c.c_uint32), P, P, P, c.POINTER(c.c_uint64), P]
        lib.em2r_gc_group_colors.restype = c.c_int

    def compare(self, graph0, graph1):
        """-> (status, dict): the dict of capi.graph_comparison_take without path; None where status is not OK."""
        g0, g1 = graph(*graph0), graph(*graph1)
        capacity = max(1, min(len(g0[1]), len(g1[1])))
        counts = np.zeros(5, dtype=np.uint64)
        delta = np.zeros(capacity, dtype=np.float32)
        count = np.zeros(capacity, dtype=np.uint64)
        bins = c.c_uint64(0)
        status = self.lib.em2r_gc_compare(_ptr(g0[0]), len(g0[0]), _ptr(g0[1]), _ptr(g0[2]), _ptr(g0[3]), len(g0[1]),
                                          _ptr(g1[0]), len(g1[0]), _ptr(g1[1]), _ptr(g1[2]), _ptr(g1[3]), len(g1[1]),
                                          _ptr(counts), _ptr(delta), _ptr(count), c.byref(bins))
        if status != OK:
            return status, None
        out = {key: int(value) for key, value in zip(COUNT_KEYS, counts)}
        out["binDelta"] = delta[:bins.value].copy()
        out["binCount"] = count[:bins.value].copy()
        return status, out

    def group_colors(self, group, v0, v1):
        """-> (status, dict): the dict of capi.group_colors_take without path; None where status is not OK."""
        group = np.ascontiguousarray(group, dtype=np.uint32)
        v0 = np.ascontiguousarray(v0, dtype=np.uint32)
        v1 = np.ascontiguousarray(v1, dtype=np.uint32)
        groups = int(group.max()) + 1 if len(group) else 0
        capacity = max(1, len(v0))
        pair0 = np.zeros(capacity, dtype=np.uint32)
        pair1 = np.zeros(capacity, dtype=np.uint32)
        edges = np.zeros(capacity, dtype=np.uint64)
        table = np.zeros(max(1, groups), dtype=np.uint32)
        group_count, pair_count = c.c_uint32(0), c.c_uint64(0)
        status = self.lib.em2r_gc_group_colors(_ptr(group), len(group), _ptr(v0), _ptr(v1), len(v0), c.byref(group_count), _ptr(pair0),
                                               _ptr(pair1), _ptr(edges), c.byref(pair_count), _ptr(table))
        if status != OK:
            return status, None
        n = pair_count.value
        return status, {"groupCount": int(group_count.value), "pairGroup0": pair0[:n].copy(), "pairGroup1": pair1[:n].copy(),
                        "pairEdgeCount": edges[:n].copy(), "colorTable": table[:group_count.value].copy()}


@functools.lru_cache(maxsize=None)
def load():
    build = os.path.join(NATIVE_DIR, "build")
    os.makedirs(build, exist_ok=True)
    path = os.path.join(build, "libem2graphcomparerestatement.so")
    if not os.path.exists(path) or os.path.getmtime(path) < os.path.getmtime(SOURCE):
        tmp = path + ".%d.tmp" % os.getpid()
        # -ffp-contract=off: the bin is a difference, a quotient, std::round and a product, each rounded on its own
        cmd = ["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-o", tmp, SOURCE]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError("graph compare restatement build failed: " + r.stderr)
        os.replace(tmp, path)
    return GraphCompareRestatement(ctypes.CDLL(path))


# ---- an independent statement in Python ----

@functools.lru_cache(maxsize=None)
def _libm():
    libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
    libm.roundf.argtypes, libm.roundf.restype = [c.c_float], c.c_float
    return libm


def bin_of(s0, s1):
    """0.01f * std::round((s1 - s0) / 0.01f) in float32 operations; roundf is libm's (numpy's and Python's round are ties to even)."""
    with np.errstate(all="ignore"):
        delta = F(s1) - F(s0)
        quotient = delta / F(0.01)
        return F(0.01) * F(_libm().roundf(float(quotient)))


def bits(values):
    return np.ascontiguousarray(values, dtype=np.float32).view(np.uint32)


def python_compare(graph0, graph1):
    """The comparison with dicts, Counter-like multisets and np.float32 scalars -> the dict of GraphCompareRestatement.compare
    (graphs without errors only)."""
    maps = []
    for cells, v0, v1, similarity in (graph(*graph0), graph(*graph1)):
        edges = {}
        for a, b, s in zip(cells[v0].tolist(), cells[v1].tolist(), similarity):
            edges.setdefault((min(a, b), max(a, b)), F(s))
        maps.append(edges)
    multiset = [{}, {}]
    for which, g in enumerate((graph0, graph1)):
        for cell in np.asarray(g[0]).tolist():
            multiset[which][cell] = multiset[which].get(cell, 0) + 1
    out = {"commonVertexCount": sum(min(n, multiset[1].get(cell, 0)) for cell, n in multiset[0].items()),
           "edgeCount0": len(maps[0]), "edgeCount1": len(maps[1]), "commonEdgeCount": 0, "commonIdenticalEdgeCount": 0}
    histogram = []                                   # [key, count] in insertion order; the two zeros are one key
    for key in sorted(maps[0]):
        if key not in maps[1]:
            continue
        s0, s1 = maps[0][key], maps[1][key]
        out["commonEdgeCount"] += 1
        out["commonIdenticalEdgeCount"] += 1 if s0 == s1 else 0
        product = bin_of(s0, s1)
        for entry in histogram:
            if entry[0] == product:
                entry[1] += 1
                break
        else:
            histogram.append([product, 1])
    histogram.sort(key=lambda entry: float(entry[0]))
    out["binDelta"] = np.asarray([entry[0] for entry in histogram], dtype=np.float32)
    out["binCount"] = np.asarray([entry[1] for entry in histogram], dtype=np.uint64)
    return out


def python_group_colors(group, v0, v1):
    """The group graph and the literal greedy -> the dict of GraphCompareRestatement.group_colors."""
    group = np.asarray(group, dtype=np.int64)
    groups = int(group.max()) + 1 if len(group) else 0
    between = {}
    for a, b in zip(group[np.asarray(v0, dtype=np.int64)].tolist(), group[np.asarray(v1, dtype=np.int64)].tolist()):
        if a != b:
            between[(min(a, b), max(a, b))] = between.get((min(a, b), max(a, b)), 0) + 1
    table = []
    for g in range(groups):
        adjacent = sorted(set(table[low] for (low, high) in between if high == g))
        color = len(adjacent)
        for index, value in enumerate(adjacent):
            if value != index:
                color = index
                break
        table.append(color)
    pairs = sorted(between)
    return {"groupCount": groups, "pairGroup0": np.asarray([p[0] for p in pairs], dtype=np.uint32),
            "pairGroup1": np.asarray([p[1] for p in pairs], dtype=np.uint32),
            "pairEdgeCount": np.asarray([between[p] for p in pairs], dtype=np.uint64), "colorTable": np.asarray(table, dtype=np.uint32)}


def assert_same_comparison(mine, theirs, what):
    for key in COUNT_KEYS:
        assert mine[key] == theirs[key], "%s: %s %d != %d" % (what, key, mine[key], theirs[key])
    assert mine["binCount"].dtype == theirs["binCount"].dtype == np.uint64 and mine["binDelta"].dtype == np.float32
    assert np.array_equal(bits(mine["binDelta"]), bits(theirs["binDelta"])), \
        "%s: binDelta %s != %s" % (what, mine["binDelta"].tolist(), theirs["binDelta"].tolist())
    assert np.array_equal(mine["binCount"], theirs["binCount"]), "%s: binCount differs" % what
    assert int(mine["binCount"].sum()) == mine["commonEdgeCount"], "%s: the bins do not sum to the common edges" % what


def assert_same_group_colors(mine, theirs, what):
    assert mine["groupCount"] == theirs["groupCount"], "%s: groupCount" % what
    for key in ("pairGroup0", "pairGroup1", "pairEdgeCount", "colorTable"):
        assert mine[key].dtype == theirs[key].dtype and np.array_equal(mine[key], theirs[key]), "%s: %s differs" % (what, key)


def assert_proper(colors, what):
    """No pair of the group graph joins two groups of one colour."""
    table = colors["colorTable"]
    same = table[colors["pairGroup0"]] == table[colors["pairGroup1"]]
    assert not same.any(), "%s: adjacent groups share a colour" % what


# ---- inputs ----

def pair_of_edges(s0, s1, cells=(3, 9)):
    """Two graphs of one edge each between the same two cells, with similarities s0 and s1."""
    return graph(cells, [0], [1], [s0]), graph(cells, [1], [0], [s1])

def path_graph(n, similarity):
    """Cells 0 ... n, edges (i, i + 1) with similarity[i]: their keys ascend with i."""
    return graph(np.arange(n + 1), np.arange(n), np.arange(1, n + 1), similarity)


SIMILARITY_GRID = (np.arange(19, dtype=np.float32) * F(0.05) + F(0.05)).astype(np.float32)


def random_graph(rng, cell_pool, vertex_count, edge_count, perturbed=0.03):
    """A graph of vertex_count vertices drawn from cell_pool without repeats (at least 2 where there are edges), edge_count
    edges between distinct vertices, similarities from SIMILARITY_GRID with a few per cent moved by up to 2e-3."""
    cells = rng.choice(cell_pool, size=vertex_count, replace=False).astype(np.uint32)
    if edge_count == 0 or vertex_count < 2:
        return graph(cells, [], [], [])
    v0 = rng.integers(0, vertex_count, size=edge_count)
    v1 = (v0 + rng.integers(1, vertex_count, size=edge_count)) % vertex_count
    similarity = SIMILARITY_GRID[rng.integers(0, len(SIMILARITY_GRID), size=edge_count)].copy()
    moved = rng.random(edge_count) < perturbed
    similarity[moved] += (rng.random(int(moved.sum())) * 4e-3 - 2e-3).astype(np.float32)
    return graph(cells, v0, v1, similarity)


def similar_graph(rng, g, keep=0.7, changed=0.3, shuffle=True):
    """A second graph of the same cells in another vertex order that keeps a share of g's edges (some with another similarity,
    some turned round) and adds none."""
    cells, v0, v1, similarity = g
    n = len(cells)
    order = rng.permutation(n) if shuffle else np.arange(n)
    position = np.empty(n, dtype=np.int64)
    position[order] = np.arange(n)
    kept = rng.random(len(v0)) < keep
    a, b, s = position[v0[kept]], position[v1[kept]], similarity[kept].copy()
    turn = rng.random(len(a)) < 0.5
    a, b = np.where(turn, b, a), np.where(turn, a, b)
    move = rng.random(len(a)) < changed
    s[move] = SIMILARITY_GRID[rng.integers(0, len(SIMILARITY_GRID), size=int(move.sum()))]
    return graph(cells[order], a, b, s)
