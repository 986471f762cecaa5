"""em2_cell_graph_compare and em2_graph_group_colors on the GPU against the one-thread restatement
(tests/native/em2_graph_compare_restatement.cpp): every counter and every array equal, the floats by their bits, on both paths
and through both the host entry and the em2_dev_ entry (edge arrays in device memory)."""
import ctypes
import functools

import numpy as np
import pytest

import graph_compare_binding as gb
from expressionmatrix2_amd import capi

pytestmark = pytest.mark.gpu

F = np.float32
EM2_ERROR_RUNTIME = 5
PATHS = (capi.GRAPH_COMPARE_TABLE, capi.GRAPH_COMPARE_LIST)
GRID_THREADS = 1024 * 256                   # the kernels' grids are capped at 1024 blocks of 256 threads


def sized(rng, edges):
    vertices = max(4, edges // 3)
    g0 = gb.random_graph(rng, np.arange(3 * vertices, dtype=np.uint32) * np.uint32(5) + np.uint32(1), vertices, edges)
    return g0, gb.similar_graph(rng, g0)


def float_case(pairs):
    """Edges (i, i + 1) in key order with the similarities pairs[i] = (s0, s1), and an edge only graph 0 has in front."""
    s0 = [F(0.3)] + [F(a) for a, _ in pairs]
    s1 = [F(b) for _, b in pairs]
    cells, v0, v1, _ = gb.path_graph(len(s0), s0)
    return gb.graph(cells, v0, v1, s0), gb.graph(cells, v0[1:], v1[1:], s1)


@functools.lru_cache(maxsize=None)
def cases():
    rng = np.random.default_rng(99)
    out = {}
    # sizes
    for edges in (1, 63, 64, 65, 257, 1000):
        out["%d edges" % edges] = sized(rng, edges)
    g0, g1 = sized(rng, 50)
    out["no edges in graph 0"] = (gb.graph(g0[0], [], [], []), g1)
    out["no edges in graph 1"] = (g0, gb.graph(g1[0], [], [], []))
    out["no edges"] = (gb.graph(g0[0], [], [], []), gb.graph(g1[0], [], [], []))
    out["no vertices"] = (gb.graph([], [], [], []), gb.graph([], [], [], []))
    out["no vertices in graph 1"] = (g0, gb.graph([], [], [], []))
    out["100000 edges"] = sized(rng, 100000)
    out["a second trip of the grid"] = sized(rng, GRID_THREADS + 40000)
    # vertex numbering
    g0 = gb.random_graph(rng, np.arange(100, dtype=np.uint32), 60, 300)
    out["another vertex order"] = (g0, gb.similar_graph(rng, g0, keep=1.0, changed=0.0))
    out["disjoint cells"] = (g0, gb.random_graph(rng, np.arange(100, 200, dtype=np.uint32), 60, 300))
    subset = gb.random_graph(rng, g0[0][:30], 30, 120)
    out["a subset of the cells"] = (g0, subset)
    out["a superset of the cells"] = (subset, g0)
    out["a repeated cell id"] = (gb.graph([5, 5, 7, 9, 5], [0, 1, 4, 2], [3, 2, 3, 3], [0.5, 0.25, 0.75, 0.4]),
                                 gb.graph([9, 5, 5, 5, 7, 7], [0, 4, 5], [1, 2, 0], [0.5, 0.3, 0.4]))
    # the key uses all 64 bits
    wide = [0, 2 ** 31, 2 ** 32 - 2, 5, 2 ** 31 + 1]
    pairs = [(a, b) for a in range(5) for b in range(a + 1, 5)]
    out["cell ids up to 2^32 - 2"] = (gb.graph(wide, [a for a, _ in pairs], [b for _, b in pairs], np.linspace(0.1, 0.9, 10)),
                                      gb.graph(wide[::-1], [4 - b for a, b in pairs[2:]], [4 - a for a, b in pairs[2:]],
                                               np.linspace(0.3, 0.9, 8)))
    # duplicates: the first in edge order stays, in graph 0 and in graph 1
    out["duplicates"] = (gb.graph([1, 2, 3], [0, 1, 1, 2, 0], [1, 0, 2, 1, 1], [0.25, 0.75, 0.5, 0.1, 0.9]),
                         gb.graph([2, 1, 3], [0, 1, 2, 0, 0], [1, 0, 0, 2, 1], [0.75, 0.25, 0.2, 0.5, 0.6]))
    # the ends of the join
    path = gb.path_graph(50, np.full(50, 0.5))
    out["the first and the last key of graph 1"] = (gb.graph(np.arange(51), [0, 49, 0, 3], [1, 50, 50, 7], [0.5, 0.6, 0.1, 0.2]), path)
    out["no common edge"] = (gb.graph(np.arange(51), np.arange(49), np.arange(2, 51), np.full(49, 0.5)), path)
    g0 = gb.random_graph(rng, np.arange(500, dtype=np.uint32), 200, 1000)
    out["all edges common"] = (g0, gb.similar_graph(rng, g0, keep=1.0, changed=0.0))
    # float cases
    filler = [(0.5, 0.499), (0.5, 0.501), (0.5, 0.5), (0.5, 0.6)]
    out["zero bin: +0 first"] = float_case([(0.5, 0.5)] + filler)
    out["zero bin: -0.000999987 first"] = float_case([(0.5, 0.499)] + filler)
    out["zero bin: +0.000999987 first"] = float_case([(0.5, 0.501)] + filler)
    out["zero bin: a negative denormal first"] = float_case([(np.uint32(1).view(np.float32), 0.0)] + filler)
    out["quotients of +-0.5"] = float_case([(0.0, 0.005), (0.0, -0.005)])
    out["a quotient of 0.4999995"] = float_case([(0.2, 0.205)])
    out["a quotient of 1.5"] = float_case([(0.0, 0.015)])
    out["the edge of the table"] = float_case([(0.0, s) for s in (20.47, 20.475, 20.48, 20.485, 20.49, 20.5, -20.47, -20.475, -20.48,
                                                                  -20.485, -20.49, -20.5, 20.48, -20.49)])
    out["bins of +-inf"] = float_case([(-3e38, 3e38), (3e38, -3e38), (0.5, 0.5), (-3e38, 3e38), (1e37, -1e37)])
    out["-0 against +0"] = float_case([(-0.0, 0.0), (0.0, -0.0)])
    # contention and counters
    n = 100000
    out["100000 edges in one bin"] = (gb.path_graph(n, np.full(n, 0.5)), gb.path_graph(n, np.full(n, 0.5)))
    spread = (F(0.5) + (np.arange(n) % 400 - 200).astype(np.float32) * F(0.01)).astype(np.float32)
    out["100000 edges in 400 bins"] = (gb.path_graph(n, np.full(n, 0.5)), gb.path_graph(n, spread))
    # a NaN on an edge only one graph has
    out["NaN on uncommon edges"] = (gb.graph([1, 2, 3], [0, 1], [1, 2], [0.5, np.nan]),
                                    gb.graph([3, 1, 2, 8], [1, 0], [2, 3], [0.25, np.nan]))
    return out


CASE_NAMES = sorted(cases())


@functools.lru_cache(maxsize=None)
def expected(name):
    status, reference = gb.load().compare(*cases()[name])
    assert status == gb.OK
    return reference


def on_device(g):
    """The three edge arrays of a graph in device memory: (tensors to keep, the arguments of dev_cell_graph_compare)."""
    import torch
    cells, v0, v1, similarity = g
    tensors = [torch.from_numpy(v0.view(np.int32).copy()).cuda(), torch.from_numpy(v1.view(np.int32).copy()).cuda(),
               torch.from_numpy(similarity.copy()).cuda()]
    torch.cuda.synchronize()
    return tensors, (cells, tensors[0].data_ptr(), tensors[1].data_ptr(), tensors[2].data_ptr(), len(v0))


def both_entries(g0, g1, path):
    host = capi.cell_graph_compare(g0, g1, path)
    keep0, arguments0 = on_device(g0)
    keep1, arguments1 = on_device(g1)
    device = capi.dev_cell_graph_compare(*arguments0, *arguments1, path)
    del keep0, keep1
    return host, device


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("name", CASE_NAMES)
def test_comparison_equals_the_restatement(name, path):
    g0, g1 = cases()[name]
    for entry, mine in zip(("host", "device"), both_entries(g0, g1, path)):
        assert mine["path"] == path
        gb.assert_same_comparison(mine, expected(name), "%s, %s entry, path %d" % (name, entry, path))


def test_the_cases_are_what_their_names_say():
    assert expected("no common edge")["commonEdgeCount"] == 0 and expected("no common edge")["edgeCount0"] == 49
    assert expected("all edges common")["commonEdgeCount"] == expected("all edges common")["edgeCount0"] > 900
    assert expected("the first and the last key of graph 1")["commonEdgeCount"] == 2
    assert expected("another vertex order")["commonVertexCount"] == 60 and expected("disjoint cells")["commonVertexCount"] == 0
    assert expected("a subset of the cells")["commonVertexCount"] == 30
    assert expected("a repeated cell id")["commonVertexCount"] == 5
    assert expected("duplicates")["edgeCount0"] == 2 and expected("duplicates")["edgeCount1"] == 2
    assert expected("duplicates")["binDelta"].tolist() == [float(F(0.01) * F(-30.0)), float(F(0.01) * F(50.0))]
    assert expected("a second trip of the grid")["edgeCount0"] > GRID_THREADS
    assert expected("cell ids up to 2^32 - 2")["commonEdgeCount"] == 8
    assert expected("100000 edges in one bin")["binCount"].tolist() == [100000]
    assert len(expected("100000 edges in 400 bins")["binCount"]) == 400
    assert gb.bits(expected("bins of +-inf")["binDelta"]).tolist()[0] == 0xff800000
    assert gb.bits(expected("bins of +-inf")["binDelta"]).tolist()[-1] == 0x7f800000
    assert gb.bits(expected("zero bin: -0.000999987 first")["binDelta"]).tolist()[0] == 0x80000000
    assert gb.bits(expected("zero bin: a negative denormal first")["binDelta"]).tolist()[0] == 0x80000000
    assert gb.bits(expected("zero bin: +0.000999987 first")["binDelta"]).tolist()[0] == 0
    edge = expected("the edge of the table")["binDelta"]
    for r in (2047.0, 2048.0, 2049.0, 2050.0):
        assert F(0.01) * F(r) in edge and F(0.01) * F(-r) in edge
    assert expected("NaN on uncommon edges")["commonEdgeCount"] == 1


def raw_compare(g0, g1, path):
    lib = capi.load()
    handle = ctypes.c_void_p(None)
    rc = lib.em2_cell_graph_compare(capi._ptr(g0[0]), len(g0[0]), capi._ptr(g0[1]), capi._ptr(g0[2]), capi._ptr(g0[3]), len(g0[1]),
                                    capi._ptr(g1[0]), len(g1[0]), capi._ptr(g1[1]), capi._ptr(g1[2]), capi._ptr(g1[3]), len(g1[1]),
                                    path, ctypes.byref(handle))
    return rc, capi.last_error(), handle.value


@pytest.mark.parametrize("path", PATHS)
def test_errors(path):
    good = gb.graph([1, 2, 3], [0, 1], [1, 2], [0.5, 0.25])
    restatement = gb.load()
    # a NaN on a common edge, and a difference of two infinities
    for s0, s1 in ((np.nan, 0.5), (0.5, np.nan), (np.inf, np.inf)):
        g0, g1 = gb.graph([7, 11, 3], [0, 2], [1, 0], [s0, 0.5]), gb.graph([11, 7], [0], [1], [s1])
        assert restatement.compare(g0, g1)[0] == gb.NOT_A_NUMBER
        rc, text, handle = raw_compare(g0, g1, path)
        assert rc == capi.EM2_ERROR_UNSUPPORTED and handle is None and "cells 7 and 11" in text, text
        keep0, arguments0 = on_device(g0)
        keep1, arguments1 = on_device(g1)
        with pytest.raises(RuntimeError, match="em2_dev_cell_graph_compare: .*cells 7 and 11 is not a number"):
            capi.dev_cell_graph_compare(*arguments0, *arguments1, path)
    # an edge between a cell and itself (two vertices of one cell), in either graph
    loop = gb.graph([4, 9, 4], [0, 0], [1, 2], [0.5, 0.5])
    for g0, g1, which in ((loop, good, 0), (good, loop, 1)):
        assert restatement.compare(g0, g1)[0] == gb.SELF_LOOP
        rc, text, handle = raw_compare(g0, g1, path)
        assert rc == EM2_ERROR_RUNTIME and handle is None
        assert text == "em2_cell_graph_compare: graph %d, edge 1: cellIdA != cellIdB (both ends are cell 4)" % which
    # a vertex index out of range: no object
    for bad in (gb.graph([1, 2, 3], [0, 3], [1, 2], [0.5, 0.25]), gb.graph([1, 2, 3], [0, 1], [1, 2 ** 32 - 1], [0.5, 0.25]),
                gb.graph([], [0], [0], [0.5])):
        for g0, g1, which in ((bad, good, 0), (good, bad, 1)):
            assert restatement.compare(g0, g1)[0] == gb.BAD_INDEX
            rc, text, handle = raw_compare(g0, g1, path)
            assert rc == capi.EM2_ERROR_INVALID_ARGUMENT and handle is None
            assert text == "em2_cell_graph_compare: graph %d, edge %d: a vertex index is not below the vertex count" % (which, len(bad[1]) - 1)
    with pytest.raises(RuntimeError, match="path must be 0"):
        capi.cell_graph_compare(good, good, 2)
    # the library works after its refusals
    gb.assert_same_comparison(capi.cell_graph_compare(good, good, path), restatement.compare(good, good)[1], "after the errors")


@pytest.mark.parametrize("chunk", range(4))
def test_fuzz(chunk):
    """200 random pairs of graphs in four chunks: sizes around the wave and block sizes, similarities from a grid of 19 values
    with a few per cent moved a little, so that identical and nearly identical edges both occur."""
    rng = np.random.default_rng(1000 + chunk)
    restatement = gb.load()
    sizes = (0, 1, 2, 7, 63, 64, 65, 300)
    for trial in range(50):
        pool = np.arange(60, dtype=np.uint32) * np.uint32(rng.integers(1, 1000)) + np.uint32(rng.integers(0, 5))
        g0 = gb.random_graph(rng, pool, int(rng.integers(2, 40)), int(rng.choice(sizes)))
        if trial % 2:
            g1 = gb.similar_graph(rng, g0)
        else:
            g1 = gb.random_graph(rng, pool, int(rng.integers(2, 40)), int(rng.choice(sizes)))
        status, reference = restatement.compare(g0, g1)
        assert status == gb.OK
        for path in PATHS:
            for entry, mine in zip(("host", "device"), both_entries(g0, g1, path)):
                gb.assert_same_comparison(mine, reference, "chunk %d trial %d, %s entry, path %d" % (chunk, trial, entry, path))


# ---- the group graph and its colours ----

def group_cases():
    rng = np.random.default_rng(7)
    out = {}
    out["one group"] = (np.zeros(6), [0, 1, 2], [1, 2, 3])
    out["inside groups"] = ([0, 0, 1, 1, 2, 2], [0, 2, 4], [1, 3, 5])
    out["a path of 20 groups"] = (np.arange(20), np.arange(19), np.arange(1, 20))
    clique = [(a, b) for a in range(13) for b in range(a + 1, 13)]
    out["a clique of 13 groups"] = (np.arange(13), [a for a, _ in clique], [b for _, b in clique])
    out["gaps"] = ([0, 3, 3, 7, 9], [0, 1, 3, 2], [1, 3, 4, 4])
    out["own groups"] = (rng.permutation(300), rng.integers(0, 300, 900), rng.integers(0, 300, 900))
    out["high low"] = ([0, 1, 2, 3], [3, 2, 1], [0, 0, 0])
    out["low high"] = ([0, 1, 2, 3], [0, 0, 0], [3, 2, 1])
    out["both ways"] = ([0, 1, 2, 3], [0, 3, 1, 2, 0], [3, 0, 2, 1, 3])
    out["random"] = (rng.integers(0, 25, 200), rng.integers(0, 200, 1500), rng.integers(0, 200, 1500))
    out["a second trip of the grid"] = (rng.integers(0, 40, 5000), rng.integers(0, 5000, GRID_THREADS + 1000),
                                        rng.integers(0, 5000, GRID_THREADS + 1000))
    out["no edges"] = ([2, 0, 1], [], [])
    out["nothing"] = ([], [], [])
    return out


GROUP_CASES = group_cases()


@pytest.mark.parametrize("path", (capi.CONTINGENCY_LDS, capi.CONTINGENCY_SORT))
@pytest.mark.parametrize("name", sorted(GROUP_CASES))
def test_group_colors_equal_the_restatement(name, path):
    import torch
    group, v0, v1 = GROUP_CASES[name]
    status, reference = gb.load().group_colors(group, v0, v1)
    assert status == gb.OK
    gb.assert_proper(reference, name)
    groups = reference["groupCount"]
    if path == capi.CONTINGENCY_LDS and groups * groups > capi.CONTINGENCY_LDS_CELLS:
        assert name == "own groups"                                # 300 groups: the sort path only
        with pytest.raises(RuntimeError, match="the LDS path holds a table of at most 16384 cells"):
            capi.graph_group_colors(group, v0, v1, path)
        mine = capi.graph_group_colors(group, v0, v1, capi.CONTINGENCY_AUTOMATIC)
        assert mine["path"] == capi.CONTINGENCY_SORT
        gb.assert_same_group_colors(mine, reference, name)
        return
    mine = capi.graph_group_colors(group, v0, v1, path)
    assert mine["path"] == (path if len(v0) else 0)
    gb.assert_same_group_colors(mine, reference, "%s, host entry, path %d" % (name, path))
    d0 = torch.from_numpy(np.asarray(v0, dtype=np.uint32).view(np.int32).copy()).cuda()
    d1 = torch.from_numpy(np.asarray(v1, dtype=np.uint32).view(np.int32).copy()).cuda()
    torch.cuda.synchronize()
    device = capi.dev_graph_group_colors(group, d0.data_ptr(), d1.data_ptr(), len(v0), path)
    gb.assert_same_group_colors(device, reference, "%s, device entry, path %d" % (name, path))
    if name == "a path of 20 groups":
        assert mine["colorTable"].tolist() == [0, 1] * 10
    if name == "a clique of 13 groups":
        assert mine["colorTable"].tolist() == list(range(13))


def test_group_colors_refuse_an_index_out_of_range():
    for group, v0, v1 in (([0, 1], [0], [2]), ([0, 1], [2 ** 32 - 1], [0]), ([], [0], [0])):
        assert gb.load().group_colors(group, v0, v1)[0] == gb.BAD_INDEX
        for path in (capi.CONTINGENCY_AUTOMATIC, capi.CONTINGENCY_LDS, capi.CONTINGENCY_SORT):
            with pytest.raises(RuntimeError) as error:
                capi.graph_group_colors(group, v0, v1, path)
            assert str(error.value) == "em2_graph_group_colors: a vertex index is not below the vertex count"
