"""ctypes binding of tests/native/em2_cluster_graph_restatement.cpp, the C++ restatement of what
ExpressionMatrix::createClusterGraph does after the label propagation (src/ExpressionMatrix.cpp:2153-2181,
src/ClusterGraph.cpp:59-386, src/ExpressionMatrix.cpp:1179-1296, src/regressionCoefficient.cpp), and the inputs the
cluster graph tests share.  Compiled with g++ at first use, with the flags of fsp0_binding.  Test infrastructure only."""
import ctypes
import os
import subprocess

import numpy as np

import fsp0_binding
import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE_DIR = os.path.join(ROOT, "tests", "native")
SOURCE = os.path.join(NATIVE_DIR, "em2_cluster_graph_restatement.cpp")

COUNT_DTYPE = fsp0_binding.COUNT_DTYPE

c = ctypes
P = c.c_void_p

RESULT_KEYS = ("clusterIds", "cellOffsets", "cells", "unclusteredCells", "averages", "edgeCluster0", "edgeCluster1",
               "edgeSimilarity")


def _ptr(a):
    return a.ctypes.data_as(c.c_void_p)


class NanSimilarity(RuntimeError):
    pass


class ClusterGraphRestatement:
    def __init__(self, lib):
        self.lib = lib
        lib.em2r_cluster_average_expression.argtypes = [P, P, c.c_uint32, P, P, c.c_uint32, P]
        lib.em2r_cluster_average_expression.restype = None
        lib.em2r_cluster_similarities.argtypes = [P, c.c_uint32, P, P, c.c_uint64, P]
        lib.em2r_cluster_similarities.restype = None
        lib.em2r_cluster_graph_create.argtypes = [P, P, c.c_uint32, P, c.c_uint32, P, P, c.c_uint64, P, c.c_uint64, c.c_uint64,
                                                  c.c_double, c.c_double, c.c_int, c.POINTER(P)]
        lib.em2r_cluster_graph_create.restype = c.c_int
        lib.em2r_cluster_graph_sizes.argtypes = [P, c.POINTER(c.c_uint32), c.POINTER(c.c_uint64), c.POINTER(c.c_uint64),
                                                 c.POINTER(c.c_uint64), c.POINTER(c.c_int)]
        lib.em2r_cluster_graph_sizes.restype = None
        lib.em2r_cluster_graph_get.argtypes = [P] * 9
        lib.em2r_cluster_graph_get.restype = None
        lib.em2r_cluster_graph_free.argtypes = [P]
        lib.em2r_cluster_graph_free.restype = None
        lib.em2r_sort_by_size.argtypes = [P, c.c_uint32, c.c_int, P]
        lib.em2r_sort_by_size.restype = None

    def average_expression(self, toc, data, gene_count, cluster_cells, cluster_offsets):
        toc = np.ascontiguousarray(toc, dtype=np.uint64)
        data = np.ascontiguousarray(data, dtype=COUNT_DTYPE)
        cells = np.ascontiguousarray(cluster_cells, dtype=np.uint32)
        offsets = np.ascontiguousarray(cluster_offsets, dtype=np.uint64)
        out = np.zeros((len(offsets) - 1, gene_count), dtype=np.float64)
        self.lib.em2r_cluster_average_expression(_ptr(toc), _ptr(data), gene_count, _ptr(cells), _ptr(offsets), len(offsets) - 1,
                                                 _ptr(out))
        return out

    def similarities(self, averages, edge0, edge1):
        averages = np.ascontiguousarray(averages, dtype=np.float64)
        e0 = np.ascontiguousarray(edge0, dtype=np.uint32)
        e1 = np.ascontiguousarray(edge1, dtype=np.uint32)
        out = np.zeros(len(e0), dtype=np.float64)
        self.lib.em2r_cluster_similarities(_ptr(averages), averages.shape[1], _ptr(e0), _ptr(e1), len(e0), _ptr(out))
        return out

    def create(self, toc, data, gene_count, vertex_rows, edge_vertex0, edge_vertex1, labels, min_cluster_size=100, k=3,
               similarity_threshold=0.5, similarity_threshold_for_merge=0.9, stop_after=0):
        """-> dict with RESULT_KEYS as capi.cluster_graph_create, plus knnTie (whether makeKnn's tie rule decided anything).
        Raises NanSimilarity where the device code must fail.  stop_after 1 / 2 / 3: the graph after the first similarities /
        the merge / removeSmallVertices and the second similarities, cluster ids still the labels."""
        toc = np.ascontiguousarray(toc, dtype=np.uint64)
        data = np.ascontiguousarray(data, dtype=COUNT_DTYPE)
        labels = np.ascontiguousarray(labels, dtype=np.uint32)
        rows = None if vertex_rows is None else np.ascontiguousarray(vertex_rows, dtype=np.uint32)
        v0 = np.ascontiguousarray(edge_vertex0, dtype=np.uint32)
        v1 = np.ascontiguousarray(edge_vertex1, dtype=np.uint32)
        handle = P(None)
        rc = self.lib.em2r_cluster_graph_create(_ptr(toc), _ptr(data), gene_count, None if rows is None else _ptr(rows), len(labels),
                                                _ptr(v0), _ptr(v1), len(v0), _ptr(labels), min_cluster_size, k, similarity_threshold,
                                                similarity_threshold_for_merge, stop_after, c.byref(handle))
        if rc == 1:
            raise NanSimilarity("a NaN similarity when makeKnn starts")
        try:
            clusters, tie = c.c_uint32(0), c.c_int(0)
            clustered, unclustered, edges = c.c_uint64(0), c.c_uint64(0), c.c_uint64(0)
            self.lib.em2r_cluster_graph_sizes(handle, c.byref(clusters), c.byref(clustered), c.byref(unclustered), c.byref(edges),
                                              c.byref(tie))
            out = {
                "clusterIds": np.zeros(clusters.value, dtype=np.uint32),
                "cellOffsets": np.zeros(clusters.value + 1, dtype=np.uint64),
                "cells": np.zeros(clustered.value, dtype=np.uint32),
                "unclusteredCells": np.zeros(unclustered.value, dtype=np.uint32),
                "averages": np.zeros((clusters.value, gene_count), dtype=np.float64),
                "edgeCluster0": np.zeros(edges.value, dtype=np.uint32),
                "edgeCluster1": np.zeros(edges.value, dtype=np.uint32),
                "edgeSimilarity": np.zeros(edges.value, dtype=np.float64),
            }
            self.lib.em2r_cluster_graph_get(handle, *[_ptr(out[key]) for key in RESULT_KEYS])
            out["knnTie"] = bool(tie.value)
        finally:
            self.lib.em2r_cluster_graph_free(handle)
        return out

    def sort_by_size(self, sizes, stable):
        sizes = np.ascontiguousarray(sizes, dtype=np.uint32)
        order = np.zeros(len(sizes), dtype=np.uint32)
        self.lib.em2r_sort_by_size(_ptr(sizes), len(sizes), 1 if stable else 0, _ptr(order))
        return order


def load():
    build = os.path.join(NATIVE_DIR, "build")
    os.makedirs(build, exist_ok=True)
    path = os.path.join(build, "libem2clustergraphrestatement.so")
    if not os.path.exists(path) or os.path.getmtime(path) < os.path.getmtime(SOURCE):
        tmp = path + ".%d.tmp" % os.getpid()
        cmd = ["g++", "-std=c++17", "-O2", "-msse4.2", "-ffp-contract=off", "-fPIC", "-shared", "-o", tmp, SOURCE]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError("cluster graph restatement build failed: " + r.stderr)
        os.replace(tmp, path)
    return ClusterGraphRestatement(ctypes.CDLL(path))


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def assert_same_graph(mine, theirs):
    """Every field of a device result equals the restatement's; doubles as bit patterns."""
    for key in RESULT_KEYS:
        a, b = mine[key], theirs[key]
        assert a.shape == b.shape, (key, a.shape, b.shape)
        if a.dtype == np.float64:
            assert np.array_equal(bits(a), bits(b)), key
        else:
            assert np.array_equal(a, b), key


def assert_parity_case(expected):
    """What every parity case must satisfy on the restatement's output: the two unpinned places were not reached."""
    assert not expected["knnTie"], "makeKnn's tie rule decided: choose another input"
    assert not np.isnan(expected["edgeSimilarity"]).any()


# ---- inputs ----

def planted(spec, genes, density, seed, non_integer=False, noise=0.35):
    """Cells around one profile per planted cluster, cluster after cluster -> (toc, data, planted cluster per cell).
    spec: per cluster (size, base, mutate): the cluster's marker genes are those of cluster `base` (itself: a fresh random
    set of about density * genes) with a fraction `mutate` of the genes drawn again -- clusters of one family have similar
    averages.  A cell expresses each marker gene with probability 1 - noise and any other gene with probability
    density * noise, counts 1..8 (times a factor that is no power of two for non_integer)."""
    rows, owner, markers = [], [], []
    gene_ids = np.arange(genes, dtype=np.uint64)
    for cl, (size, base, mutate) in enumerate(spec):
        own = synth.uniform01(seed, 1000 + cl, gene_ids) < density
        if base == cl:
            marker = own
        else:
            marker = np.where(synth.uniform01(seed, 2000 + cl, gene_ids) < mutate, own, markers[base])
        markers.append(marker)
        for i in range(size):
            cell = np.uint64(len(rows))
            u = synth.uniform01(seed, 5, cell * np.uint64(genes) + gene_ids)
            present = np.where(marker, u < 1. - noise, u < density * noise)
            g = np.nonzero(present)[0].astype(np.uint32)
            if len(g) == 0:
                g = np.array([cl % genes], dtype=np.uint32)
            count = 1. + np.floor(8. * synth.uniform01(seed, 6, cell * np.uint64(genes) + g.astype(np.uint64)))
            if non_integer:
                count = count * (0.37 + synth.uniform01(seed, 7, cell * np.uint64(genes) + g.astype(np.uint64)))
            rows.append((g, count.astype(np.float32)))
            owner.append(cl)
    toc = np.zeros(len(rows) + 1, dtype=np.uint64)
    toc[1:] = np.cumsum([len(g) for g, _ in rows])
    data = np.zeros(int(toc[-1]), dtype=COUNT_DTYPE)
    data["gene"] = np.concatenate([g for g, _ in rows])
    data["count"] = np.concatenate([cnt for _, cnt in rows])
    return toc, data, np.array(owner, dtype=np.uint32)


def edges_between(labels, pairs, seed=3):
    """Cell-graph edges that join the given pairs of labels (one or two edges per pair, between arbitrary members) and a
    few edges inside every label."""
    labels = np.asarray(labels)
    members = {}
    for v, label in enumerate(labels.tolist()):
        members.setdefault(label, []).append(v)
    v0, v1 = [], []
    for i, (a, b) in enumerate(pairs):
        ma, mb = members[a], members[b]
        pick = int(synth.hash_u64(seed, np.array([i], dtype=np.uint64))[0])
        v0.append(ma[pick % len(ma)])
        v1.append(mb[(pick >> 20) % len(mb)])
        if i % 2:                                         # a second, parallel connection the other way round
            v0.append(mb[(pick >> 8) % len(mb)])
            v1.append(ma[(pick >> 30) % len(ma)])
    for label, m in members.items():
        for i in range(len(m) - 1):
            v0.append(m[i])
            v1.append(m[i + 1])
    return np.array(v0, dtype=np.uint32), np.array(v1, dtype=np.uint32)


def interleave(labels, seed=11):
    """A permutation of the vertices, so that labels first occur in an order that is not their numeric one and the cell
    lists are not runs of consecutive vertices.  -> order (new vertex v is old cell order[v])."""
    n = len(labels)
    key = synth.hash_u64(seed, np.arange(n, dtype=np.uint64))
    return np.argsort(key, kind="stable").astype(np.uint32)


def wide_range(data, seed=13):
    """The counts times 2^e, e uniform in [-24, 24), per entry.  A sum of float32 values of similar magnitude is exact in
    double, whatever its order; only when a gene is a large part of one cell's vector and a tiny part of another's do the
    additions round, and then their order shows."""
    out = data.copy()
    e = np.floor(48. * synth.uniform01(seed, 31, np.arange(len(data), dtype=np.uint64))) - 24.
    out["count"] = (data["count"].astype(np.float64) * np.exp2(e)).astype(np.float32)
    return out


def shuffled(toc, data, labels, seed=11):
    """The same cells in a hashed order: labels first occur in an order that is not their numeric one, and the vertices
    of a label are not consecutive.  -> (toc, data, labels)."""
    order = interleave(labels, seed)
    toc = np.asarray(toc, dtype=np.uint64)
    lengths = (toc[1:] - toc[:-1])[order]
    out_toc = np.zeros(len(order) + 1, dtype=np.uint64)
    out_toc[1:] = np.cumsum(lengths)
    pieces = [data[int(toc[c]):int(toc[c + 1])] for c in order.tolist()]
    return out_toc, np.concatenate(pieces), np.asarray(labels, dtype=np.uint32)[order]


class Case:
    """The arguments of one cluster_graph_create call."""
    def __init__(self, toc, data, genes, labels, v0, v1, vertex_rows=None, **parameters):
        self.toc, self.data, self.genes, self.labels, self.v0, self.v1, self.vertex_rows = toc, data, genes, labels, v0, v1, vertex_rows
        self.parameters = dict(min_cluster_size=100, k=3, similarity_threshold=0.5, similarity_threshold_for_merge=0.9)
        self.parameters.update(parameters)

    def arguments(self):
        return (self.toc, self.data, self.genes, self.vertex_rows, self.v0, self.v1, self.labels)


def case_merge_split(non_integer=False):
    """Planted cluster 0 carries two labels (70 and 30, alternating cells); clusters 1 and 2 are its relatives.  Edges:
    70-30, 70-label 1, 30-label 2, 1-2.  The merge of 70 and 30 must fire; whichever of the two is removed takes its edge
    along."""
    toc, data, owner = planted([(24, 0, 0.), (14, 0, 0.45), (15, 0, 0.45)], 96, 0.25, seed=21, non_integer=non_integer)
    labels = np.where(owner == 0, np.where(np.arange(len(owner)) % 2 == 0, 70, 30), owner).astype(np.uint32)
    toc, data, labels = shuffled(toc, data, labels, seed=5)
    v0, v1 = edges_between(labels, [(70, 30), (70, 1), (30, 2), (1, 2)])
    return Case(toc, data, 96, labels, v0, v1, min_cluster_size=5, similarity_threshold=0.3, similarity_threshold_for_merge=0.75)


def case_chain3():
    """One planted cluster under three labels joined 8-9 and 9-4 only: one component of three."""
    toc, data, owner = planted([(30, 0, 0.), (12, 0, 0.5)], 80, 0.25, seed=22)
    labels = np.where(owner == 0, np.array([8, 9, 4])[np.arange(len(owner)) % 3], 1).astype(np.uint32)
    toc, data, labels = shuffled(toc, data, labels, seed=6)
    v0, v1 = edges_between(labels, [(8, 9), (9, 4), (4, 1)])
    return Case(toc, data, 80, labels, v0, v1, min_cluster_size=5, similarity_threshold=0.3, similarity_threshold_for_merge=0.65)


def case_small(non_integer=False):
    """Clusters of 3, 1 and 4 cells beside three that stay (minClusterSize 6); one cluster is a single cell."""
    spec = [(12, 0, 0.), (3, 0, 0.5), (10, 0, 0.5), (1, 3, 0.), (4, 0, 0.5), (9, 0, 0.5)]
    toc, data, owner = planted(spec, 72, 0.25, seed=23, non_integer=non_integer)
    labels = (owner + 10).astype(np.uint32)
    toc, data, labels = shuffled(toc, data, labels, seed=7)
    v0, v1 = edges_between(labels, [(10, 11), (10, 12), (12, 13), (12, 15), (14, 15), (10, 15), (11, 13)])
    return Case(toc, data, 72, labels, v0, v1, min_cluster_size=6, similarity_threshold=0.2)


def case_knn():
    """A hub and five relatives, every pair of them joined: with k = 1 makeKnn prunes, and keeps edges through one end."""
    spec = [(14, 0, 0.)] + [(9 + i, 0, 0.2 + 0.08 * i) for i in range(5)]
    toc, data, owner = planted(spec, 120, 0.25, seed=24)
    labels = (owner * 3 + 2).astype(np.uint32)
    toc, data, labels = shuffled(toc, data, labels, seed=8)
    ids = sorted(set(labels.tolist()))
    pairs = [(a, b) for i, a in enumerate(ids) for b in ids[i + 1:]]
    v0, v1 = edges_between(labels, pairs)
    return Case(toc, data, 120, labels, v0, v1, min_cluster_size=5, k=1, similarity_threshold=0.3)


def case_renumber():
    """48 clusters of 3, 4 or 5 cells: most sizes are equal, and above 16 elements std::sort is not stable."""
    sizes = [3 + int(x) for x in (synth.hash_u64(25, np.arange(48, dtype=np.uint64)) % np.uint64(3))]
    spec = [(sizes[0], 0, 0.)] + [(size, 0, 0.3 + 0.01 * (i % 7)) for i, size in enumerate(sizes[1:])]
    toc, data, owner = planted(spec, 64, 0.3, seed=25)
    labels = (owner + 100).astype(np.uint32)
    v0, v1 = edges_between(labels, [(100 + i, 100 + (i * 7 + 1) % 48) for i in range(48) if i != (i * 7 + 1) % 48])
    return Case(toc, data, 64, labels, v0, v1, min_cluster_size=1, similarity_threshold=0.2, similarity_threshold_for_merge=2.)


def case_nan():
    """A cluster whose cells express every gene equally: its average has no variance, its similarities are NaN."""
    toc, data, owner = planted([(8, 0, 0.), (8, 0, 0.4)], 64, 0.25, seed=26)
    flat = np.zeros(6 * 64, dtype=COUNT_DTYPE)
    flat["gene"] = np.tile(np.arange(64, dtype=np.uint32), 6)
    flat["count"] = 1.
    toc = np.concatenate([toc, toc[-1] + np.uint64(64) * np.arange(1, 7, dtype=np.uint64)])
    data = np.concatenate([data, flat])
    labels = np.concatenate([owner, np.full(6, 2, dtype=np.uint32)]).astype(np.uint32)
    v0, v1 = edges_between(labels, [(0, 1), (1, 2), (0, 2)])
    return Case(toc, data, 64, labels, v0, v1, min_cluster_size=5)


def case_wide():
    """case_small with non-integer counts spread over 48 binary orders of magnitude: the additions round."""
    case = case_small(non_integer=True)
    return Case(case.toc, wide_range(case.data), case.genes, case.labels, case.v0, case.v1, min_cluster_size=6,
                similarity_threshold=-1.)


def case_rows(non_integer=True):
    """case_small over a CSR that holds more rows than vertices, in another order (vertex_rows)."""
    case = case_small(non_integer=non_integer)
    n = len(case.labels)
    extra_toc, extra_data, _ = planted([(5, 0, 0.)], case.genes, 0.2, seed=27)
    toc = np.concatenate([extra_toc, extra_toc[-1] + case.toc[1:]])
    data = np.concatenate([extra_data, case.data])
    rows = (5 + np.arange(n)).astype(np.uint32)
    # (the CSR starts with five rows no vertex uses)
    return Case(toc, data, case.genes, case.labels, case.v0, case.v1, vertex_rows=rows, **case.parameters)


SMALL_CASES = {
    "merge_split": case_merge_split,
    "merge_split_non_integer": lambda: case_merge_split(non_integer=True),
    "chain3": case_chain3,
    "small": case_small,
    "small_non_integer": lambda: case_small(non_integer=True),
    "knn": case_knn,
    "renumber": case_renumber,
    "rows": case_rows,
    "wide": case_wide,
}
