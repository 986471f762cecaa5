"""The C++ restatement of ClusterGraph (tests/native/em2_cluster_graph_restatement.cpp) against an independent Python
restatement with explicit sequential loops and float32 / float64 casts, what the arithmetic is NOT, and the hand-made label
cases: merge, chain, small clusters, makeKnn, the unstable renumbering, NaN.  No GPU."""
import numpy as np
import pytest

import cluster_graph_binding as cgb
import fsp0_binding

F32, F64 = np.float32, np.float64


@pytest.fixture(scope="module")
def restatement():
    return cgb.load()


# ---- the independent restatement: src/ExpressionMatrix.cpp:1179-1296, src/regressionCoefficient.cpp:10-42 ----

def py_average(toc, data, genes, cells):
    average = [F64(0.)] * genes
    for cell in cells:
        entries = data[int(toc[cell]):int(toc[cell + 1])]
        total = F64(0.)
        for count in entries["count"]:
            total = total + F64(F32(count) * F32(count))                 # a float product, widened
        factor = F32(F64(1.) / np.sqrt(total))
        for gene, count in zip(entries["gene"].tolist(), entries["count"]):
            average[gene] = average[gene] + F64(F32(count) * factor)
    factor = F64(1.) / F64(len(cells))
    average = [a * factor for a in average]
    total = F64(0.)
    for a in average:
        total = total + a * a
    factor = F64(1.) / np.sqrt(total)
    return np.array([a * factor for a in average], dtype=F64)


def py_similarity(x, y):
    sx = sy = sxx = syy = sxy = F64(0.)
    for a, b in zip(x, y):
        a, b = F64(a), F64(b)
        sx, sy, sxx, syy, sxy = sx + a, sy + b, sxx + a * a, syy + b * b, sxy + a * b
    n = F64(len(x))
    with np.errstate(invalid="ignore", divide="ignore"):
        return (n * sxy - sx * sy) / np.sqrt((n * sxx - sx * sx) * (n * syy - sy * sy))


def py_cluster_graph(case, order_by_size):
    """src/ClusterGraph.cpp:59-386 in plain Python; order_by_size(sizes) -> the positions in std::sort's order.  -> the
    result dict plus 'trace' (what the hand-made cases assert on)."""
    p = case.parameters
    rows = case.vertex_rows if case.vertex_rows is not None else np.arange(len(case.labels))
    vertices, where = [], {}                           # [label, cells, alive]
    for v, label in enumerate(case.labels.tolist()):
        if label not in where:
            where[label] = len(vertices)
            vertices.append([label, [], True])
        vertices[where[label]][1].append(v)
    edges, seen = [], set()                            # [v0, v1, similarity, alive]
    for a, b in zip(case.v0.tolist(), case.v1.tolist()):
        a, b = where[case.labels[a]], where[case.labels[b]]
        if a != b and frozenset((a, b)) not in seen:
            seen.add(frozenset((a, b)))
            edges.append([a, b, None, True])

    def compute():
        average = {i: py_average(case.toc, case.data, case.genes, [int(rows[c]) for c in v[1]]) for i, v in enumerate(vertices) if v[2]}
        for e in edges:
            if e[3]:
                e[2] = py_similarity(average[e[0]], average[e[1]])
        return average

    def drop(i):
        vertices[i][2] = False
        for e in edges:
            if i in (e[0], e[1]):
                e[3] = False

    trace = {}
    compute()
    trace["first"] = [(vertices[e[0]][0], vertices[e[1]][0], e[2]) for e in edges]
    component = list(range(len(vertices)))
    changed = True
    while changed:                                     # the smallest vertex index of the component, by relaxation
        changed = False
        for e in edges:
            if e[2] > p["similarity_threshold_for_merge"]:
                low = min(component[e[0]], component[e[1]])
                if component[e[0]] != low or component[e[1]] != low:
                    component[e[0]] = component[e[1]] = low
                    changed = True
    trace["merged"] = {}
    for i in range(len(vertices)):
        if component[i] != i:
            vertices[component[i]][1].extend(vertices[i][1])
            trace["merged"].setdefault(vertices[component[i]][0], []).append(vertices[i][0])
            drop(i)
    unclustered = []
    for i, v in enumerate(vertices):
        if v[2] and len(v[1]) < p["min_cluster_size"]:
            unclustered.extend(v[1])
            drop(i)
    average = compute()
    for e in edges:
        if e[3] and e[2] < p["similarity_threshold"]:
            e[3] = False
    if any(e[3] and np.isnan(e[2]) for e in edges):
        raise cgb.NanSimilarity("NaN")
    trace["before_knn"] = sum(1 for e in edges if e[3])
    keep, kept_by = set(), {}
    for i, v in enumerate(vertices):
        if not v[2]:
            continue
        mine = sorted(((e[2], j) for j, e in enumerate(edges) if e[3] and i in (e[0], e[1])), reverse=True)
        for _, j in mine[:p["k"]]:
            keep.add(j)
            kept_by.setdefault(j, set()).add(i)
    for j, e in enumerate(edges):
        if e[3] and j not in keep:
            e[3] = False
    trace["kept_through_one_end"] = sum(1 for j in keep if len(kept_by[j]) == 1)
    alive = [i for i, v in enumerate(vertices) if v[2]]
    final = {}
    for new, position in enumerate(order_by_size([len(vertices[i][1]) for i in alive])):
        final[alive[position]] = new
    live = [e for e in edges if e[3]]
    return {
        "clusterIds": np.array([final[i] for i in alive], dtype=np.uint32),
        "cellOffsets": np.cumsum([0] + [len(vertices[i][1]) for i in alive]).astype(np.uint64),
        "cells": np.array([c for i in alive for c in vertices[i][1]], dtype=np.uint32),
        "unclusteredCells": np.array(unclustered, dtype=np.uint32),
        "averages": np.array([average[i] for i in alive], dtype=F64).reshape(len(alive), case.genes),
        "edgeCluster0": np.array([final[e[0]] for e in live], dtype=np.uint32),
        "edgeCluster1": np.array([final[e[1]] for e in live], dtype=np.uint32),
        "edgeSimilarity": np.array([e[2] for e in live], dtype=F64),
        "trace": trace,
    }


def both(restatement, case):
    expected = restatement.create(*case.arguments(), **case.parameters)
    independent = py_cluster_graph(case, lambda sizes: restatement.sort_by_size(sizes, stable=False).tolist())
    cgb.assert_same_graph(expected, independent)
    cgb.assert_parity_case(expected)
    return expected, independent["trace"]


@pytest.mark.parametrize("name", sorted(cgb.SMALL_CASES))
def test_restatement_equals_the_python_restatement(restatement, name):
    both(restatement, cgb.SMALL_CASES[name]())


def test_averages_and_similarities_alone(restatement):
    toc, data = fsp0_binding.clustered(40, 90, 0.1, seed=5, cluster_count=3, non_integer=True)
    cells = np.array([7, 3, 3, 39, 0, 12, 11, 10, 38, 20], dtype=np.uint32)          # not ascending, one cell twice
    offsets = np.array([0, 4, 5, 10], dtype=np.uint64)                               # a cluster of one cell
    averages = restatement.average_expression(toc, data, 90, cells, offsets)
    for c in range(3):
        mine = py_average(toc, data, 90, cells[int(offsets[c]):int(offsets[c + 1])].tolist())
        assert np.array_equal(cgb.bits(averages[c]), cgb.bits(mine))
    similarity = restatement.similarities(averages, [0, 1, 2], [1, 2, 0])
    for e, (a, b) in enumerate([(0, 1), (1, 2), (2, 0)]):
        assert cgb.bits(similarity[e]) == cgb.bits(py_similarity(averages[a], averages[b]))
        assert cgb.bits(similarity[e]) == cgb.bits(py_similarity(averages[b], averages[a]))       # symmetric bit for bit


def test_what_the_average_is_not(restatement):
    """On non-integer counts of widely different magnitude (cgb.wide_range: float32 values of similar magnitude add up
    exactly in double) the order of the double additions shows: numpy's pairwise sum over the cells, and the sum over the
    cells in ascending order where the list is not ascending, differ from the restatement in at least one bit."""
    genes = 150
    toc, data = fsp0_binding.clustered(400, genes, 0.2, seed=9, cluster_count=2, non_integer=True)
    data = cgb.wide_range(data)
    cells = cgb.interleave(np.zeros(400), seed=3)
    offsets = np.array([0, 400], dtype=np.uint64)
    expected = restatement.average_expression(toc, data, genes, cells, offsets)[0]

    def normalized_rows(order):
        dense = np.zeros((len(order), genes), dtype=F64)
        for i, cell in enumerate(order.tolist()):
            entries = data[int(toc[cell]):int(toc[cell + 1])]
            total = F64(0.)
            for count in entries["count"]:
                total = total + F64(F32(count) * F32(count))
            dense[i, entries["gene"]] = (entries["count"] * F32(F64(1.) / np.sqrt(total))).astype(F64)
        return dense

    def finish(sums):
        a = sums * (F64(1.) / F64(400))
        total = F64(0.)
        for x in a:
            total = total + x * x
        return a * (F64(1.) / np.sqrt(total))

    dense = normalized_rows(cells)
    in_order = np.zeros(genes, dtype=F64)
    for row in dense:
        in_order = in_order + row
    assert np.array_equal(cgb.bits(finish(in_order)), cgb.bits(expected))                        # the loop above is the contract
    pairwise = np.sum(np.ascontiguousarray(dense.T), axis=1)                                    # numpy's pairwise summation
    assert not np.array_equal(cgb.bits(finish(pairwise)), cgb.bits(expected))
    ascending = np.zeros(genes, dtype=F64)
    for row in normalized_rows(np.sort(cells)):
        ascending = ascending + row
    assert not np.array_equal(cgb.bits(finish(ascending)), cgb.bits(expected))


def test_merge_of_a_split_cluster(restatement):
    case = cgb.case_merge_split()
    expected, trace = both(restatement, case)
    first = [label for i, label in enumerate(case.labels.tolist()) if label in (70, 30)][0]
    other = 100 - first
    assert trace["merged"] == {first: [other]}
    # the survivor's cells: its own in vertex order, then the other's in vertex order
    own = [v for v, label in enumerate(case.labels.tolist()) if label == first]
    appended = [v for v, label in enumerate(case.labels.tolist()) if label == other]
    survivor = int(np.nonzero(np.diff(expected["cellOffsets"]) == 24)[0][0])
    begin, end = int(expected["cellOffsets"][survivor]), int(expected["cellOffsets"][survivor + 1])
    assert expected["cells"][begin:end].tolist() == own + appended
    assert own + appended != sorted(own + appended)                                   # a list that is not ascending
    # the removed vertex was joined to a third cluster by an edge above the threshold; that edge is lost, not transferred
    partner = {70: 1, 30: 2}[other]
    lost = [s for a, b, s in trace["first"] if {a, b} == {other, partner}]
    assert len(lost) == 1 and lost[0] > case.parameters["similarity_threshold"]
    sizes = np.diff(expected["cellOffsets"]).tolist()
    id_of = dict(zip(sizes, expected["clusterIds"].tolist()))                           # sizes 24, 14, 15 are distinct
    partner_size = {1: 14, 2: 15}[partner]
    edges = {frozenset(e) for e in zip(expected["edgeCluster0"].tolist(), expected["edgeCluster1"].tolist())}
    assert frozenset((id_of[24], id_of[partner_size])) not in edges
    assert len(edges) == 1


def test_chain_of_three_labels_is_one_component(restatement):
    case = cgb.case_chain3()
    expected, trace = both(restatement, case)
    first = case.labels.tolist()[[i for i, label in enumerate(case.labels.tolist()) if label in (8, 9, 4)][0]]
    assert list(trace["merged"]) == [first] and sorted(trace["merged"][first] + [first]) == [4, 8, 9]
    assert sorted(np.diff(expected["cellOffsets"]).tolist()) == [12, 30]
    assert not any(s > case.parameters["similarity_threshold_for_merge"] for a, b, s in trace["first"] if {a, b} == {8, 4})


def test_small_clusters_become_unclustered_cells_in_vertex_order(restatement):
    case = cgb.case_small()
    expected, _ = both(restatement, case)
    labels = case.labels.tolist()
    order = []
    for label in labels:
        if label not in order:
            order.append(label)
    small = [label for label in order if labels.count(label) < 6]
    assert len(small) == 3
    assert expected["unclusteredCells"].tolist() == [v for label in small for v, l in enumerate(labels) if l == label]
    assert len(expected["clusterIds"]) == 3


def test_make_knn_prunes_and_keeps_through_one_end(restatement):
    case = cgb.case_knn()
    expected, trace = both(restatement, case)
    assert trace["before_knn"] > len(expected["edgeSimilarity"]) > 0
    assert trace["kept_through_one_end"] >= 1
    degree = np.bincount(np.concatenate([expected["edgeCluster0"], expected["edgeCluster1"]]))
    assert degree.max() > case.parameters["k"]                                         # a hub keeps edges others chose


def test_renumbering_is_std_sort_not_a_stable_sort(restatement):
    case = cgb.case_renumber()
    expected, _ = both(restatement, case)
    sizes = np.diff(expected["cellOffsets"]).astype(np.uint32)
    assert len(sizes) >= 40
    unstable = restatement.sort_by_size(sizes, stable=False)
    stable = restatement.sort_by_size(sizes, stable=True)
    assert not np.array_equal(unstable, stable)
    final = np.zeros(len(sizes), dtype=np.uint32)
    final[unstable] = np.arange(len(sizes), dtype=np.uint32)
    assert np.array_equal(expected["clusterIds"], final)
    assert np.all(np.diff(sizes[unstable].astype(np.int64)) <= 0)


def test_zero_variance_cluster_is_the_nan_error(restatement):
    case = cgb.case_nan()
    with pytest.raises(cgb.NanSimilarity):
        restatement.create(*case.arguments(), **case.parameters)
    with pytest.raises(cgb.NanSimilarity):
        py_cluster_graph(case, lambda sizes: list(range(len(sizes))))
    first = restatement.create(*case.arguments(), stop_after=1, **case.parameters)
    assert np.isnan(first["edgeSimilarity"]).sum() == 2
