"""The yardstick of the signature graph tests, without a GPU: tests/native/em2_signature_graph_restatement.cpp (std::map,
map::find per zero bit, std::sort) against an independent numpy statement on every shared case, its three CSV texts on a
hand-written example, and the argument checks of the library's entries, none of which reaches a device."""
import ctypes

import numpy as np
import pytest

import signature_graph_binding as sgb
from expressionmatrix2_amd import capi

OK, INVALID, NO_DEVICE, UNSUPPORTED = 0, 1, 2, 6


@pytest.fixture(scope="module")
def restatement():
    return sgb.load()


def numpy_graph(signatures, lsh_count, min_cell_count):
    """Groups: np.unique over the rows as big-endian bytes (byte order = word order = the map's order).  Edges: a membership
    test per (vertex, zero bit) -- a searchsorted per bit for one word, a dict of Python integers for more."""
    cells, words = signatures.shape
    as_bytes = signatures.astype(">u8").view(np.uint8).reshape(cells, words * 8)
    rows, inverse, counts = np.unique(as_bytes, axis=0, return_inverse=True, return_counts=True)
    inverse = inverse.reshape(-1)
    keep = counts >= min_cell_count
    vertex_of_group = np.cumsum(keep) - 1
    order = np.argsort(inverse, kind="stable")                  # cells by group, ascending within a group
    order = order[keep[inverse[order]]]
    vertex_signatures = np.ascontiguousarray(rows[keep]).view(">u8").astype(np.uint64).reshape(-1, words)
    offsets = np.concatenate([[0], np.cumsum(counts[keep])]).astype(np.uint64)
    vertices = len(vertex_signatures)
    if words == 1:
        keys = vertex_signatures[:, 0]
        found = []
        for bit in range(lsh_count):
            mask = np.uint64(1 << (63 - bit))
            v0 = np.nonzero((keys & mask) == 0)[0]
            wanted = keys[v0] | mask
            at = np.searchsorted(keys, wanted)
            hit = (at < vertices) & (keys[np.minimum(at, max(vertices - 1, 0))] == wanted) if vertices else np.zeros(0, bool)
            found.append(np.stack([v0[hit], np.full(hit.sum(), bit), at[hit]], axis=1))
        found = np.concatenate(found) if found else np.zeros((0, 3), np.int64)
        found = found[np.lexsort((found[:, 1], found[:, 0]))]
        e0, e1 = found[:, 0], found[:, 2]
    else:
        total = words * 64
        values = [int.from_bytes(rows[keep][v].tobytes(), "big") for v in range(vertices)]
        vertex_of = {value: v for v, value in enumerate(values)}
        e0, e1 = [], []
        for v0, value in enumerate(values):
            for bit in range(lsh_count):
                mask = 1 << (total - 1 - bit)
                if not value & mask and (value | mask) in vertex_of:
                    e0.append(v0)
                    e1.append(vertex_of[value | mask])
    assert vertex_of_group[keep].tolist() == list(range(vertices))
    return {"distinctCount": len(rows), "vertexSignatures": vertex_signatures, "cellOffsets": offsets,
            "cells": order.astype(np.uint32), "edgeVertex0": np.asarray(e0, dtype=np.uint32), "edgeVertex1": np.asarray(e1, dtype=np.uint32)}


@pytest.mark.parametrize("name,min_cell_count", sgb.GRAPH_CASES)
def test_restatement_agrees_with_numpy(name, min_cell_count):
    signatures, lsh_count = sgb.case(name)
    theirs = sgb.reference(name, min_cell_count)
    sgb.assert_same_graph(numpy_graph(signatures, lsh_count, min_cell_count), theirs, name)
    assert np.all(theirs["edgeVertex1"] > theirs["edgeVertex0"])


def test_the_cases_are_what_they_are_meant_to_be():
    assert sgb.reference("one-cell-one-bit", 0)["cells"].tolist() == [0]
    both = sgb.reference("one-bit-both", 0)
    assert (len(both["cellOffsets"]) - 1, both["edgeVertex0"].tolist(), both["edgeVertex1"].tolist()) == (2, [0], [1])
    cube = sgb.reference("hypercube", 0)
    assert len(cube["cellOffsets"]) - 1 == 64 and len(cube["edgeVertex0"]) == 6 * 32
    assert np.diff(sgb.reference("hypercube-200", 0)["cellOffsets"]).max() > 1
    for name, bits in (("bits-63", (0, 62)), ("bits-64", (0, 63)), ("bits-65", (0, 63, 64)), ("bits-128", (0, 63, 64, 127)),
                       ("bits-1024", (0, 63, 64, 511, 1023))):
        graph = sgb.reference(name, 0)
        assert len(graph["edgeVertex0"]) == len(bits), name           # random keys never neighbour: the planted ones only
        differing = graph["vertexSignatures"][graph["edgeVertex0"]] ^ graph["vertexSignatures"][graph["edgeVertex1"]]
        found = sorted(64 * w + 63 - int(word).bit_length() + 1 for row in differing for w, word in enumerate(row) if word)
        assert found == sorted(bits), name
    whole = sgb.reference("one-group-70000", 0)
    assert np.array_equal(whole["cells"], np.arange(70000)) and whole["cellOffsets"].tolist() == [0, 70000]
    many = sgb.reference("uniform-20-bits", 0)
    assert len(many["cellOffsets"]) - 1 > 65536 and len(many["edgeVertex0"]) > 65536
    sizes = np.diff(sgb.reference("sizes-1-2-3", 0)["cellOffsets"])
    assert len(sizes) == 100 and set(sizes.tolist()) == {1, 2, 3} and min(np.bincount(sizes.astype(np.int64))[1:]) > 16


def test_the_filter_on_the_path():
    """0000 x 3 -- 0100 x 1 -- 0110 x 2."""
    everything = sgb.reference("path-3-1-2", 0)
    assert np.diff(everything["cellOffsets"]).tolist() == [3, 1, 2]
    assert (everything["edgeVertex0"].tolist(), everything["edgeVertex1"].tolist()) == ([0, 1], [1, 2])
    sgb.assert_same_graph(sgb.reference("path-3-1-2", 1), everything, "minCellCount 1")
    two = sgb.reference("path-3-1-2", 2)                                  # the middle vertex and both its edges go
    assert two["distinctCount"] == 3 and np.diff(two["cellOffsets"]).tolist() == [3, 2] and len(two["edgeVertex0"]) == 0
    assert two["vertexSignatures"][:, 0].tolist() == [0, 0b0110 << 60] and two["cells"].tolist() == [0, 2, 5, 1, 4]
    none = sgb.reference("path-3-1-2", 4)
    assert none["distinctCount"] == 3 and none["cellOffsets"].tolist() == [0] and len(none["cells"]) == len(none["edgeVertex0"]) == 0


def test_csv_texts_of_a_hand_written_example(restatement, tmp_path):
    # five cells, three bits: x_x twice, __x twice, xxx once
    signatures = sgb.of_integers([0b101, 0b001, 0b111, 0b001, 0b101], 3)
    restatement.analyze_lsh_signatures(signatures, 3, str(tmp_path))
    files = sgb.read_files(str(tmp_path))
    assert files["Signatures.csv"] == b"__x,2\nx_x,2\nxxx,1\n"             # (three elements: std::sort is an insertion sort, stable)
    assert files["Histogram.csv"] == b"1,1,1,1\n2,2,4,5\n"
    assert files["LshSignatureStatistics.csv"] == b"Bit,Set,Unset,Total\n0,3,2,5\n1,1,4,5\n2,5,0,5\n"


@pytest.mark.parametrize("name", sgb.ANALYZE_CASES)
def test_csv_texts_agree_with_numpy(restatement, tmp_path, name):
    """Everything but the order of equal sizes in Signatures.csv, which is std::sort's."""
    signatures, lsh_count = sgb.case(name)
    restatement.analyze_lsh_signatures(signatures, lsh_count, str(tmp_path))
    files = sgb.read_files(str(tmp_path))
    graph = numpy_graph(signatures, lsh_count, 0)
    sizes = np.diff(graph["cellOffsets"]).astype(np.int64)
    lines = [line.split(",") for line in files["Signatures.csv"].decode().splitlines()]
    assert [int(size) for _, size in lines] == sorted(sizes.tolist(), reverse=True)
    text = ["".join("x" if (int(row[i >> 6]) >> (63 - (i & 63))) & 1 else "_" for i in range(lsh_count)) for row in graph["vertexSignatures"]]
    assert sorted((t, str(s)) for t, s in zip(text, sizes.tolist())) == sorted((t, s) for t, s in lines)
    frequency = np.bincount(sizes)
    running, expected = 0, ""
    for size in np.nonzero(frequency)[0]:
        running += int(size * frequency[size])
        expected += "%d,%d,%d,%d\n" % (size, frequency[size], size * frequency[size], running)
    assert files["Histogram.csv"].decode() == expected
    bits = np.unpackbits(signatures.astype(">u8").view(np.uint8).reshape(len(signatures), -1), axis=1)[:, :lsh_count]
    set_count = bits.sum(axis=0)
    assert np.array_equal(restatement.signature_statistics(signatures, lsh_count)[0], set_count.astype(np.uint64))
    expected = "Bit,Set,Unset,Total\n" + "".join("%d,%d,%d,%d\n" % (i, s, len(signatures) - s, len(signatures)) for i, s in enumerate(set_count))
    assert files["LshSignatureStatistics.csv"].decode() == expected


# ---- the library's argument checks: return code and the whole text; nothing here reaches a device ----

SIG = np.zeros((6, 2), dtype=np.uint64)
COUNTS = np.zeros(128, dtype=np.uint64)


def _call(name, *arguments):
    lib = capi.load()
    rc = getattr(lib, name)(*arguments)
    return rc, lib.em2_last_error().decode()


def _entries():
    """name -> the call with (signatures, cellCount, lshCount)."""
    handle = ctypes.c_void_p(None)
    return {
        "em2_signature_graph_create": lambda s, n, L: _call("em2_signature_graph_create", s, n, L, 0, ctypes.byref(handle)),
        "em2_dev_signature_graph_create": lambda s, n, L: _call("em2_dev_signature_graph_create", s, n, L, 0, ctypes.byref(handle)),
        "em2_lsh_signature_statistics": lambda s, n, L: _call("em2_lsh_signature_statistics", s, n, L, COUNTS.ctypes.data),
        "em2_dev_lsh_signature_statistics": lambda s, n, L: _call("em2_dev_lsh_signature_statistics", s, n, L, COUNTS.ctypes.data),
        "em2_analyze_lsh_signatures": lambda s, n, L: _call("em2_analyze_lsh_signatures", s, n, L, None),
    }


@pytest.mark.parametrize("name", sorted(_entries()))
def test_entry_argument_errors(name):
    call = _entries()[name]
    assert call(SIG.ctypes.data, 6, 0) == (INVALID, name + ": lshCount must be positive")
    assert call(SIG.ctypes.data, 6, 65537) == (UNSUPPORTED, name + ": lshCount above 65536 is not supported")
    assert call(SIG.ctypes.data, 0, 128) == (INVALID, name + ": cellCount must be positive")
    assert call(None, 6, 128) == (INVALID, name + ": null pointer")
    assert call(None, 0, 0) == (INVALID, name + ": lshCount must be positive")       # (the order: lshCount, cellCount, pointers)
    if capi.device_count() == 0:
        assert call(SIG.ctypes.data, 6, 128) == (NO_DEVICE, name + ": no HIP device is visible (this library has no CPU path)")


def test_null_results_and_handles():
    assert _call("em2_signature_graph_create", SIG.ctypes.data, 6, 128, 0, None) == (INVALID, "em2_signature_graph_create: null pointer")
    for name in ("em2_lsh_signature_statistics", "em2_dev_lsh_signature_statistics"):
        assert _call(name, SIG.ctypes.data, 6, 128, None) == (INVALID, name + ": null pointer")
    assert _call("em2_signature_graph_sizes", None, None, None, None, None, None) == (INVALID, "em2_signature_graph_sizes: null pointer")
    assert _call("em2_signature_graph_get", None, None, None, None, None, None) == (INVALID, "em2_signature_graph_get: null pointer")
    capi.load().em2_signature_graph_free(None)


def test_facade_arguments_and_names(tmp_path):
    """What the facade decides without the library: the required arguments and the names of graphs that do not exist."""
    import synth
    from expressionmatrix2_amd import ExpressionMatrix, files
    toc, genes, counts = synth.expression_matrix(20, 30, density=0.2, cluster_count=2, seed=3)
    directory = str(tmp_path / "data")
    files.create_directory(directory, 30, toc, capi.make_counts(genes, counts))
    files.add_gene_set(directory, "NoGenes", np.zeros(0, dtype=np.uint32))
    files.add_cell_set(directory, "NoCells", np.zeros(0, dtype=np.uint32))
    e = ExpressionMatrix(directory)
    with pytest.raises(TypeError, match="signatureGraphName, lshName and minCellCount are required"):
        e.createSignatureGraph(signatureGraphName="G", lshName="L")
    with pytest.raises(RuntimeError, match=r"^Signature graph G does not exists\.$"):
        e.removeSignatureGraph("G")
    with pytest.raises(RuntimeError, match=r"^Signature graph G does not exists\.$"):
        e.getSignatureGraphEdges("G")
    assert e.getSignatureGraphNames() == []
    with pytest.raises(RuntimeError, match=r"^Cell set Nobody does not exist\.$"):
        e.createSignatureGraph(signatureGraphName="G", cellSetName="Nobody", lshName="L", minCellCount=1)
    with pytest.raises(RuntimeError, match=r"^Gene set Nothing does not exist\.$"):
        e.analyzeLshSignatures(geneSetName="Nothing")
    with pytest.raises(RuntimeError, match=r"^Cell set Nobody does not exist\.$"):
        e.analyzeLshSignatures(cellSetName="Nobody")
    with pytest.raises(RuntimeError, match=r"^Gene set NoGenes is empty\.$"):
        e.analyzeLshSignatures(geneSetName="NoGenes")
    with pytest.raises(RuntimeError, match=r"^Gene set NoGenes is empty\.$"):             # the gene set comes first (:1379-1398)
        e.analyzeLshSignatures(geneSetName="NoGenes", cellSetName="NoCells")
    with pytest.raises(RuntimeError, match=r"^Cell set NoCells is empty\.$"):
        e.analyzeLshSignatures(cellSetName="NoCells")
    with pytest.raises(RuntimeError, match=r"^Cell set NoCells is empty\.$"):
        e.createSignatureGraph(signatureGraphName="G", cellSetName="NoCells", lshName="L", minCellCount=1)
    for bad in (-1, 2 ** 64, 1.5):                       # a size_t in the reference: nothing wraps around on the way there
        with pytest.raises(ValueError, match="minCellCount must be an integer"):
            e.createSignatureGraph(signatureGraphName="G", lshName="L", minCellCount=bad)
    e.close()
