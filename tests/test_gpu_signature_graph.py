"""createSignatureGraph, analyzeLshSignatures and the signature statistics on the GPU (csrc/em2_signature_graph.hip) against
tests/native/em2_signature_graph_restatement.cpp, which tests/test_signature_graph_cpu.py holds against numpy.  Integer work:
every array is compared with np.array_equal, every file byte for byte."""
import os

import numpy as np
import pytest

import signature_graph_binding as sgb
import synth
from expressionmatrix2_amd import ExpressionMatrix, capi, files

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def restatement():
    return sgb.load()


@pytest.mark.parametrize("name,min_cell_count", sgb.GRAPH_CASES)
def test_graph_equals_the_restatement(name, min_cell_count):
    signatures, lsh_count = sgb.case(name)
    theirs = sgb.reference(name, min_cell_count)
    if name == "uniform-20-bits":                            # (the scans of the vertices and of the edges span several blocks)
        assert len(theirs["cellOffsets"]) - 1 > 65536 and len(theirs["edgeVertex0"]) > 65536
    sgb.assert_same_graph(capi.signature_graph_create(signatures, lsh_count, min_cell_count), theirs, "%s, minCellCount %d" % (name, min_cell_count))


def test_filter_removes_the_middle_of_the_path():
    signatures, lsh_count = sgb.case("path-3-1-2")
    graph = capi.signature_graph_create(signatures, lsh_count, 2)
    assert graph["distinctCount"] == 3 and np.diff(graph["cellOffsets"]).tolist() == [3, 2]
    assert graph["vertexSignatures"][:, 0].tolist() == [0, 0b0110 << 60] and graph["cells"].tolist() == [0, 2, 5, 1, 4]
    assert len(graph["edgeVertex0"]) == len(graph["edgeVertex1"]) == 0
    empty = capi.signature_graph_create(signatures, lsh_count, 4)
    assert empty["distinctCount"] == 3 and empty["vertexSignatures"].shape == (0, 1) and empty["cellOffsets"].tolist() == [0]
    assert len(empty["cells"]) == len(empty["edgeVertex0"]) == 0


def test_every_lane_of_the_hypercube_finds_its_neighbour():
    graph = capi.signature_graph_create(*sgb.case("hypercube"))
    assert graph["vertexSignatures"][:, 0].tolist() == [v << 58 for v in range(64)]
    expected = [(v, v | (32 >> bit)) for v in range(64) for bit in range(6) if not v & (32 >> bit)]
    assert list(zip(graph["edgeVertex0"].tolist(), graph["edgeVertex1"].tolist())) == expected and len(expected) == 192


@pytest.mark.parametrize("name,min_cell_count", [("hypercube-200", 0), ("bits-65", 0), ("bits-1024", 0), ("uniform-20-bits", 3)])
def test_device_entry_equals_the_host_entry_and_a_call_repeats_itself(name, min_cell_count):
    signatures, lsh_count = sgb.case(name)
    first = capi.signature_graph_create(signatures, lsh_count, min_cell_count)
    second = capi.signature_graph_create(signatures, lsh_count, min_cell_count)
    device = capi.dev_signature_graph_create(signatures, lsh_count, min_cell_count)
    for key in sgb.GRAPH_KEYS:
        assert first[key].tobytes() == second[key].tobytes() == device[key].tobytes(), key
    sgb.assert_same_graph(device, sgb.reference(name, min_cell_count), name)


def test_a_bit_behind_lsh_count_is_an_error():
    signatures = sgb.of_integers([1, 2, 3], 8).copy()
    signatures[1, 0] |= np.uint64(1 << 55)
    with pytest.raises(RuntimeError, match="^em2_signature_graph_create: a signature has a bit set at or beyond lshCount$"):
        capi.signature_graph_create(signatures, 8)
    wide = np.zeros((3, 2), dtype=np.uint64)
    wide[2, 1] = 1 << 62
    with pytest.raises(RuntimeError, match="a signature has a bit set at or beyond lshCount"):
        capi.signature_graph_create(wide, 65)
    wide[2, 1] = 1 << 63
    assert capi.signature_graph_create(wide, 65)["distinctCount"] == 2


@pytest.mark.parametrize("cell_count", [1, 63, 65, 100000])
@pytest.mark.parametrize("lsh_count", [1, 64, 65, 1024])
def test_statistics(restatement, lsh_count, cell_count):
    rng = np.random.default_rng(lsh_count * 1000003 + cell_count)
    bits = rng.integers(0, 2, (cell_count, lsh_count), dtype=np.uint8)
    bits[:, lsh_count - 1] = 1                               # one bit set in every cell
    if lsh_count > 1:
        bits[:, lsh_count // 2] = 0                          # and one in none
    signatures = sgb.pack_bits(bits)
    expected = bits.sum(axis=0, dtype=np.uint64)
    assert np.array_equal(restatement.signature_statistics(signatures, lsh_count)[0], expected)
    assert np.array_equal(capi.lsh_signature_statistics(signatures, lsh_count), expected)


def test_statistics_take_device_signatures():
    import torch
    signatures, lsh_count = sgb.case("bits-128")
    d_signatures = torch.from_numpy(signatures.view(np.int64).copy()).to("cuda")
    torch.cuda.synchronize()
    counts = np.zeros(lsh_count, dtype=np.uint64)
    capi.check(capi.load().em2_dev_lsh_signature_statistics(d_signatures.data_ptr(), len(signatures), lsh_count, capi._ptr(counts)))
    assert np.array_equal(counts, capi.lsh_signature_statistics(signatures, lsh_count))


@pytest.mark.parametrize("name", sgb.ANALYZE_CASES)
def test_analyze_writes_the_restatements_files(restatement, tmp_path, name):
    signatures, lsh_count = sgb.case(name)
    mine, theirs = tmp_path / "mine", tmp_path / "theirs"
    mine.mkdir()
    theirs.mkdir()
    restatement.analyze_lsh_signatures(signatures, lsh_count, str(theirs))
    capi.analyze_lsh_signatures(signatures, lsh_count, str(mine))
    assert sgb.read_files(str(mine)) == sgb.read_files(str(theirs))


# ---- the facade ----

@pytest.fixture(scope="module")
def matrix(tmp_path_factory):
    cells, genes = 600, 200
    toc, g, c = synth.expression_matrix(cells, genes, density=0.1, cluster_count=4, seed=11)
    directory = str(tmp_path_factory.mktemp("signature_graph") / "data")
    files.create_directory(directory, genes, toc, capi.make_counts(g, c))
    files.add_cell_set(directory, "Odd", np.arange(1, cells, 2, dtype=np.uint32))
    files.add_cell_set(directory, "Nobody", np.zeros(0, dtype=np.uint32))
    files.add_gene_set(directory, "NoGenes", np.zeros(0, dtype=np.uint32))
    e = ExpressionMatrix(directory)
    e.computeLshSignatures(lshName="All12", lshCount=12)
    e.computeLshSignatures(cellSetName="Odd", lshName="Odd12", lshCount=12)
    yield e, directory
    e.close()


@pytest.mark.parametrize("cell_set,lsh_name,min_cell_count", [("AllCells", "All12", 1), ("Odd", "Odd12", 1), ("Odd", "Odd12", 3)])
def test_facade_graph(restatement, matrix, cell_set, lsh_name, min_cell_count):
    e, directory = matrix
    lsh_count, signatures = files.read_lsh(directory, lsh_name)
    assert lsh_count == 12
    theirs = restatement.signature_graph(signatures, lsh_count, min_cell_count)
    name = "%s-%d" % (lsh_name, min_cell_count)
    e.createSignatureGraph(signatureGraphName=name, cellSetName=cell_set, lshName=lsh_name, minCellCount=min_cell_count)
    assert name in e.getSignatureGraphNames()
    vertex_signatures, cell_counts = e.getSignatureGraphVertices(name)
    assert np.array_equal(vertex_signatures, theirs["vertexSignatures"]) and np.array_equal(cell_counts, np.diff(theirs["cellOffsets"]))
    assert len(cell_counts) > 1 and len(theirs["edgeVertex0"]) > 0
    cell_ids = np.arange(600, dtype=np.uint32) if cell_set == "AllCells" else np.arange(1, 600, 2, dtype=np.uint32)
    for v in range(len(cell_counts)):
        local, global_ids = e.getSignatureGraphCells(name, v)
        expected = theirs["cells"][int(theirs["cellOffsets"][v]):int(theirs["cellOffsets"][v + 1])]
        assert np.array_equal(local, expected) and np.array_equal(global_ids, cell_ids[expected])
    v0, v1 = e.getSignatureGraphEdges(name)
    assert np.array_equal(v0, theirs["edgeVertex0"]) and np.array_equal(v1, theirs["edgeVertex1"])
    e.removeSignatureGraph(name)
    assert name not in e.getSignatureGraphNames()


def test_facade_errors(matrix):
    e, _ = matrix
    e.createSignatureGraph(signatureGraphName="Twice", lshName="All12", minCellCount=1)
    for arguments, text in [
            (dict(signatureGraphName="Twice", lshName="All12", minCellCount=1), "Signature graph Twice already exists."),
            (dict(signatureGraphName="G", cellSetName="Missing", lshName="All12", minCellCount=1), "Cell set Missing does not exist."),
            (dict(signatureGraphName="G", cellSetName="Nobody", lshName="All12", minCellCount=1), "Cell set Nobody is empty."),
            (dict(signatureGraphName="G", cellSetName="Odd", lshName="All12", minCellCount=1),
             "LSH object All12 has a number of cells inconsistent with cell set Odd.")]:
        with pytest.raises(RuntimeError) as error:
            e.createSignatureGraph(**arguments)
        assert str(error.value) == text
    assert e.getSignatureGraphNames() == ["Twice"]
    e.removeSignatureGraph("Twice")
    for call in (lambda: e.removeSignatureGraph("Twice"), lambda: e.getSignatureGraphVertices("Twice"),
                 lambda: e.getSignatureGraphCells("Twice", 0), lambda: e.getSignatureGraphEdges("Twice")):
        with pytest.raises(RuntimeError) as error:
            call()
        assert str(error.value) == "Signature graph Twice does not exists."
    for arguments, text in [(dict(geneSetName="Missing"), "Gene set Missing does not exist."),
                            (dict(geneSetName="NoGenes"), "Gene set NoGenes is empty."),
                            (dict(cellSetName="Missing"), "Cell set Missing does not exist."),
                            (dict(cellSetName="Nobody"), "Cell set Nobody is empty.")]:
        with pytest.raises(RuntimeError) as error:
            e.analyzeLshSignatures(**arguments)
        assert str(error.value) == text


def test_facade_analyze_lsh_signatures(matrix, tmp_path, monkeypatch):
    e, directory = matrix
    e.computeLshSignatures(cellSetName="Odd", lshName="Odd70", lshCount=70, seed=7)
    lsh_count, signatures = files.read_lsh(directory, "Odd70")
    expected = tmp_path / "expected"
    working = tmp_path / "working"
    expected.mkdir()
    working.mkdir()
    capi.analyze_lsh_signatures(signatures, lsh_count, str(expected))
    monkeypatch.chdir(working)
    e.analyzeLshSignatures(cellSetName="Odd", lshCount=70, seed=7)
    assert sgb.read_files(str(working)) == sgb.read_files(str(expected))
    assert not [name for name in os.listdir(directory) if name.startswith("tmp-")]
