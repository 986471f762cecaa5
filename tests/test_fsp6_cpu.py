"""findSimilarPairs6 without a GPU: the facade and the C ABI exist, the reference's errors come in its order and with its
texts (src/ExpressionMatrixLsh.cpp:859-893), the documented decisions (permutedBitCount 0, the kernels' limits) hold, and the
host entry reports the missing device.  Then the C++ restatement (tests/native/em2_fsp6_restatement.cpp) on cases small
enough to check by hand."""
import ctypes

import numpy as np
import pytest

import fsp6_binding
import synth
from expressionmatrix2_amd import ExpressionMatrix, capi, files

EM2_ERROR_INVALID_ARGUMENT = 1
EM2_ERROR_RUNTIME = 5


@pytest.fixture(scope="module")
def restatement():
    return fsp6_binding.load()


@pytest.fixture()
def matrix(tmp_path):
    d = str(tmp_path / "data")
    toc, g, c = synth.expression_matrix(40, 30, density=0.2, cluster_count=3, seed=5)
    files.create_directory(d, 30, toc, capi.make_counts(g, c))
    files.write_lsh(d, "L", 128, synth.random_signatures(40, 128))
    files.write_lsh(d, "Short", 128, synth.random_signatures(39, 128))
    files.add_gene_set(d, "NoGenes", np.zeros(0, dtype=np.uint32))
    files.add_cell_set(d, "NoCells", np.zeros(0, dtype=np.uint32))
    return d


def test_facade_and_abi_exist():
    lib = capi.load()
    for name in ("em2_find_similar_pairs6", "em2_dev_find_similar_pairs6", "em2_matrix_find_similar_pairs6"):
        assert hasattr(lib, name)
    assert lib.em2_abi_version() == 1
    assert callable(ExpressionMatrix.findSimilarPairs6)


def test_facade_required_arguments(matrix):
    e = ExpressionMatrix(matrix)
    with pytest.raises(TypeError):
        e.findSimilarPairs6(lshName="L", similarPairsName="P", permutationCount=4)
    with pytest.raises(TypeError):
        e.findSimilarPairs6(similarPairsName="P", permutationCount=4, searchCount=10)


def test_facade_errors_in_reference_order(matrix):
    e = ExpressionMatrix(matrix)
    with pytest.raises(RuntimeError, match="Gene set Nope does not exist."):
        e.findSimilarPairs6(geneSetName="Nope", lshName="L", similarPairsName="P", permutationCount=4, searchCount=10,
                            permutedBitCount=1000)
    with pytest.raises(RuntimeError, match="Gene set NoGenes is empty."):
        e.findSimilarPairs6(geneSetName="NoGenes", lshName="L", similarPairsName="P", permutationCount=4, searchCount=10)
    with pytest.raises(RuntimeError, match="Cell set Nope does not exist."):
        e.findSimilarPairs6(cellSetName="Nope", lshName="L", similarPairsName="P", permutationCount=4, searchCount=10)
    with pytest.raises(RuntimeError, match="Cell set NoCells is empty."):
        e.findSimilarPairs6(cellSetName="NoCells", lshName="L", similarPairsName="P", permutationCount=4, searchCount=10)
    with pytest.raises(RuntimeError, match="LSH object Short has a number of cells inconsistent with cell set AllCells"):
        e.findSimilarPairs6(lshName="Short", similarPairsName="P", permutationCount=4, searchCount=10, permutedBitCount=1000)
    with pytest.raises(RuntimeError, match="^Argument permutationStoreBitCount 129 exceeds number of signature bits 128$"):
        e.findSimilarPairs6(lshName="L", similarPairsName="P", permutationCount=4, searchCount=10, permutedBitCount=129)
    with pytest.raises(RuntimeError, match="permutedBitCount must be positive"):
        e.findSimilarPairs6(lshName="L", similarPairsName="P", permutationCount=4, searchCount=10, permutedBitCount=0)


def _host_call(sig, L, k=5, thr=0.2, P=4, S=10, pbits=64, seed=231):
    sig = np.ascontiguousarray(sig, dtype=np.uint64)
    n = sig.shape[0]
    pairs = np.zeros((n, max(k, 1)), dtype=capi.PAIR_DTYPE)
    used = np.zeros(n, dtype=np.uint32)
    lib = capi.load()
    rc = lib.em2_find_similar_pairs6(capi._ptr(sig), n, L, k, thr, P, S, pbits, seed, capi._ptr(pairs), capi._ptr(used))
    return rc, lib.em2_last_error().decode()


def test_abi_argument_errors_before_the_device():
    sig = synth.random_signatures(200, 128)
    assert _host_call(sig, 128, pbits=200) == (EM2_ERROR_RUNTIME,
                                              "Argument permutationStoreBitCount 200 exceeds number of signature bits 128")
    rc, message = _host_call(sig, 128, pbits=0)
    assert rc == EM2_ERROR_INVALID_ARGUMENT and "permutedBitCount" in message
    rc, message = _host_call(sig, 128, P=65)
    assert rc == capi.EM2_ERROR_UNSUPPORTED and "permutationCount above 64" in message
    rc, message = _host_call(sig, 128, P=64, S=9000)
    assert rc == capi.EM2_ERROR_UNSUPPORTED and "8192" in message
    # what the queues can hold caps searchCount: 2 permutations x 199 other cells
    rc, _ = _host_call(sig, 128, P=2, S=10**9)
    assert rc != capi.EM2_ERROR_UNSUPPORTED
    rc, message = _host_call(sig, 0)
    assert rc == EM2_ERROR_INVALID_ARGUMENT


def test_host_entry_without_device():
    if capi.device_count() > 0:
        pytest.skip("a GPU is visible: the no-device answer cannot be observed here")
    rc, message = _host_call(synth.random_signatures(20, 64), 64)
    assert rc == capi.EM2_ERROR_NO_DEVICE and "no HIP device" in message


def test_restatement_rejects_like_the_reference(restatement):
    sig = synth.random_signatures(5, 64)
    with pytest.raises(ValueError, match="1"):
        restatement.find_similar_pairs6(sig, 64, 3, 0.2, 2, 10, permuted_bit_count=65)
    with pytest.raises(ValueError, match="2"):
        restatement.find_similar_pairs6(sig, 64, 3, 0.2, 2, 10, permuted_bit_count=0)


def test_restatement_permutations_are_one_generator(restatement):
    """One std::mt19937 for all permutations; permutedBitCount truncates without changing the draws; the int seed wraps."""
    long = restatement.permutations(100, 3, 100, 231)
    short = restatement.permutations(100, 3, 7, 231)
    assert np.array_equal(long[:, :7], short)
    assert all(sorted(row) == list(range(100)) for row in long)
    assert not np.array_equal(long[0], long[1])
    assert np.array_equal(restatement.permutations(64, 2, 64, -3), restatement.permutations(64, 2, 64, -3))
    assert not np.array_equal(restatement.permutations(64, 2, 64, -3), restatement.permutations(64, 2, 64, 3))


def test_restatement_one_cell(restatement):
    cell, sim, used = restatement.find_similar_pairs6(synth.random_signatures(1, 64), 64, 3, -1.0, 4, 10)
    assert used.tolist() == [0]


def test_restatement_two_cells_quirk(restatement):
    """Sorted positions 0 and 1: the cell at 0 has a forward pointer; the cell at 1 would need a backward one, which the
    reference only starts from position 2 (:1031) -- so exactly one of the two cells finds the other."""
    sig = np.array([[0x8000000000000000], [0]], dtype=np.uint64)       # cell 1 sorts first in every permutation
    cell, sim, used = restatement.find_similar_pairs6(sig, 64, 3, -1.0, 3, 10)
    assert used.tolist() == [0, 1]
    assert cell[1, 0] == 0 and sim[1, 0] == np.float32(np.cos(np.pi / 64))


def test_restatement_three_cells(restatement):
    """Three identical cells sort by id; position 1 (cell 1) looks forward only, position 2 (cell 2) backward to 1 and 0."""
    sig = np.zeros((3, 1), dtype=np.uint64)
    cell, sim, used = restatement.find_similar_pairs6(sig, 64, 3, 0.2, 1, 10)
    assert used.tolist() == [2, 1, 2]
    assert cell[0, :2].tolist() == [1, 2] and cell[1, 0] == 2 and cell[2, :2].tolist() == [0, 1]
    assert (sim[used > 0, 0] == np.float32(1.0)).all()


def test_restatement_nothing_to_search(restatement):
    sig = synth.clustered_signatures(30, 128, cluster_count=2, flip=0.05, seed=1)
    for P, S in ((0, 50), (4, 0)):
        cell, sim, used = restatement.find_similar_pairs6(sig, 128, 5, -1.0, P, S)
        assert used.sum() == 0 and (cell == 0).all() and (sim == 0).all()


def test_restatement_search_beyond_the_queue(restatement):
    """searchCount above what the queues hold (every pointer walks to its end): every other cell is found, once."""
    n, P = 12, 3
    sig = synth.clustered_signatures(n, 64, cluster_count=2, flip=0.2, seed=2)
    cell, sim, used = restatement.find_similar_pairs6(sig, 64, n, -1.0, P, 2 * P * n + 5)
    for c in range(n):
        found = cell[c, :used[c]].tolist()
        assert len(found) == len(set(found)) and c not in found
    # the queues were empty before searchCount ran out: a larger one changes nothing
    again = restatement.find_similar_pairs6(sig, 64, n, -1.0, P, 10**6)
    assert np.array_equal(again[0], cell) and np.array_equal(again[2], used)


def test_restatement_rows_subset(restatement):
    sig = synth.clustered_signatures(80, 128, cluster_count=4, flip=0.1, seed=3)
    full = restatement.find_similar_pairs6(sig, 128, 6, 0.2, 5, 40, 64, 9)
    rows = np.array([79, 0, 33], dtype=np.uint32)
    part = restatement.find_similar_pairs6(sig, 128, 6, 0.2, 5, 40, 64, 9, rows=rows)
    for got, want in zip(part, full):
        assert np.array_equal(got, want[rows])
