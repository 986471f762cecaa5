"""GPU parity of findSimilarPairs6 (the Charikar permutation search, src/ExpressionMatrixLsh.cpp:842-1145) through the C ABI
and the facade against the literal C++ restatement (tests/native/em2_fsp6_restatement.cpp, built with this box's
libstdc++).  Bit-exact: cell ids, float similarity bit patterns, usedCount."""
import os

import numpy as np
import pytest

import fsp6_binding
import synth
from expressionmatrix2_amd import ExpressionMatrix, capi, files

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def restatement():
    return fsp6_binding.load()


def assert_same(pairs, gused, cell, sim, used):
    assert np.array_equal(gused, used)
    assert np.array_equal(pairs["cell"], cell)
    assert np.array_equal(pairs["similarity"].view(np.uint32), sim.view(np.uint32))


@pytest.mark.parametrize("n,L,k,thr,P,S,pbits,seed", [
    (300, 128, 5, 0.2, 4, 50, 64, 231),
    (1000, 1024, 20, 0.2, 16, 200, 64, 231),
    (500, 256, 10, 0.0, 8, 100, 128, 7),
    (400, 100, 4, 0.1, 6, 64, 100, 5),           # L not a multiple of 64: padding in the second prefix word
    (700, 192, 8, 0.2, 5, 300, 65, -3),          # a second word with one live bit; a negative seed
    (257, 64, 70, -0.9, 3, 1000, 1, 231),        # 1-bit prefixes: ties everywhere; k above the neighbours
    (350, 256, 6, 1.0, 6, 80, 64, 231),          # nothing passes
    (350, 256, 0, 0.2, 6, 80, 64, 231),          # k = 0
    (600, 512, 12, 0.3, 64, 128, 200, 42),       # the largest permutation count; four prefix words
    (120, 64, 30, 0.0, 2, 5000, 16, 1),          # searchCount above what the queues hold
])
def test_fsp6_matches_restatement(restatement, n, L, k, thr, P, S, pbits, seed):
    sig = synth.clustered_signatures(n, L, cluster_count=4, flip=0.12, seed=n + L)
    cell, sim, used = restatement.find_similar_pairs6(sig, L, k, thr, P, S, pbits, seed)
    pairs, gused = capi.find_similar_pairs6(sig, L, k, thr, P, S, pbits, seed)
    assert_same(pairs, gused, cell, sim, used)
    if thr < 1.0 and k > 0:
        assert used.sum() > 0
    else:
        assert used.sum() == 0


def test_fsp6_identical_cells_and_repeat(restatement):
    sig = np.tile(synth.random_signatures(1, 256, seed=3), (300, 1))
    cell, sim, used = restatement.find_similar_pairs6(sig, 256, 8, 0.2, 6, 40, 64, 231)
    for _ in range(2):
        pairs, gused = capi.find_similar_pairs6(sig, 256, 8, 0.2, 6, 40, 64, 231)
        assert_same(pairs, gused, cell, sim, used)


@pytest.mark.parametrize("n", [1, 2, 3])
def test_fsp6_tiny(restatement, n):
    sig = synth.random_signatures(n, 64, seed=n)
    if n == 2:
        sig = np.array([[0x8000000000000000], [0]], dtype=np.uint64)       # cell 1 sorts first in every permutation
    cell, sim, used = restatement.find_similar_pairs6(sig, 64, 3, -1.0, 3, 10, 64, 231)
    pairs, gused = capi.find_similar_pairs6(sig, 64, 3, -1.0, 3, 10, 64, 231)
    assert_same(pairs, gused, cell, sim, used)
    if n == 2:
        assert used.tolist() == [0, 1]            # position 1 starts no backward pointer


def test_fsp6_repeat_call_identical():
    sig = synth.clustered_signatures(800, 512, cluster_count=5, flip=0.1, seed=8)
    a = capi.find_similar_pairs6(sig, 512, 10, 0.2, 12, 150, 64, 5)
    b = capi.find_similar_pairs6(sig, 512, 10, 0.2, 12, 150, 64, 5)
    assert np.array_equal(a[0].view(np.uint64), b[0].view(np.uint64)) and np.array_equal(a[1], b[1])


def test_fsp6_row_shards_through_device_api(restatement):
    import torch
    n, L, k, thr, P, S, pbits, seed = 1500, 512, 12, 0.2, 10, 150, 64, 231
    sig = synth.clustered_signatures(n, L, cluster_count=6, flip=0.08, seed=77)
    whole_pairs, whole_used = capi.find_similar_pairs6(sig, L, k, thr, P, S, pbits, seed)
    cell, sim, used = restatement.find_similar_pairs6(sig, L, k, thr, P, S, pbits, seed)
    assert_same(whole_pairs, whole_used, cell, sim, used)
    d_sig = torch.from_numpy(sig.view(np.int64)).cuda()
    parts, part_used = [], []
    for begin, end in [(0, 600), (600, 601), (601, n)]:
        rows = end - begin
        d_pairs = torch.zeros((rows, k, 2), dtype=torch.int32, device="cuda")
        d_used = torch.zeros(rows, dtype=torch.int32, device="cuda")
        capi.dev_find_similar_pairs6(d_sig.data_ptr(), n, begin, end, L, k, thr, P, S, pbits, seed, d_pairs.data_ptr(),
                                     d_used.data_ptr(), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        parts.append(d_pairs.cpu().numpy().view(np.uint32))
        part_used.append(d_used.cpu().numpy().view(np.uint32))
    p = np.concatenate(parts)
    assert np.array_equal(np.concatenate(part_used), used)
    assert np.array_equal(p[:, :, 0], cell) and np.array_equal(p[:, :, 1], sim.view(np.uint32))


def test_fsp6_facade_files(restatement, tmp_path):
    d = str(tmp_path / "data")
    cells, genes = 600, 500
    toc, g, c = synth.expression_matrix(cells, genes, density=0.05, cluster_count=4, seed=9)
    files.create_directory(d, genes, toc, capi.make_counts(g, c))
    e = ExpressionMatrix(d)
    e.computeLshSignatures(lshName="L", lshCount=256, seed=231)
    e.findSimilarPairs6(lshName="L", similarPairsName="P6", k=15, similarityThreshold=0.2, permutationCount=8,
                        searchCount=120, permutedBitCount=64, seed=231)
    L, sig = files.read_lsh(d, "L")
    cell, sim, used = restatement.find_similar_pairs6(sig, L, 15, 0.2, 8, 120, 64, 231)
    pairs = np.zeros((cells, 15), dtype=capi.PAIR_DTYPE)
    pairs["cell"] = cell
    pairs["similarity"] = sim
    files.write_similar_pairs(d, "Expected", "AllGenes", "AllCells", 15, pairs, used)
    for part in ("-Info", "-Pairs", "-CellInfo"):
        got = open(os.path.join(d, "SimilarPairs-P6" + part), "rb").read()
        want = open(os.path.join(d, "SimilarPairs-Expected" + part), "rb").read()
        assert got == want, part
    assert used.sum() > 0
    # the defaults of the reference's binding (k=100, threshold 0.2, 64 permuted bits, seed 231)
    e.findSimilarPairs6(lshName="L", similarPairsName="D", permutationCount=4, searchCount=50)
    k, p, u = files.read_similar_pairs(d, "D")
    cell, sim, used = restatement.find_similar_pairs6(sig, L, 100, 0.2, 4, 50, 64, 231)
    assert k == 100
    assert_same(p, u, cell, sim, used)


def test_fsp6_scale_sampled_rows(restatement):
    """100 000 cells x 1024 bits, 16 permutations, searchCount 400: the whole device run, 2 048 rows checked."""
    n, L, k, thr, P, S, pbits, seed = 100000, 1024, 20, 0.2, 16, 400, 64, 231
    sig = synth.clustered_signatures(n, L, cluster_count=64, flip=0.15, seed=2024)
    pairs, gused = capi.find_similar_pairs6(sig, L, k, thr, P, S, pbits, seed)
    rows = np.unique(synth.hash_u64(5, np.arange(4096, dtype=np.uint64)) % np.uint64(n)).astype(np.uint32)[:2048]
    rows = np.union1d(rows, np.array([0, 1, n - 2, n - 1], dtype=np.uint32)).astype(np.uint32)
    assert len(rows) >= 2048
    cell, sim, used = restatement.find_similar_pairs6(sig, L, k, thr, P, S, pbits, seed, rows=rows)
    assert_same(pairs[rows], gused[rows], cell, sim, used)
    assert used.sum() > 0
