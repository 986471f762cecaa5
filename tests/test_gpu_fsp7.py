"""GPU parity of findSimilarPairs7 through the C ABI against the oracle's literal restatement
of src/ExpressionMatrixLsh.cpp:507-827.  Bit-exact: cell ids, float similarity bit patterns, usedCount."""
import numpy as np
import pytest

import synth
from expressionmatrix2_amd import ExpressionMatrix, capi, files

pytestmark = pytest.mark.gpu


def assert_same(pairs, gused, cell, sim, used):
    assert np.array_equal(gused, used)
    assert np.array_equal(pairs["cell"], cell)
    assert np.array_equal(pairs["similarity"].view(np.uint32), sim.view(np.uint32))


@pytest.mark.parametrize("n,L,k,thr,lengths,max_check,log2b", [
    (300, 128, 5, 0.2, [16, 8], 50, 12),
    (1000, 256, 10, 0.2, [32, 16, 8], 100, 12),          # 32 >= 12: hashed buckets; 8 < 12: direct
    (1000, 256, 10, 0.2, [32, 16, 8], 7, 20),
    (777, 1024, 100, 0.2, [20, 14], 0, 16),              # no check limit
    (500, 192, 3, 0.0, [64, 33, 1], 1000, 10),           # 64-bit slices, slices straddling words, 1-bit slices
    (2000, 512, 20, 0.5, [24], 300, 24),                 # length == log2BucketCount: hashed
    (900, 100, 4, 0.1, [7, 3], 40, 5),                   # lshCount not a multiple of 64, remainder bits unused
    (65, 64, 70, -0.9, [2], 0, 8),                       # k above the number of cells
    (400, 128, 5, 2.0, [16], 50, 10),                    # threshold above 1: mismatchCount-1 wraps, everything passes
    (500, 32, 100, 0.2, [64, 2], 0, 4),                  # found by tools/fuzz_parity.py: maxCheck 0 and a first length
                                                         # without any slice end the walk before it starts (:667)
    (500, 32, 100, 0.2, [64, 2], 9, 4),                  # same shape with a limit: the 64-bit length is just skipped
])
def test_fsp7_matches_oracle(oracle, n, L, k, thr, lengths, max_check, log2b):
    sig = synth.clustered_signatures(n, L, cluster_count=4, flip=0.12, seed=n + L)
    cell, sim, used = oracle.find_similar_pairs7(sig, L, k, thr, lengths, max_check, log2b)
    pairs, gused = capi.find_similar_pairs7(sig, L, k, thr, lengths, max_check, log2b)
    assert_same(pairs, gused, cell, sim, used)
    if thr < 1.0 and n > 100 and not (max_check == 0 and lengths[0] > L):
        assert used.sum() > 0


def test_fsp7_identical_cells_and_repeat(oracle):
    sig = np.tile(synth.random_signatures(1, 256, seed=3), (500, 1))
    cell, sim, used = oracle.find_similar_pairs7(sig, 256, 8, 0.2, [16, 8], 64, 12)
    for _ in range(2):
        pairs, gused = capi.find_similar_pairs7(sig, 256, 8, 0.2, [16, 8], 64, 12)
        assert_same(pairs, gused, cell, sim, used)


def test_fsp7_errors():
    sig = synth.random_signatures(10, 64)
    with pytest.raises(RuntimeError, match="The slice lengths are not in decreasing order."):
        capi.find_similar_pairs7(sig, 64, 3, 0.2, [8, 8], 5, 10)
    with pytest.raises(RuntimeError, match="Each slice length can be at most 64 bits."):
        capi.find_similar_pairs7(sig, 64, 3, 0.2, [65], 5, 10)
    with pytest.raises(RuntimeError, match="Assertion failed"):
        capi.find_similar_pairs7(sig, 64, 3, -1.5, [8], 5, 10)
    with pytest.raises(RuntimeError, match="positive"):
        capi.find_similar_pairs7(sig, 64, 3, 0.2, [8, 0], 5, 10)


def test_fsp7_facade_files(oracle, tmp_path):
    d = str(tmp_path / "data")
    cells, genes = 600, 500
    toc, g, c = synth.expression_matrix(cells, genes, density=0.05, cluster_count=4, seed=9)
    files.create_directory(d, genes, toc, capi.make_counts(g, c))
    e = ExpressionMatrix(d)
    e.computeLshSignatures(lshName="L", lshCount=256, seed=231)
    e.findSimilarPairs7(lshName="L", similarPairsName="P7", k=15, similarityThreshold=0.2, lshSliceLengths=[16, 10],
                        maxCheck=80, log2BucketCount=12)
    L, sig = files.read_lsh(d, "L")
    cell, sim, used = oracle.find_similar_pairs7(sig, L, 15, 0.2, [16, 10], 80, 12)
    k, pairs, u = files.read_similar_pairs(d, "P7")
    assert k == 15
    assert_same(pairs, u, cell, sim, used)
    with pytest.raises(RuntimeError, match="The slice lengths are not in decreasing order."):
        e.findSimilarPairs7(lshName="L", similarPairsName="Q", lshSliceLengths=[8, 16], maxCheck=10, log2BucketCount=10)
    with pytest.raises(RuntimeError, match="Gene set Nope does not exist."):
        e.findSimilarPairs7(geneSetName="Nope", lshName="L", similarPairsName="Q", lshSliceLengths=[8], maxCheck=10,
                            log2BucketCount=10)


def test_bucketed_and_graph_golden_digests():
    """The committed digests of the fsp5 / fsp7 / cell-graph regression cases (tests/golden/oracle_regression.json,
    written by the oracle) straight against the GPU results."""
    import json
    import os
    from golden.make_golden import bucketed_cases, digest
    with open(os.path.join(os.path.dirname(__file__), "golden", "oracle_regression.json")) as f:
        golden = json.load(f)
    sig, cases = bucketed_cases()
    for name, a in cases.items():
        if name.startswith("fsp5"):
            pairs, used = capi.find_similar_pairs5(sig, 512, a["k"], a["thr"], a["q"], a["overflow"])
        else:
            pairs, used = capi.find_similar_pairs7(sig, 512, a["k"], a["thr"], a["lengths"], a["max_check"], a["log2b"])
        assert digest(np.ascontiguousarray(pairs["cell"]), np.ascontiguousarray(pairs["similarity"]), used) == golden[name], name
    pairs, used = capi.find_similar_pairs4(sig, 512, 20, 0.2)
    ids = np.arange(900, dtype=np.uint32)
    assert digest(*capi.cell_graph_edges(pairs, used, ids, ids, 0.5, 5)) == golden["cellgraph_900_thr0.5_k5"]


# ---- the limits of csrc/em2_fsp7.hip: one wave serving several rows, row ranges, k = 4096, bucket keys above 32 bits ----

def assert_tail_zero(cell, sim_bits, used):
    """Slots beyond usedCount are zero (include/em2_lsh.h: "unused slots are zero")."""
    beyond = np.arange(cell.shape[1])[None, :] >= used[:, None]
    assert not cell[beyond].any() and not sim_bits[beyond].any()


def check(oracle, sig, L, k, thr, lengths, max_check, log2b, repeat=1):
    """The host entry against the oracle, bit for bit; returns the oracle's (cell, sim, used)."""
    cell, sim, used = oracle.find_similar_pairs7(sig, L, k, thr, lengths, max_check, log2b)
    for _ in range(repeat):
        pairs, gused = capi.find_similar_pairs7(sig, L, k, thr, lengths, max_check, log2b)
        assert_same(pairs, gused, cell, sim, used)
        assert_tail_zero(pairs["cell"], pairs["similarity"].view(np.uint32), gused)
    return cell, sim, used


REUSE = dict(L=64, k=6, thr=0.2, lengths=[8, 4], max_check=150, log2b=10)
WAVES = 8192                    # runFsp7 launches min(rows, 8192) waves; traverseKernel strides over the rows


@pytest.fixture(scope="module")
def reuse_case(oracle):
    """24581 cells: three copies of 8192 cells and five more, so that rows r, r + 8192 and r + 16384 -- equal signatures,
    the same buckets in the same order -- are served by the same wave (rows 0, 8192 and 16384 by wave 0), five waves
    serve a fourth row, and a "seen" bit left behind by one row removes a candidate of the next.  Computed once and
    never written to."""
    base = synth.clustered_signatures(WAVES, 64, cluster_count=4, flip=0.1, seed=7)
    sig = np.concatenate([base, base, base, base[:5]])
    a = REUSE
    # preconditions, on the input and on the oracle's result: the cut at 150 (no multiple of 64) falls inside a bucket
    # of the first table, and every row has neighbours to lose
    first_slice = (sig[:, 0] >> np.uint64(64 - a["lengths"][0])).astype(np.int64)           # 8 < log2b: direct buckets
    assert np.bincount(first_slice).max() > a["max_check"]
    expect = oracle.find_similar_pairs7(sig, a["L"], a["k"], a["thr"], a["lengths"], a["max_check"], a["log2b"])
    assert expect[2].min() > 0
    for array in (sig,) + expect:
        array.setflags(write=False)
    return sig, expect


def test_fsp7_wave_serves_several_rows(reuse_case):
    """More than 8192 rows: the seen bits are cleared from the candidate list after every row, the wave's candidate and
    neighbour scratch and selected[] are used again.  Twice in one process."""
    sig, (cell, sim, used) = reuse_case
    assert len(sig) == 3 * WAVES + 5
    a = REUSE
    for _ in range(2):
        pairs, gused = capi.find_similar_pairs7(sig, a["L"], a["k"], a["thr"], a["lengths"], a["max_check"], a["log2b"])
        assert_same(pairs, gused, cell, sim, used)
        assert_tail_zero(pairs["cell"], pairs["similarity"].view(np.uint32), gused)


SENTINEL = 0x5a5a5a5a


def test_fsp7_row_shard_through_device_api(reuse_case):
    """em2_dev_find_similar_pairs7 on row ranges, on torch's current stream: row - rowBegin indexes the outputs, wave w
    starts at row rowBegin + w.  (5, 8202) is 8197 rows, so five waves serve a second row with rowBegin > 0."""
    import torch
    sig, (cell, sim, used) = reuse_case
    n, a = len(sig), REUSE
    d_sig = torch.from_numpy(sig.view(np.int64)).cuda()
    stream = torch.cuda.current_stream().cuda_stream
    for begin, end in [(0, 900), (900, 901), (901, 2500), (5, 8202), (24000, 24581), (700, 700)]:
        rows = end - begin
        d_pairs = torch.full((max(rows, 1), a["k"], 2), SENTINEL, dtype=torch.int32, device="cuda")
        d_used = torch.full((max(rows, 1),), SENTINEL, dtype=torch.int32, device="cuda")
        capi.dev_find_similar_pairs7(d_sig.data_ptr(), n, begin, end, a["L"], a["k"], a["thr"], a["lengths"], a["max_check"],
                                     a["log2b"], d_pairs.data_ptr(), d_used.data_ptr(), stream)
        torch.cuda.synchronize()
        p = d_pairs.cpu().numpy().view(np.uint32)
        u = d_used.cpu().numpy().view(np.uint32)
        if rows == 0:                                    # an empty range is OK and writes nothing
            assert (p == SENTINEL).all() and (u == SENTINEL).all()
            continue
        assert np.array_equal(u, used[begin:end]), (begin, end)
        assert np.array_equal(p[:, :, 0], cell[begin:end]), (begin, end)
        assert np.array_equal(p[:, :, 1], sim[begin:end].view(np.uint32)), (begin, end)
        assert_tail_zero(p[:, :, 0], p[:, :, 1], u)


@pytest.mark.parametrize("thr", [-0.9, 0.3])
def test_fsp7_selection_at_k_4096(oracle, thr):
    """k = kMaxK = the size of selected[].  thr -0.9: every row has 4299 neighbours for 4096 slots (bisection over the
    64-bit keys of a list longer than k, rank sort of 4096 keys).  thr 0.3: rows above and rows at or below k in one
    launch."""
    k = 4096
    sig = synth.clustered_signatures(4300, 128, cluster_count=1, flip=0.2, seed=11)
    cell, sim, used = check(oracle, sig, 128, k, thr, [2], 0, 8)
    if thr < 0:
        assert (used == k).all()
    else:
        assert (used == k).any() and (used < k).any()


@pytest.mark.parametrize("k", [64, 65, 66])
def test_fsp7_selection_around_n_equal_k(oracle, k):
    """65 neighbours per row (every other cell passes): k = 64 is n == k + 1 (bisection), k = 65 is n == k (the copy
    branch, no slot left to clear), k = 66 is n < k (one slot cleared)."""
    sig = synth.clustered_signatures(66, 128, cluster_count=1, flip=0.2, seed=11)
    cell, sim, used = check(oracle, sig, 128, k, -0.9, [1], 0, 8)
    assert (used == min(k, 65)).all()
    if k == 66:                                          # n, as the oracle counts it
        assert (np.sort(cell[:, :65], axis=1) == np.array([np.delete(np.arange(66), r) for r in range(66)])).all()


@pytest.mark.parametrize("lengths,max_check,log2b", [
    ([39, 33], 200, 40),            # direct buckets from slices wider than 32 bits
    ([64, 40], 200, 40),            # hashed buckets under a 40-bit mask
    ([64, 9], 77, 1),               # log2BucketCount 1: every slice is hashed into one of two buckets, runs of hundreds
])
def test_fsp7_bucket_keys(oracle, lengths, max_check, log2b):
    """The bucket part of the sort key (table << 40 | bucket) above 32 bits and at its smallest."""
    sig = synth.clustered_signatures(1500, 256, cluster_count=6, flip=0.01, seed=13)
    cell, sim, used = check(oracle, sig, 256, 10, 0.2, lengths, max_check, log2b)
    assert used.sum() > 0


def test_fsp7_cut_in_a_chunk_with_seen_members_and_the_row(oracle):
    """320 identical cells and 6 outliers that differ from them in the first 16-bit slice only.  For an identical cell
    the first table offers the 319 others; the second table's bucket holds all 326 cells: the cell itself, 319 members
    already seen and the outliers, fresh.  maxCheck = 321 = 64 * 5 + 1 takes outliers 3 and 70 and must leave outlier
    100, which sits in the same 64-member chunk as 70 (and, for rows 64..127, as the row itself).  An outlier's first
    bucket holds nobody else, its second one everybody: 325 fresh members, cut at 321 inside the sixth chunk.  k above
    the number of cells, so every candidate taken shows in the result."""
    L, k, thr, lengths, log2b = 128, 400, 0.2, [16, 8], 20             # 16 and 8 < 20: direct buckets, no collisions
    outliers = [3, 70, 100, 130, 200, 300]
    n, max_check = 320 + len(outliers), 64 * 5 + 1
    sig = np.tile(synth.random_signatures(1, L, seed=5), (n, 1))
    for j, o in enumerate(outliers):
        for bit in range(j + 1):                                       # j + 1 mismatches, all inside slice 0 of length 16
            sig[o, 0] ^= np.uint64(1) << np.uint64(63 - bit)
    assert n - len(outliers) - 1 < max_check < n - 1
    cell, sim, used = check(oracle, sig, L, k, thr, lengths, max_check, log2b, repeat=2)
    assert (used == max_check).all()                                   # the cut was reached on every row, nobody failed thr
    identical = np.setdiff1d(np.arange(n), outliers)
    taken = np.array([np.isin(outliers, cell[r, :used[r]]) for r in identical])
    assert (taken == [True, True, False, False, False, False]).all()   # by the oracle: cut between members 70 and 100
