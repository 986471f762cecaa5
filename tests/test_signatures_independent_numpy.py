"""The oracle against a second, independent restatement of Lsh::computeCellLshSignatures (src/Lsh.cpp:118-224) and of the per-cell sums it reads
(ExpressionMatrixSubset::computeSums, src/ExpressionMatrixSubset.cpp:46-58) in numpy float64 -- sharing no code with
oracle/em2_oracle.cpp.  The signature of a cell is the sign pattern of sequentially rounded double sums, so the ORDER of the
additions and the separate rounding of every product (no fused multiply-add: the reference is an SSE4.2 build) are what is
restated here: numpy's elementwise `count * v` and `+=` round each operation on its own, one gene (Lsh.cpp:137-144) or one
expression count (:188-198) after the other, vectorised only ACROSS the bits, which are independent.  The hyperplanes are an
input (the normal variates of the reference's Boost are not reproducible here).  The oracle must give the same
64-bit words, including on counts that are no integers, on magnitudes that differ by many orders, and on cells without counts."""
import numpy as np
import pytest

import synth
from projection_limit_cases import compute_signatures      # the restatement itself: tests/projection_limit_cases.py (reference_values)


@pytest.mark.parametrize("cells,genes,L,density,scale", [
    (60, 400, 128, 0.05, None),          # integer counts, as the benchmark's
    (40, 300, 100, 0.08, 0.37),          # fractional counts: every addition rounds
    (30, 500, 1024, 0.03, None),         # the benchmark's width
    (25, 200, 70, 0.2, 1e-3),            # lshCount no multiple of 64; many counts per cell
])
def test_oracle_equals_independent_restatement(oracle, cells, genes, L, density, scale):
    toc, g, c = synth.expression_matrix(cells, genes, density=density, cluster_count=4, seed=cells + genes)
    if scale is not None:
        c = (c * np.float32(scale) + np.float32(0.123)).astype(np.float32)
    vectors = oracle.generate_lsh_vectors(genes, L, 231)
    expect = compute_signatures(toc, g, c, genes, vectors, L)
    got = oracle.compute_signatures(toc, g, c, genes, vectors, L)
    assert np.array_equal(expect, got)


def test_magnitudes_and_empty_cells(oracle):
    rng = np.random.default_rng(5)
    genes, L = 120, 192
    vectors = rng.standard_normal((genes, L)) * np.exp(rng.uniform(-40, 40, size=(genes, 1)))       # rows of very different size
    toc = np.array([0, 0, 5, 5, 40, 41], dtype=np.uint64)                                             # cells 0 and 2 have no counts
    g = np.concatenate([np.sort(rng.choice(genes, 5, replace=False)), np.sort(rng.choice(genes, 35, replace=False)), [7]]).astype(np.uint32)
    c = np.exp(rng.uniform(-20, 20, size=41)).astype(np.float32)
    expect = compute_signatures(toc, g, c, genes, vectors, L)
    got = oracle.compute_signatures(toc, g, c, genes, vectors, L)
    assert np.array_equal(expect, got)
