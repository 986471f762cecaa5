"""Eight fixed random draws of tests/expression_cases.py for each entry that reads the expression counts itself (findSimilarPairs0,
analyzeSimilarPairs, analyzeLsh, createClusterGraph, findSimilarGenePairs0, the gene information content), every draw its own test:
the device entry against the CPU restatement with the comparison of the entry's own test file (expression_cases.check; bit for bit,
byte for byte on the csv files, gene_information_binding.assert_within_bound for the doubles of the information content).
tools/fuzz_parity.py sweeps the same generator for as long as it is given; tests/test_expression_cases_cpu.py asserts, without a
GPU, that these draws are runnable and which kernel forms they reach.

A draw runs only below expression_cases.COST_CAP, chosen so that the slowest restatement of a fixed draw stays at about 2 s on one
CPU thread.  Measured restatement times of the fixed draws, seconds, in the order of FIXED_SEEDS (input generation included):
    fsp0              0.59 0.07 0.01 0.00 1.21 0.18 1.25 0.00    (1.3e8 of cost is about 2 s: 2100 cells x 37 577 genes, all rows, 2.4 s
                                                                  at 1.8e8)
    stored_pairs      0.02 0.00 0.01 0.04 0.53 0.00 0.58 0.03
    analyze_lsh       0.01 1.27 0.02 0.01 0.09 0.03 0.01 0.01    (2100 cells with every pair in the csv, 5.5 s, is above the cap)
    cluster_graph     0.02 0.06 0.00 0.02 0.02 0.02 0.06 0.35    (no draw of its lists reaches the cap)
    gene_pairs        0.11 0.01 0.01 0.00 0.56 0.01 0.43 0.00    (5e8 gene pairs x cells is about 2 s; 2049 genes x 1025 cells, 8.6 s,
                                                                  is above the cap)
    gene_information  0.21 0.04 0.00 0.01 0.00 0.01 0.00 0.09    (no draw of its lists reaches the cap)"""
import pytest

import expression_cases as ec

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def references():
    cache = {}
    return lambda name: cache.setdefault(name, ec.ENTRIES[name].reference())


@pytest.mark.parametrize("name,seed", [(name, seed) for name in ec.ENTRIES for seed in ec.FIXED_SEEDS[name]])
def test_fixed_draw(references, name, seed):
    entry = ec.ENTRIES[name]
    case = entry.draw(ec.rng_of(name, seed))
    assert ec.runnable(name, case), "a fixed draw above the cost cap: %r" % case
    try:
        difference = entry.check(case, references(name))
    except ec.Discarded as reason:
        pytest.fail("a fixed draw that the reference leaves open (%s): %r" % (reason, case))
    assert difference is None, "%s %r: %s" % (name, case, difference)
