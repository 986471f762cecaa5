"""What keeps the sweep over tests/expression_cases.py honest, without a GPU: the restatements alone run the draws, so that
  * of the first 200 draws of every entry at most a quarter are skipped (above the cost cap, or discarded because the reference
    leaves the case open: a makeKnn tie or a NaN similarity in the cluster graph, CZI_ASSERT(bin < binCount) in the two analyses),
    and the eight fixed draws of tests/test_gpu_expression_sweep.py are all runnable;
  * the fixed draws reach, between them, the kernel forms they are there for -- asserted from the shapes, with the formulas of
    csrc/em2_expression.h and csrc/em2_fsp0.hip as expression_cases restates them, themselves checked here against the values the
    existing tests rely on;
  * a case dict reproduces its inputs, and the planted oddities are really there.
The ranged form of the fsp0 restatement, which the ranged draws are compared with, is proved against a full run in
tests/test_fsp0_cpu.py."""
import json

import numpy as np
import pytest

import expression_cases as ec


@pytest.fixture(scope="module")
def outcomes():
    """Per entry and seed 1 .. SWEEP_DRAWS: "run", "cost" or the reason the draw was discarded for."""
    cache = {}

    def of(name):
        if name not in cache:
            entry, reference = ec.ENTRIES[name], ec.ENTRIES[name].reference()
            result = {}
            for seed in range(1, ec.SWEEP_DRAWS + 1):
                case = entry.draw(ec.rng_of(name, seed))
                if not ec.runnable(name, case):
                    result[seed] = "cost"
                    continue
                try:
                    entry.expect(case, reference)
                    result[seed] = "run"
                except ec.Discarded as reason:
                    result[seed] = str(reason)
            cache[name] = result
        return cache[name]
    return of


@pytest.mark.parametrize("name", list(ec.ENTRIES))
def test_at_most_a_quarter_of_the_draws_is_skipped(outcomes, name):
    result = outcomes(name)
    skipped = [seed for seed, outcome in result.items() if outcome != "run"]
    print("%s: %d of %d draws skipped: %s" % (name, len(skipped), len(result), sorted(set(result.values()) - {"run"})))
    assert len(skipped) * 4 <= len(result), {reason: list(result.values()).count(reason) for reason in set(result.values())}
    assert all(result[seed] == "run" for seed in ec.FIXED_SEEDS[name]), [(seed, result[seed]) for seed in ec.FIXED_SEEDS[name]]
    assert len(set(ec.FIXED_SEEDS[name])) == ec.SEEDS_PER_ENTRY and max(ec.FIXED_SEEDS[name]) <= ec.SWEEP_DRAWS


@pytest.mark.parametrize("name", list(ec.ENTRIES))
def test_the_fixed_draws_reach_the_forms_they_are_there_for(name):
    reached = set()
    for case in ec.fixed_draws(name):
        reached |= ec.forms(name, case)
    missing = [form for form in ec.REQUIRED_FORMS[name] if form not in reached]
    assert not missing, (missing, sorted(reached))


def test_fsp0_fixed_draws_in_detail():
    """Both row-vector forms, all three block sizes, a k above the candidate count, a ranged call and a planted tie input, each
    from the case dict and the launch rule of runFsp0 written out once more, independently of expression_cases.fsp0_form."""
    seen = set()
    for case in ec.fixed_draws("fsp0"):
        cells, genes, k = case["cells"], case["genes"], case["k"]
        needed = min(k, cells - 1)
        capacity = 1 << max(needed - 1, 0).bit_length()
        own = 8 * capacity + 8 * 1024 + 128
        row = (4 * genes + 7) // 8 * 8 + (4 * ((genes + 31) // 32) + 7) // 8 * 8
        if row + own <= 160 * 1024:
            seen.add(("lds", 256 if row + own <= 40 * 1024 else 512 if row + own <= 80 * 1024 else 1024))
        else:
            seen.add(("global", 256))
        if k > cells - 1:
            seen.add("k above")
        if case["rows"]:
            seen.add("ranged")
            assert 0 <= case["rows"][0] < case["rows"][1] <= cells
        if "duplicate_cells" in case["plant"]:
            seen.add("ties")
        assert ec.fsp0_form(cells, genes, k)["slot_capacity"] == capacity
    assert {("lds", 256), ("lds", 512), ("lds", 1024), ("global", 256), "k above", "ranged", "ties"} <= seen


def test_restated_formulas():
    """The values the existing tests rely on: 36 864 genes fit next to fsp0's LDS and 40 000 do not; the limit of the kernels
    without LDS of their own is that of tests/test_gpu_analyze_lsh.py; 12 000 and 30 000 genes take the 512- and 1024-thread
    forms; slot capacities are powers of two up to 4096."""
    assert ec.row_vector_bytes(1) == 16 and ec.row_vector_bytes(64) == 256 + 8 and ec.row_vector_bytes(65) == 264 + 16
    assert ec.fsp0_own_lds_bytes(1) == 8 + 8192 + 128
    assert ec.fsp0_form(90, 36864, 3)["in_lds"] and not ec.fsp0_form(260, 40000, 12)["in_lds"]
    assert ec.fsp0_form(257, 12000, 10)["threads"] == 512 and ec.fsp0_form(130, 30000, 5)["threads"] == 1024
    assert ec.fsp0_form(700, 900, 20)["threads"] == 256 and ec.fsp0_form(700, 900, 20)["batches"] == 3
    assert [ec.slot_capacity(4100, k) for k in (0, 1, 2, 3, 128, 129, 4096, 4097)] == [1, 1, 2, 4, 128, 256, 4096, 8192]
    assert ec.slot_capacity(4098, 4097) == 8192 and not ec.fsp0_form(4098, 20, 4097)["supported"]
    assert ec.slot_capacity(4097, 5000) == 4096 and ec.fsp0_form(4097, 20, 5000)["supported"]
    assert ec.ANALYZE_LSH_LIMIT == 39718 and ec.row_vector_bytes(39718) <= 160 * 1024 < ec.row_vector_bytes(39719)
    assert ec.FSP0_LIMIT_K50 < ec.FSP0_LIMIT_K1 < ec.ANALYZE_LSH_LIMIT
    for limit, capacity in ((ec.FSP0_LIMIT_K1, 1), (ec.FSP0_LIMIT_K50, 64)):
        assert ec.fsp0_form(100, limit, capacity)["in_lds"] and not ec.fsp0_form(100, limit + 1, capacity)["in_lds"]
    assert ec.stored_pairs_in_lds(ec.FSP0_LIMIT_K1) and not ec.stored_pairs_in_lds(ec.FSP0_LIMIT_K1 + 1)


def test_a_case_reproduces_its_inputs_and_survives_json():
    for name, entry in ec.ENTRIES.items():
        case = entry.draw(ec.rng_of(name, 3))
        again = json.loads(json.dumps(case))
        assert again == case and entry.draw(ec.rng_of(name, 3)) == case
        assert entry.cost(again) == entry.cost(case)
        if name != "cluster_graph":
            a, b = ec.matrix(case), ec.matrix(again)
            assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


def test_the_planted_oddities_are_there():
    base = {"cells": 65, "genes": 129, "density": 0.25, "clusters": 3, "matrix_seed": 99, "counts": "non_integer"}
    dense = lambda toc, data: (np.repeat(np.arange(len(toc) - 1), np.diff(toc.astype(np.int64))), data["gene"], data["count"])
    plain_toc, plain = ec.matrix(dict(base, plant=[]))
    assert (np.diff(plain_toc.astype(np.int64)) > 0).all() and (plain["count"] > 0).all()
    assert (plain["count"] != np.floor(plain["count"])).any()
    wide = ec.matrix(dict(base, counts="wide", plant=[]))[1]["count"]
    assert wide.max() / wide.min() > 2.0 ** 30
    toc, data = ec.matrix(dict(base, plant=["empty_cell"]))
    assert (np.diff(toc.astype(np.int64)) == 0).sum() == 1
    toc, data = ec.matrix(dict(base, plant=["constant_cell"]))
    full = np.nonzero(np.diff(toc.astype(np.int64)) == 129)[0]
    assert len(full) == 1 and (data["count"][int(toc[full[0]]):int(toc[full[0] + 1])] == 2.5).all()
    toc, data = ec.matrix(dict(base, plant=["empty_gene"]))
    assert len(np.unique(data["gene"])) < len(np.unique(plain["gene"]))
    toc, data = ec.matrix(dict(base, plant=["stored_zero"]))
    assert len(data) == len(plain) and 0 < (data["count"] == 0).sum() < len(data) // 5
    toc, data = ec.matrix(dict(base, plant=["duplicate_cells"]))
    cells = [data[int(toc[c]):int(toc[c + 1])].tobytes() for c in range(65)]
    assert sum(cells[c] == cells[c - 1] for c in range(1, 65)) >= 8
    toc, data = ec.matrix(dict(base, plant=["duplicate_genes"]))
    rows, genes, counts = dense(toc, data)
    table = np.zeros((65, 129), dtype=np.float32)
    table[rows, genes] = counts
    assert sum(np.array_equal(table[:, g], table[:, g - 1]) and table[:, g].any() for g in range(1, 129)) >= 16
    for plant in ec.PLANTS:                                      # the CSR stays a CSR: ascending genes within every cell
        toc, data = ec.matrix(dict(base, plant=[plant]))
        rows, genes, _ = dense(toc, data)
        assert (np.diff(rows * 1000 + genes.astype(np.int64)) > 0).all() and genes.max() < 129 and len(toc) == 66
