"""Rank-sum marker genes on the GPU (csrc/em2_rank_genes.hip): every array equal, bit for bit, to the one-thread restatement
(tests/native/em2_rank_genes_restatement.cpp, a std::sort of all N values per gene), through the host entry and through the
device entry, with the test limits at their defaults and forced small (one block, chunks of 64 entries, the counters of the
accumulate pass in global memory from three groups on); the input errors, which leave the outputs untouched."""
import numpy as np
import pytest

import rank_genes_binding as rgb
from expressionmatrix2_amd import capi

pytestmark = pytest.mark.gpu

# cells x genes x groups: 1, 63, 64, 65 and 300 cells; 1, 33 and 70 genes; 1, 2, 3 and 65 groups
CASES = ["random-1x1x1", "random-63x33x2", "random-64x1x3", "random-65x70x65", "random-300x33x3", "odd", "chunks"]
# (maxBlocks, chunkEntries, ldsGroupLimit)
LIMITS = {"defaults": (0, 0, 0), "one block": (1, 0, 0), "chunks of 64": (0, 64, 0), "global counters": (0, 0, 2), "all small": (1, 64, 2)}


@pytest.fixture(scope="module")
def restatement():
    return rgb.load()


@pytest.fixture
def limits():
    """Sets the test limits and restores the defaults afterwards."""
    lib = capi.load()
    yield lambda name: lib.em2_set_rank_genes_test_limits(*LIMITS[name])
    lib.em2_set_rank_genes_test_limits(0, 0, 0)


@pytest.mark.parametrize("limit", list(LIMITS))
@pytest.mark.parametrize("name", CASES)
def test_both_entries_equal_the_restatement(restatement, limits, name, limit):
    toc, data, genes, group, groups = rgb.case(name)
    theirs = restatement.rank_genes(toc, data, genes, group, groups)
    limits(limit)
    rgb.assert_same(capi.rank_genes(toc, data, genes, group, groups), theirs, "%s, %s, host entry" % (name, limit))
    rgb.assert_same(capi.dev_rank_genes(toc, data, genes, group, groups, fill=0xab), theirs, "%s, %s, device entry" % (name, limit),
                    rgb.INTEGERS)


@pytest.mark.parametrize("limit", ["defaults", "all small"])
@pytest.mark.parametrize("method", [1, 2])
def test_normalised_values_and_an_empty_cell(restatement, limits, method, limit):
    toc, data, genes, group, groups = rgb.case("random-300x33x3")
    norm = rgb.norm_inverses(toc, data)[method - 1]
    theirs = restatement.rank_genes(toc, data, genes, group, groups, norm)
    limits(limit)
    rgb.assert_same(capi.rank_genes(toc, data, genes, group, groups, norm), theirs, "method %d, host entry" % method)
    rgb.assert_same(capi.dev_rank_genes(toc, data, genes, group, groups, norm), theirs, "method %d, device entry" % method, rgb.INTEGERS)


def test_the_chunk_case_holds_what_it_says(limits):
    """With chunks of 64 entries: a run of 300 equal values crosses five chunks, a gene of 300 distinct values, a gene stored
    nowhere, a gene of stored zeros only."""
    toc, data, genes, group, groups = rgb.case("chunks")
    dense = rgb.dense_values(toc, data, genes)
    stored = np.zeros(dense.shape, dtype=bool)
    stored[np.repeat(np.arange(300), np.diff(toc.astype(np.int64))), data["gene"]] = True
    assert stored[:, 0].all() and len(np.unique(dense[:, 0])) == 1 and 300 > 4 * 64
    assert stored[:, 1].all() and len(np.unique(dense[:, 1])) == 300
    assert not stored[:, 2].any() and stored[:, 3].any() and not dense[:, 3].any()
    limits("chunks of 64")
    mine = capi.rank_genes(toc, data, genes, group, groups)
    assert mine["tieSum"][0] == 300 ** 3 - 300 and mine["tieSum"][1] == 0
    assert np.array_equal(mine["nonZeroCount"][0], mine["groupSize"]) and not mine["nonZeroCount"][3].any()


def test_groups_of_every_kind(restatement, limits):
    """One group that is the whole universe (z = 0, auc = 0.5), an empty group among others, every cell in no group."""
    toc, data, genes, _, _ = rgb.case("random-65x70x65")
    for limit in ("defaults", "all small"):
        limits(limit)
        for group, groups in [(np.zeros(65, np.uint32), 1), (np.arange(65, dtype=np.uint32) % 2 * 2, 4), (np.full(65, rgb.NO_GROUP, np.uint32), 3)]:
            mine = capi.rank_genes(toc, data, genes, group, groups)
            rgb.assert_same(mine, restatement.rank_genes(toc, data, genes, group, groups), "%d groups, %s" % (groups, limit))
            if groups == 1:
                assert not mine["zScore"].any() and np.all(mine["auc"] == 0.5)


def bad_inputs():
    toc, data, genes, group, groups = rgb.case("random-63x33x2")
    descending = toc.copy()
    descending[10], descending[11] = toc[11], toc[10]
    beyond = data.copy()
    beyond["gene"][int(toc[20])] = genes
    unsorted = data.copy()
    first = int(toc[30])
    assert toc[31] - toc[30] >= 2
    unsorted["gene"][[first, first + 1]] = unsorted["gene"][[first + 1, first]]
    nan = data.copy()
    nan["count"][int(toc[40])] = np.nan
    bad_group = group.copy()
    bad_group[50] = groups
    return {"a descending toc": ((descending, data, genes, group, groups), "toc .* not ascending"),
            "a gene id that is not below geneCount": ((toc, beyond, genes, group, groups), "a local gene id is not below geneCount"),
            "unsorted gene ids": ((toc, unsorted, genes, group, groups), "the gene ids of a cell are not strictly ascending"),
            "NaN": ((toc, nan, genes, group, groups), "a value is not a number"),
            "a group id that is not below groupCount": ((toc, data, genes, bad_group, groups), "a group id is neither below groupCount nor the no-group value")}


@pytest.mark.parametrize("what", list(bad_inputs()))
def test_an_input_error_leaves_the_outputs_untouched(what):
    arguments, text = bad_inputs()[what]
    with pytest.raises(RuntimeError, match="em2_dev_rank_genes: " + text) as error:
        capi.dev_rank_genes(*arguments, fill=0xab)
    for name, array in error.value.outputs.items():
        assert np.all(array.view(np.uint8) == 0xab), name
    with pytest.raises(RuntimeError, match="em2_rank_genes: " + text):          # (a descending toc: the host's own check answers)
        capi.rank_genes(*arguments)


def test_an_infinite_factor_times_a_stored_zero_is_not_a_number():
    """0 * inf: the value is defined as the float product, so the call fails as for any NaN."""
    toc, data, genes, group, groups = rgb.case("random-63x33x2")
    zero = data.copy()
    zero["count"][int(toc[5])] = 0.
    norm = np.ones(63)
    norm[5] = np.inf
    with pytest.raises(RuntimeError, match="em2_rank_genes: a value is not a number"):
        capi.rank_genes(toc, zero, genes, group, groups, norm)
