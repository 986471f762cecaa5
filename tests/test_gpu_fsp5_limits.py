"""findSimilarPairs5 on the paths the shapes of tests/test_gpu_fsp5.py do not reach: several passes of unionKernel's bitmap,
filterWideKernel with lanes beyond the row, an unaligned signature array, candidate lists of exactly the lengths at which
another selection launch takes over, slice counts at the form switches, slices of 31 and 32 bits, the overflow rule at
size == bucketOverflow.  Everything bit-exact against the CPU oracle (q = 31, 32: against the numpy model the CPU test checks
against the oracle at q = 30); every test asserts through em2_dev_find_similar_pairs5_last_launch that the form it means ran.
The inputs come from tests/fsp5_limit_cases.py; tests/test_fsp5_limit_cases_cpu.py shows that they are what is claimed here."""
import numpy as np
import pytest

import fsp5_limit_cases as cases
from expressionmatrix2_amd import capi

pytestmark = pytest.mark.gpu


def last():
    return capi.dev_find_similar_pairs5_last_launch()


def same(got_cell, got_sim, got_used, cell, sim, used):
    assert np.array_equal(got_used, used)
    assert np.array_equal(got_cell, cell)
    assert np.array_equal(got_sim.view(np.uint32), sim.view(np.uint32))


def host_run(sig, L, k, thr, q, ovf):
    pairs, used = capi.find_similar_pairs5(sig, L, k, thr, q, ovf)
    return pairs["cell"], pairs["similarity"], used


def device_run(sig, L, k, thr, q, ovf, begin, end, misaligned=False):
    """em2_dev_find_similar_pairs5 for the rows [begin, end); misaligned: the signatures start 8 bytes past a 16-byte boundary."""
    import torch
    flat = torch.from_numpy(np.ascontiguousarray(sig).view(np.int64).reshape(-1))
    buffer = torch.empty(flat.numel() + 1, dtype=torch.int64, device="cuda")
    assert buffer.data_ptr() % 16 == 0
    d_sig = buffer[1:] if misaligned else buffer[:-1]
    d_sig.copy_(flat)
    assert d_sig.data_ptr() % 16 == (8 if misaligned else 0)
    rows = end - begin
    d_pairs = torch.full((rows, max(k, 1), 2), 0x5a5a5a5a, dtype=torch.int32, device="cuda")
    d_used = torch.full((rows,), 0x5a5a5a5a, dtype=torch.int32, device="cuda")
    capi.dev_find_similar_pairs5(d_sig.data_ptr(), len(sig), begin, end, L, k, thr, q, ovf, d_pairs.data_ptr(), d_used.data_ptr(),
                                 torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    p = d_pairs.cpu().numpy().view(np.uint32)[:, :k]
    return p[:, :, 0], p[:, :, 1].view(np.float32), d_used.cpu().numpy().view(np.uint32)


def check_all(oracle, sig, L, k, thr, q, ovf):
    cell, sim, used = oracle.find_similar_pairs5(sig, L, k, thr, q, ovf)
    same(*host_run(sig, L, k, thr, q, ovf), cell, sim, used)
    return used


# ---- B1: three passes of the bitmap ----
@pytest.fixture(scope="module")
def union_case(oracle):
    P = last()["union_ids_per_pass"]
    c = cases.union_passes_case(P)
    c["expected"] = {thr: oracle.find_similar_pairs5_cells(c["sig"], c["L"], c["k"], thr, c["q"], 0, c["cells"])
                     for thr in cases.UNION_THRESHOLDS}
    return c


@pytest.mark.parametrize("thr", cases.UNION_THRESHOLDS)
def test_union_three_passes_all_rows(union_case, thr):
    """All 2 P + 4099 rows through the host entry: ids on both sides of both pass edges in one bucket, a pass beyond the staged
    ids between two staged ones, a bucket longer than the members a block holds in registers whose tail lies in the last pass.
    More than 2^20 cells: two batches at the least."""
    c = union_case
    cell, sim, used = host_run(c["sig"], c["L"], c["k"], thr, c["q"], 0)
    info = last()
    assert info["union_form"] == 1 and info["union_passes"] == 3 and info["union_ids_per_pass"] == c["P"]
    assert info["batches"] >= 2 and info["cells"] == c["n"] and info["packed"] == 1
    assert info["filter_form"] == "cooperative"                      # one word per signature
    rows = c["cells"]
    same(cell[rows], sim[rows], used[rows], *c["expected"][thr])
    assert used[c["family_c"]].min() == c["k"]
    if thr < -1:
        # every candidate passes: with k = 8 every cell of the three families has a full row
        assert (used[c["family_a"]] >= 6).all() and (used[c["family_b"]] == c["k"]).all()


def test_union_three_passes_row_range_from_inside_pass_1(union_case):
    c = union_case
    begin, end = c["rows"]
    inside = (c["cells"] >= begin) & (c["cells"] < end)
    rows = c["cells"][inside] - begin
    for thr in cases.UNION_THRESHOLDS:
        cell, sim, used = device_run(c["sig"], c["L"], c["k"], thr, c["q"], 0, begin, end)
        info = last()
        assert info["union_passes"] == 3 and info["cells"] == end - begin
        ecell, esim, eused = c["expected"][thr]
        same(cell[rows], sim[rows], used[rows], ecell[inside], esim[inside], eused[inside])


# ---- B2: filter widths ----
@pytest.mark.parametrize("L", sorted(cases.FILTER_WIDTHS))
def test_filter_width(oracle, L):
    """Widths whose rows leave lanes of filterWideKernel without a unit (the `active` masking), the last cooperative width and
    the first beyond; the second threshold, 0, cuts through the mismatch counts of cells of different clusters."""
    sig = cases.filter_case(L)
    for thr in cases.FILTER_THRESHOLDS:
        used = check_all(oracle, sig, L, cases.FILTER_K, thr, cases.FILTER_Q, 0)
        assert last()["filter_form"] == cases.FILTER_WIDTHS[L][0]
        assert used.sum() > 0


@pytest.mark.parametrize("L", cases.FILTER_UNALIGNED_WIDTHS)
def test_filter_unaligned_signatures(oracle, L):
    """An even word count at an address that is 8 but not 16 bytes aligned: the cooperative form, not the 16-byte loads."""
    sig = cases.filter_case(L)
    n = len(sig)
    for thr in cases.FILTER_THRESHOLDS:
        expected = oracle.find_similar_pairs5(sig, L, cases.FILTER_K, thr, cases.FILTER_Q, 0)
        same(*device_run(sig, L, cases.FILTER_K, thr, cases.FILTER_Q, 0, 0, n, misaligned=True), *expected)
        assert last()["filter_form"] == "cooperative"
        same(*device_run(sig, L, cases.FILTER_K, thr, cases.FILTER_Q, 0, 0, n), *expected)
        assert last()["filter_form"] == cases.filter_form(L) and last()["filter_form"].startswith("wide")


# ---- B3: selection tiers ----
def check_tier(oracle, entries, L, k, flips, packed):
    sig = cases.tier_case(entries, L, flips)
    cell, sim, used = host_run(sig, L, k, cases.TIER_THRESHOLD, cases.TIER_Q, 0)
    assert last()["packed"] == packed
    assert (used == min(k, entries)).all()
    for begin, end in cases.tier_rows(entries):
        expected = oracle.find_similar_pairs5_rows(sig, L, k, cases.TIER_THRESHOLD, cases.TIER_Q, 0, begin, end)
        same(cell[begin:end], sim[begin:end], used[begin:end], *expected)


@pytest.mark.parametrize("flips", [0, cases.TIER_FLIPS])
@pytest.mark.parametrize("entries", cases.TIER_PACKED_ENTRIES)
def test_selection_packed_tier_edges(oracle, entries, flips):
    """Lists of exactly CAPACITY and CAPACITY + 1 entries of every packed tier (4096 / 5120 / 6144 / 8192 / 16384, then global
    memory): all ties, and up to 12 flipped bits per cell."""
    check_tier(oracle, entries, 64, cases.TIER_PACKED_K, flips, packed=1)


@pytest.mark.parametrize("flips", [0, cases.TIER_FLIPS])
@pytest.mark.parametrize("entries", cases.TIER_WHOLE_ENTRIES)
def test_selection_whole_entry_tier_edges(oracle, entries, flips):
    """k = 2049, one past the packed form: the tiers of whole entries (4096 / 5120 / 6656 / 12288, then global memory)."""
    check_tier(oracle, entries, 128, cases.TIER_WHOLE_K, flips, packed=0)


@pytest.mark.parametrize("flips", [0, cases.TIER_FLIPS])
@pytest.mark.parametrize("k", cases.TIER_K_EDGES)
def test_selection_k_edges(oracle, k, flips):
    """k = 1024 / 1025 (the padded survivor sort doubles) and 2048 / 2049 (the survivors fill the position arrays exactly; the
    form switches) on lists of 4500."""
    check_tier(oracle, cases.TIER_K_EDGE_ENTRIES, 128, k, flips, packed=1 if k <= 2048 else 0)


# ---- B4: slice counts ----
@pytest.mark.parametrize("L", sorted(cases.SLICES_WIDTHS))
def test_slice_counts(oracle, L):
    sig = cases.slices_case(L)
    used = check_all(oracle, sig, L, cases.SLICES_K, cases.SLICES_THRESHOLD, cases.SLICES_Q, 0)
    info = last()
    assert info["slice_count"] == cases.SLICES_WIDTHS[L]
    assert info["union_form"] == (1 if info["slice_count"] <= 256 else 0)
    assert info["union_passes"] == info["union_form"]
    assert used.sum() > 0


def test_union_form_flips_between_256_and_257_slices(oracle):
    forms = {}
    for L in (1024, 1028):
        sig = cases.slices_case(L)[:100]
        check_all(oracle, sig, L, 3, cases.SLICES_THRESHOLD, cases.SLICES_Q, 0)
        forms[L] = last()["union_form"]
    assert forms == {1024: 1, 1028: 0}


@pytest.mark.parametrize("L", cases.SLICES_OVERFLOW_WIDTHS)
def test_slice_counts_with_dropped_buckets(oracle, L):
    """A bucketOverflow that drops some of nearly every cell's buckets: descriptors of size zero inside the prefix search."""
    sig = cases.slices_case(L)
    used = check_all(oracle, sig, L, cases.SLICES_K, cases.SLICES_THRESHOLD, cases.SLICES_Q, cases.slices_overflow(sig, L))
    assert last()["union_form"] == 1 and last()["slice_count"] == cases.SLICES_WIDTHS[L]
    assert used.sum() > 0


# ---- B5: slices of 30, 31 and 32 bits ----
@pytest.mark.parametrize("q", [30, 31, 32])
def test_wide_slices_against_the_numpy_model(oracle, q):
    sig, _ = cases.wide_slice_case(q)
    L, k = cases.WIDE_L, cases.WIDE_K
    table = oracle.similarity_table(L)
    for thr in cases.WIDE_THRESHOLDS:
        expected = cases.lists_to_arrays(cases.wide_slice_model(sig, L, q, thr, table), k)
        if q == 30:
            # the model's order (similarity descending, cell ascending) is the oracle's where the oracle reaches
            same(*expected, *oracle.find_similar_pairs5_rows(sig, L, k, thr, q, 0, 0, len(sig)))
        same(*host_run(sig, L, k, thr, q, 0), *expected)
        assert last()["slice_count"] == L // q
        assert expected[2].sum() > 0


# ---- B6: small edges ----
def test_overflow_rule_at_the_bucket_size(oracle):
    """Buckets of exactly bucketOverflow cells are used, of bucketOverflow + 1 dropped (ExpressionMatrixLsh.cpp:419)."""
    sig = cases.overflow_groups_case()
    b = cases.OVERFLOW_B
    used = check_all(oracle, sig, cases.OVERFLOW_L, 50, 0.2, cases.OVERFLOW_Q, b)
    first, second = cases.OVERFLOW_GROUP_AT
    assert (used[first:first + b] == b - 1).all() and (used[second:second + b + 1] == 0).all()


def test_k_zero(oracle):
    sig = cases.edge_case()
    cell, sim, used = host_run(sig, cases.EDGE_L, 0, 0.2, cases.EDGE_Q, 0)
    assert cell.shape == (cases.EDGE_N, 0) and not used.any()
    cell, sim, used = device_run(sig, cases.EDGE_L, 0, 0.2, cases.EDGE_Q, 0, 100, 400)
    assert not used.any()


@pytest.mark.parametrize("thr,some", [(1.0, False), (2.0, False), (-2.0, True), (0.999, True)])
def test_thresholds_that_pass_nothing_and_everything(oracle, thr, some):
    sig = cases.edge_case()
    used = check_all(oracle, sig, cases.EDGE_L, 40, thr, cases.EDGE_Q, 0)
    assert bool(used.sum()) == some


def test_row_range_over_many_batches(oracle, monkeypatch):
    """A device-entry row range that does not start at row 0, cut into batches of more than 64 cells (the grouped visiting
    order runs in each): every batch writes its rows at (batchBegin - rowBegin) * k."""
    monkeypatch.setenv("EM2_FSP5_BATCH_LOG2", str(cases.BATCH_LOG2))
    sig = cases.batch_case()
    begin, end = cases.BATCH_ROWS
    args = (cases.BATCH_L, cases.BATCH_K, cases.BATCH_THRESHOLD, cases.BATCH_Q, 0)
    got = device_run(sig, *args, begin, end)
    info = last()
    assert info["batches"] >= 4 and info["cells"] == end - begin and info["cells"] / info["batches"] > 64
    assert info["filter_form"] == "wide<1,0,false>"
    same(*got, *oracle.find_similar_pairs5_rows(sig, *args, begin, end))
