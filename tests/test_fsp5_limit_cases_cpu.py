"""The inputs of tests/test_gpu_fsp5_limits.py (tests/fsp5_limit_cases.py) are what that file says they are: shown here with
numpy and the CPU oracle, without a GPU."""
import numpy as np
import pytest

import fsp5_limit_cases as cases

IDS_PER_PASS = 17408 * 32          # csrc/em2_fsp5.hip: kUnionWords * 32 (the GPU test takes it from the library)


@pytest.fixture(scope="module")
def union_case():
    return cases.union_passes_case(IDS_PER_PASS)


def test_union_case_families_by_pass(union_case):
    c = union_case
    P, n, sig = c["P"], c["n"], c["sig"]
    assert n == 2 * P + 4099 and -(-n // P) == 3                    # three passes
    values = cases.slice_values(sig, cases.UNION_L, cases.UNION_Q)
    assert values.shape == (n, 4)

    def by_pass(members):
        return tuple(int(((members >= lo) & (members < hi)).sum()) for lo, hi in ((0, P), (P, 2 * P), (2 * P, n)))

    for slice_, value, family, counts in ((cases.UNION_SLICE_A, cases.UNION_VALUE_A, c["family_a"], (2, 3, 2)),
                                          (cases.UNION_SLICE_B, cases.UNION_VALUE_B, c["family_b"], cases.UNION_FAMILY_B),
                                          (cases.UNION_SLICE_C, cases.UNION_VALUE_C, c["family_c"], cases.UNION_FAMILY_C)):
        members = np.nonzero(values[:, slice_] == value)[0]
        assert np.array_equal(members, np.sort(family))             # the family and nobody else
        assert by_pass(members) == tuple(counts)
    assert list(c["family_a"]) == [5, P - 1, P, P + 1, 2 * P - 1, 2 * P, n - 1]
    assert cases.UNION_FAMILY_B == (100, 3000, 100)                 # pass 1 alone beyond the 2304 staged ids, between two staged passes
    assert cases.UNION_FAMILY_B[1] > 2304 > cases.UNION_FAMILY_B[0]
    # (c): more members than the 6 x 1024 a block holds in registers, and those beyond are ids of pass 2 (members are numbered
    # slice by slice, ascending inside a bucket: slice 0's few first, then this bucket of slice 1)
    assert sum(cases.UNION_FAMILY_C) == 7000 > 6144
    family_c = np.sort(c["family_c"])
    assert (family_c[6144 - 64:] >= 2 * P).all()
    assert len(set(c["family_a"]) | set(c["family_b"]) | set(c["family_c"])) == 7 + 3200 + 7000          # disjoint
    begin, end = c["rows"]
    assert P < begin < 2 * P < end < n                              # the device-entry range starts inside pass 1
    in_range = c["cells"][(c["cells"] >= begin) & (c["cells"] < end)]
    assert len(in_range) >= 40 and np.isin(c["family_c"], in_range).any() and np.isin(c["family_b"], in_range).any()


def test_union_case_oracle_lists(oracle, union_case):
    """With a threshold below -1 every candidate passes: the planted cells' lists are their families (and a few chance mates)."""
    c = union_case
    cell, sim, used = oracle.find_similar_pairs5_cells(c["sig"], c["L"], 7100, -2.0, c["q"], 0, c["family_c"][:2])
    assert (used >= 6999).all() and (used < 7100).all()
    cell, sim, used = oracle.find_similar_pairs5_cells(c["sig"], c["L"], 400, -2.0, c["q"], 0, c["family_a"])
    assert (used >= 6).all() and (used < 400).all()
    for row, me in zip(cell, c["family_a"]):
        assert np.isin(np.setdiff1d(c["family_a"], [me]), row).all()


@pytest.mark.parametrize("L", sorted(cases.FILTER_WIDTHS))
def test_filter_case_widths_and_forms(hostchecks, L):
    form, units, lanes = cases.FILTER_WIDTHS[L]
    words = (L - 1) // 64 + 1
    sig = cases.filter_case(L)
    assert sig.shape == (cases.FILTER_N, words)
    assert cases.filter_form(L) == form
    if form.startswith("wide"):
        assert words % 2 == 0 and units == words // 2 and units <= lanes * int(form[5])
        assert not form.endswith("true>") and units < lanes * int(form[5])          # some lane is beyond the row
    if L == 8192:
        assert words == 128
    if L == 8256:
        assert words == 129
    if L == 1100:
        assert L % 64 != 0 and words == 18
    # threshold 0: among the candidates (cells that share a slice) there are mismatch counts on both sides of the last
    # accepted one, close to it -- a count that is off by a few flips a decision
    m_global = hostchecks.tables(L, 0.0)["m_global"]
    values = cases.slice_values(sig, L, cases.FILTER_Q)
    a, b = np.triu_indices(cases.FILTER_N, 1)
    share = np.zeros(len(a), dtype=bool)
    for s in range(values.shape[1]):
        share |= values[a, s] == values[b, s]
    m = cases.mismatches(sig, a[share], b[share])
    near = max(4, L // 64)
    assert ((m <= m_global) & (m > m_global - near)).any() and ((m > m_global) & (m <= m_global + near)).any()


def test_filter_forms_by_shape():
    assert {cases.filter_form(L) for L in range(1152, 1921, 128)} == {"wide<1,16,false>"}        # 18 .. 30 words
    assert {cases.filter_form(L) for L in range(2176, 3969, 128)} == {"wide<2,16,false>"}        # 34 .. 62 words
    assert cases.filter_form(2048) == "wide<4,4,true>" and cases.filter_form(4096) == "wide<2,16,true>"
    for L in cases.FILTER_UNALIGNED_WIDTHS:
        assert cases.filter_form(L).startswith("wide") and cases.filter_form(L, aligned=False) == "cooperative"
    # two units per lane means 17 units or more, for which the lanes per candidate always reach 16
    assert "wide<2,0,false>" not in {cases.filter_form(L) for L in range(1, 9000)}


@pytest.mark.parametrize("entries,L,flips", [(e, 64, f) for e in cases.TIER_PACKED_ENTRIES for f in (0, cases.TIER_FLIPS)] +
                         [(e, 128, f) for e in cases.TIER_WHOLE_ENTRIES + (cases.TIER_K_EDGE_ENTRIES,) for f in (0, cases.TIER_FLIPS)])
def test_tier_case_list_lengths(oracle, entries, L, flips):
    sig = cases.tier_case(entries, L, flips)
    assert len(sig) == entries + 1
    assert (sig == sig[0]).all() == (flips == 0)
    for begin, end in cases.tier_rows(entries):
        assert end - begin == 20
        cell, sim, used = oracle.find_similar_pairs5_rows(sig, L, entries + 5, cases.TIER_THRESHOLD, cases.TIER_Q, 0, begin, end)
        assert (used == entries).all()                             # k beyond the list: its whole length


@pytest.mark.parametrize("L", sorted(cases.SLICES_WIDTHS))
def test_slices_case(L):
    assert L // cases.SLICES_Q == cases.SLICES_WIDTHS[L]
    sig = cases.slices_case(L)
    assert cases.slice_values(sig, L, cases.SLICES_Q).shape == (cases.SLICES_N, cases.SLICES_WIDTHS[L])
    if L in cases.SLICES_OVERFLOW_WIDTHS:
        overflow = cases.slices_overflow(sig, L)
        dropped = (cases.bucket_sizes(cases.slice_values(sig, L, cases.SLICES_Q)) > overflow).sum(axis=1)
        partly = (dropped > 0) & (dropped < cases.SLICES_WIDTHS[L])
        assert partly.mean() > 0.9                                  # some, not all, of the cell's buckets are dropped


def test_slices_widths_cover_the_form_switches():
    assert sorted(cases.SLICES_WIDTHS.values()) == [64, 65, 255, 256, 257]
    assert cases.SLICES_WIDTHS[1024] == 256 and cases.SLICES_WIDTHS[1028] == 257


@pytest.mark.parametrize("q", [30, 31, 32])
def test_wide_slice_case(oracle, q):
    sig, copied = cases.wide_slice_case(q)
    L = cases.WIDE_L
    bits = cases.bits_of(sig, L)
    assert len(copied) == cases.WIDE_N - cases.WIDE_ORIGINALS >= cases.WIDE_N // 2
    ends = set()
    for c, partner, s, outside in copied:
        begin, end = s * q, (s + 1) * q
        assert np.array_equal(bits[c, begin:end], bits[partner, begin:end])
        assert outside in (begin - 1, end) and 0 <= outside < L and bits[c, outside] != bits[partner, outside]
        ends.add(outside == end)
        for other in range(L // q):                               # exactly one slice shared
            if other != s:
                assert not np.array_equal(bits[c, other * q:(other + 1) * q], bits[partner, other * q:(other + 1) * q])
    assert ends == {True, False}
    table = oracle.similarity_table(L)
    for thr in cases.WIDE_THRESHOLDS:
        lists = cases.wide_slice_model(sig, L, q, thr, table)
        assert max(len(found) for found in lists) <= cases.WIDE_K        # keepBest never cuts
        if thr < -1:
            for c, partner, s, outside in copied:
                assert partner in [o for o, _ in lists[c]] and c in [o for o, _ in lists[partner]]
    counts = [len(found) for found in cases.wide_slice_model(sig, L, q, cases.WIDE_THRESHOLDS[1], table)]
    all_counts = [len(found) for found in cases.wide_slice_model(sig, L, q, -2.0, table)]
    assert 0 < sum(counts) < sum(all_counts)                        # the second threshold decides


def test_wide_slice_model_is_the_oracle_at_30_bits(oracle):
    """The model that stands in for the oracle at q = 31 and 32 gives the oracle's SimilarPairs where the oracle reaches."""
    q, L, k = 30, cases.WIDE_L, cases.WIDE_K
    sig, _ = cases.wide_slice_case(q)
    table = oracle.similarity_table(L)
    for thr in cases.WIDE_THRESHOLDS:
        cell, sim, used = cases.lists_to_arrays(cases.wide_slice_model(sig, L, q, thr, table), k)
        ocell, osim, oused = oracle.find_similar_pairs5_rows(sig, L, k, thr, q, 0, 0, len(sig))
        assert np.array_equal(used, oused) and np.array_equal(cell, ocell)
        assert np.array_equal(sim.view(np.uint32), osim.view(np.uint32))
        assert used.sum() > 0


def test_overflow_groups_case(oracle):
    sig = cases.overflow_groups_case()
    b = cases.OVERFLOW_B
    sizes = cases.bucket_sizes(cases.slice_values(sig, cases.OVERFLOW_L, cases.OVERFLOW_Q))
    first, second = cases.OVERFLOW_GROUP_AT
    assert (sizes[first:first + b] == b).all() and (sizes[second:second + b + 1] == b + 1).all()
    others = np.ones(len(sig), dtype=bool)
    others[first:first + b] = others[second:second + b + 1] = False
    assert (sizes[others] <= 2).all()
    cell, sim, used = oracle.find_similar_pairs5(sig, cases.OVERFLOW_L, 50, 0.2, cases.OVERFLOW_Q, b)
    assert (used[first:first + b] == b - 1).all() and (used[second:second + b + 1] == 0).all()


def test_edge_case_thresholds(oracle):
    sig = cases.edge_case()
    for thr, some in ((1.0, False), (2.0, False), (-2.0, True)):
        cell, sim, used = oracle.find_similar_pairs5(sig, cases.EDGE_L, 6, thr, cases.EDGE_Q, 0)
        assert bool(used.sum()) == some
    cell, sim, used = oracle.find_similar_pairs5(sig, cases.EDGE_L, 40, 0.999, cases.EDGE_Q, 0)
    assert (used[:30] == 29).all() and (sim[:30, :29] == 1.0).all()             # similarity exactly 1: not above a threshold of 1


def test_batch_case_plan():
    sig = cases.batch_case()
    gathered = cases.bucket_sizes(cases.slice_values(sig, cases.BATCH_L, cases.BATCH_Q)).sum(axis=1)
    begin, end = cases.BATCH_ROWS
    assert 0 < begin < end < cases.BATCH_N
    batches = cases.plan_batches(gathered, begin, end, cases.BATCH_LOG2)
    assert len(batches) >= 4 and batches[0][0] == begin and batches[-1][1] == end
    assert all(stop - start > 64 for start, stop in batches[:-1])          # the grouped visiting order runs in every one of them
