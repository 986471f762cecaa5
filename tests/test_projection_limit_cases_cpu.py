"""The inputs of tests/projection_limit_cases.py are what tests/test_gpu_projection_limits.py says they are -- shown with the numpy
reference and the model of the tiers alone, no GPU:

(a), (b)  on this data the bounds AS CODED are sufficient (no bit a tier's model would decide has the wrong sign), at least 100 bits
          are traps (wrong-signed at more than 0.9 of the bound: a bound 10 % too small would set them wrongly) and at least as many
          lie just outside the bound, right-signed; the float-copy traps are undecided by the 16-bit tier's model; in the
          one-trap-per-word layout every other column is decided by it with a margin of two.
(c)       every engineered entry is within 4 ulps of a sign flip of the reference; fusing each multiply-add changes at least 10 % of
          the engineered bits, summing the counts of the large-plus-tiny cells in another order at least 8 of them.
(d)       the entry counts are 0..260; with the 24-bit counts no cell with a count qualifies for the integer form.

Every figure is printed (pytest -s); DESIGN.md 3.2 quotes them."""
import numpy as np
import pytest

import projection_limit_cases as cases


def tier2_k(case):
    """The (n + k) of the float-copy kernel that sees the engineered bits of a float-copy case."""
    L = case["L"]
    if L % 64 == 0:
        return 10.0 if "one-per-word" in case["name"] else 2.0
    return 8.0 if L % 32 == 0 else 2.0


@pytest.fixture(scope="module", params=cases.QUANTISATION_VARIANTS)
def quantisation(request):
    case = cases.quantisation_case(request.param)
    return case, cases.reference(case)[1], cases.model(case)


@pytest.fixture(scope="module", params=cases.FLOAT_COPY_LAYOUTS, ids=lambda p: "%s-%d" % p)
def float_copy(request):
    case = cases.float_copy_case(*request.param)
    return case, cases.reference(case)[1], cases.model(case)


@pytest.fixture(scope="module", params=cases.FLIP_WIDTHS)
def flip(request):
    case = cases.flip_case(request.param)
    return case, cases.reference(case)[1]


def words_a_smaller_bound_would_spoil(T, bound, sp, L):
    """(cell, word) pairs -- (cell, slice) or (cell, word) for the float first tiers -- in which a bound of 0.905 of the coded one leaves
    NO bit undecided although a bit is wrong-signed: nothing would be handed on, the wrong bit would stand."""
    width = 64 if L % 64 == 0 or L % 32 else 32
    cells = T.shape[0]
    ratio = np.full((cells, (L + width - 1) // width * width), np.inf)
    ratio[:, :L] = np.abs(T) / bound
    wrong = np.zeros(ratio.shape, dtype=bool)
    wrong[:, :L] = (T > 0.0) != (sp > 0.0)
    ratio, wrong = ratio.reshape(cells, -1, width), wrong.reshape(cells, -1, width)
    return int(((ratio > 0.905).all(axis=2) & wrong.any(axis=2)).sum())


# ---- (a) ----
def test_quantisation_form_and_shape(quantisation):
    case, sp, mdl = quantisation
    variant = case["name"].split("-", 1)[1]
    assert cases.first_tier(case) == ("fixed16-float" if variant == "half" else "fixed16-integer")
    assert mdl["integer"] == (variant != "half")
    toc = case["toc"]
    for c in range(len(toc) - 1):
        x = case["counts"][int(toc[c]):int(toc[c + 1])]
        assert (0.5 if variant == "half" else 1.0) in x.tolist()                         # the count that reaches any target
    # the float form's products count * q are exact: half-integers of few bits times 16-bit integers
    assert np.all(case["counts"] * 2 == np.trunc(case["counts"] * 2))
    ratio = np.abs(mdl["mean"][:, None] * mdl["S"][None, :]) / (0.501 * mdl["scale"][None, :] * mdl["absx"][:, None])
    print("%s: |mean| |S_i| over the quantisation term: median %.3g" % (case["name"], np.median(ratio)))
    if variant == "unbalanced":
        assert 0.3 < np.median(ratio) < 3.0
    else:
        assert ratio.max() < 1e-9


def test_quantisation_traps(quantisation):
    case, sp, mdl = quantisation
    s = cases.trap_statistics(mdl["T1"], mdl["bound1"], sp)
    print("%s: %d traps of %d bits, deepest %.4f of the bound, %d bits just outside it"
          % (case["name"], s["traps"], sp.size, s["depth"], s["outside"]))
    assert s["decided_wrong"] == 0
    assert s["traps"] >= 100 and s["depth"] > 0.93
    assert s["outside"] >= 100
    spoilt = words_a_smaller_bound_would_spoil(mdl["T1"], mdl["bound1"], sp, case["L"])
    print("%s: a bound of 0.905 of the coded one would leave %d words wrong with nothing handed on" % (case["name"], spoilt))
    assert spoilt >= 20
    # and the float tier behind it decides its own bits rightly too
    assert cases.trap_statistics(mdl["T2"], mdl["bound2"](2.0), sp)["decided_wrong"] == 0


def test_quantisation_sweep_covers_both_sides(quantisation):
    case, sp, mdl = quantisation
    t = mdl["T1"] / (0.501 * mdl["scale"][None, :] * mdl["absx"][:, None])
    assert t.min() < -1.4 and t.max() > 1.4
    wrong = (mdl["T1"] > 0.0) != (sp > 0.0)
    assert (wrong & (mdl["T1"] > 0.0)).sum() >= 50 and (wrong & (mdl["T1"] < 0.0)).sum() >= 50    # both directions of d


# ---- (b) ----
def test_float_copy_entries_are_what_the_copy_rounds(float_copy):
    case, sp, mdl = float_copy
    columns = case["trap_columns"]
    U = case["vectors"][:-1, columns]
    f = U.astype(np.float32).astype(np.float64)
    assert np.all(f != U)
    relative = np.abs(U - f) / np.abs(f) / cases.TWO24
    assert 0.979 < relative.min() and relative.max() < 0.981                            # 0.98 * 2^-24 from the float, every entry
    mantissa, exponent = np.frexp(np.abs(f))
    assert np.all((mantissa > 0.5) & (mantissa < 0.5 * 1.0025))                         # just above a power of two
    assert np.abs(mdl["S"][columns]).max() < 1e-9


def test_float_copy_traps(float_copy):
    case, sp, mdl = float_copy
    among = case["engineered"]
    bound = mdl["bound2"](tier2_k(case))
    s = cases.trap_statistics(mdl["T2"], bound, sp, among)
    print("%s: %d traps of %d engineered bits, deepest %.4f of the bound, %d bits just outside it"
          % (case["name"], s["traps"], among.sum(), s["depth"], s["outside"]))
    assert cases.trap_statistics(mdl["T2"], bound, sp)["decided_wrong"] == 0             # (every column, the random ones too)
    assert s["traps"] >= 100 and s["depth"] > 0.95
    assert s["outside"] >= 100
    spoilt = words_a_smaller_bound_would_spoil(mdl["T2"], bound, sp, case["L"])
    print("%s: a bound of 0.905 of the coded one would leave %d words or slices wrong with nothing handed on" % (case["name"], spoilt))
    assert spoilt >= 20
    if mdl["T1"] is not None:
        assert np.all((np.abs(mdl["T1"]) < mdl["bound1"])[s["trap_mask"]])
        assert np.all((np.abs(mdl["T1"]) < 0.999 * mdl["bound1"])[among])               # in fact every engineered bit is
        assert cases.trap_statistics(mdl["T1"], mdl["bound1"], sp)["decided_wrong"] == 0


def test_one_trap_per_word_leaves_single_bits():
    case = cases.float_copy_case("one-per-word", 1024)
    mdl = cases.model(case)
    assert [int(i) % 64 for i in case["trap_columns"][:5]] == [0, 7, 8, 56, 63]
    assert len(case["trap_columns"]) == 16 and np.array_equal(case["trap_columns"] // 64, np.arange(16))     # words 8..15: the second pass
    margin = (np.abs(mdl["T1"]) / mdl["bound1"])[~case["engineered"]].min()
    print("%s: the other columns are decided by the 16-bit tier's model with a margin of %.2f at the least" % (case["name"], margin))
    assert margin >= 2.0
    listed = cases.expected_listed(case, mdl)
    assert listed["words"] == (0, 0) and listed["bits"] == (48 * 16, 48 * 16)


# ---- (c) ----
def test_flip_entries_are_at_the_reference_flip(flip):
    case, sp = flip
    engineered = case["engineered"]
    assert engineered.sum() == case["L"] and np.all(engineered.sum(axis=0) == 1)        # every column engineered for one cell
    toc = case["toc"]
    for c in range(len(toc) - 1):
        assert case["genes"][int(toc[c])] == c                                           # the private gene comes first
        for i in np.nonzero(engineered[c])[0][:3]:
            assert cases.flip_cell_values(case, c, np.array([i]), case["vectors"][c, [i]])[0] == sp[c, i]
    distance = cases.flip_distance(case)
    assert distance[engineered].max() <= 4
    assert len(np.unique(case["ulps"])) == min(8, case["L"]) and case["ulps"].min() == -3 and case["ulps"].max() == 4
    # the bit is set on the far side of the flip -- mostly: within a few ulps of its cancellation point the sum is not monotonic
    agree = ((sp > 0.0)[engineered] == np.broadcast_to(case["ulps"] > 0, engineered.shape)[engineered]).mean()
    assert agree > 0.8 and 0.3 < (sp > 0.0)[engineered].mean() < 0.7
    assert np.any(case["counts"] != np.trunc(case["counts"]))


def test_a_fused_multiply_add_would_show(flip):
    case, sp = flip
    engineered = case["engineered"]
    changed = (cases.fused_bits(case) != (sp > 0.0)) & engineered
    share = changed.sum() / engineered.sum()
    print("%s: fusing every multiply-add changes %d of %d engineered bits (%.1f %%)" % (case["name"], changed.sum(), engineered.sum(), 100 * share))
    assert share >= 0.10


def test_another_order_of_the_cell_sum_would_show(flip):
    case, sp = flip
    cells = case["large_tiny_cells"]
    toc = case["toc"]
    for c in cells:
        x = case["counts"][int(toc[c]):int(toc[c + 1])].astype(np.float64)
        assert cases.cell_mean(x, 1) != np.sum(x[::-1])
    among = np.zeros_like(case["engineered"])
    among[cells] = case["engineered"][cells]
    changed = (cases.reordered_mean_bits(case) != (sp > 0.0)) & among
    print("%s: summing the counts in another order changes %d of %d engineered bits of the large-plus-tiny cells"
          % (case["name"], changed.sum(), among.sum()))
    assert changed.sum() >= 8
    mdl = cases.model(case)
    ratio = np.abs(mdl["mean"][:, None] * mdl["S"][None, :])[among] / np.abs(sp[among]).clip(1e-300)
    assert np.median(ratio) > 1e6                                                        # the mean term matters: it is what cancels


# ---- (d) ----
@pytest.mark.parametrize("variant", cases.ENTRY_COUNT_VARIANTS)
def test_entry_counts(variant):
    case = cases.entry_count_case(variant)
    assert np.array_equal(np.diff(case["toc"].astype(np.int64)), np.arange(261))
    assert case["gene_count"] == 300 and case["L"] == 128
    qualifies = cases.integer_form_cells(case["toc"], case["counts"])
    if variant == "integer":
        assert qualifies.all() and cases.first_tier(case) == "fixed16-integer"
    else:
        assert not qualifies[1:].any() and cases.first_tier(case) == "fixed16-float"    # (cell 0 has no count to disqualify it)
        bits = case["counts"].view(np.uint32)
        assert np.all(bits & 1 == 1)                                                     # the 24th mantissa bit is set
    mdl = cases.model(case)
    sp = cases.reference(case)[1]
    listed = cases.expected_listed(case, mdl)
    print("%s: of 261 cells x 2 words the model lists %s" % (case["name"], listed))
    # most cells reach the per-bit form with word 0 and the word form with word 1; the exact tier gets a part of them, not all
    assert listed["bits"][0] >= 200 and listed["words"][0] >= 200
    assert 50 <= listed["exact"][0] and listed["exact"][1] <= 400
    reached = np.diff(case["toc"].astype(np.int64))[(np.abs(mdl["T1"]) < 0.999 * mdl["bound1"])[:, 5]]
    assert {0, 8, 56, 57, 64, 120, 121, 128, 260} <= set(reached.tolist())                  # entry counts around the per-bit form's rounds
    assert cases.trap_statistics(mdl["T2"], mdl["bound2"](2.0), sp)["decided_wrong"] == 0
    assert 0.3 < (sp[1:] > 0.0).mean() < 0.7
