"""The signature projection where a sign is nearly undecidable (inputs: tests/projection_limit_cases.py; that they are what is
claimed: tests/test_projection_limit_cases_cpu.py).  Every case and width goes through the host entry, through the device entry with
the hyperplanes' auxiliary block (the tiers) and through the device entry without it (the exact arithmetic alone), and the signatures
must be identical to the numpy reference and to the oracle.  em2_dev_compute_signatures_tier must name the first tier the case means,
and em2_dev_compute_signatures_listed must report list lengths between what the model of the tiers is certain of and what it holds
possible -- so a case cannot pass without reaching the kernel it names.

(a) the 16-bit tier's value wrong-signed at up to 0.99 of its bound: a quantisation term below 0.501 scale sum|x| sets those bits
(b) the float copy's value wrong-signed at up to 0.97 of its bound, as words (projectionScreenItemsKernel), as single bits of a word
    (projectionScreenBitsKernel, every item of a chunk in one slice) and in both float first tiers (widths 96 and 100)
(c) entries within 4 ulps of the reference's own sign flip: a fused multiply-add or another order of the additions in the exact
    tier, or a cell mean that is not the sequential sum, changes bits
(d) 0..260 entries per cell: the parts, chunks and prefetches of the 16-bit tier and the rounds of the float tier's loops"""
import functools

import numpy as np
import pytest

import projection_limit_cases as cases
from expressionmatrix2_amd import capi

pytestmark = pytest.mark.gpu

CASES = ([("quantisation", v) for v in cases.QUANTISATION_VARIANTS] + [("float-copy",) + p for p in cases.FLOAT_COPY_LAYOUTS] +
         [("flip", L) for L in cases.FLIP_WIDTHS] + [("entry-counts", v) for v in cases.ENTRY_COUNT_VARIANTS])
EXPECTED_TIER = {("quantisation", "integer"): "fixed16-integer", ("quantisation", "half"): "fixed16-float",
                 ("quantisation", "unbalanced"): "fixed16-integer", ("float-copy", "all", 64): "fixed16-integer",
                 ("float-copy", "all", 1024): "fixed16-integer", ("float-copy", "one-per-word", 1024): "fixed16-integer",
                 ("float-copy", "all", 96): "float", ("float-copy", "all", 100): "float", ("flip", 1024): "fixed16-float",
                 ("flip", 96): "float", ("flip", 100): "float", ("flip", 63): "exact", ("entry-counts", "integer"): "fixed16-integer",
                 ("entry-counts", "mantissa24"): "fixed16-float"}


@functools.lru_cache(maxsize=None)
def prepared(key):
    """The case, the reference's words and values, the model -- computed once per case."""
    make = {"quantisation": cases.quantisation_case, "float-copy": cases.float_copy_case, "flip": cases.flip_case,
            "entry-counts": cases.entry_count_case}[key[0]]
    case = make(*key[1:])
    words, sp = cases.reference(case)
    return case, words, sp, cases.model(case)


def device_run(case, aux):
    """em2_dev_compute_signatures with or without the auxiliary block: (signatures, first tier, list lengths)."""
    import torch
    toc, genes, L = case["toc"], case["gene_count"], case["L"]
    cells = len(toc) - 1
    data = capi.make_counts(case["genes"], case["counts"])
    d_toc = torch.from_numpy(np.ascontiguousarray(toc).view(np.int64)).cuda()
    d_data = torch.from_numpy(np.ascontiguousarray(data).view(np.int64)).cuda()
    d_vectors = torch.from_numpy(np.ascontiguousarray(case["vectors"])).cuda()
    d_sig = torch.full((cells, capi.word_count(L)), 0x5a5a5a5a5a5a5a5a, dtype=torch.int64, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    d_aux = torch.empty(capi.dev_vector_aux_bytes(genes, L), dtype=torch.uint8, device="cuda")
    if aux:
        capi.dev_prepare_vectors(d_vectors.data_ptr(), genes, L, d_aux.data_ptr(), stream)
    ws_bytes = capi.dev_compute_signatures_workspace(cells, L)
    ws = torch.zeros(ws_bytes, dtype=torch.uint8, device="cuda")
    capi.dev_compute_signatures(d_toc.data_ptr(), d_data.data_ptr(), cells, genes, d_vectors.data_ptr(), d_aux.data_ptr() if aux else 0, L,
                                d_sig.data_ptr(), ws.data_ptr(), ws_bytes, stream)
    tier = capi.dev_compute_signatures_tier(ws.data_ptr(), cells, L, aux)
    listed = capi.dev_compute_signatures_listed(ws.data_ptr(), cells, L, aux)
    return d_sig.cpu().numpy().view(np.uint64), tier, listed


@pytest.mark.parametrize("key", CASES, ids=["-".join(str(part) for part in key) for key in CASES])
def test_signatures_tiers_and_lists(oracle, key):
    case, words, sp, mdl = prepared(key)
    toc, genes, counts, G, U, L = (case[k] for k in ("toc", "genes", "counts", "gene_count", "vectors", "L"))
    assert np.array_equal(oracle.compute_signatures(toc, genes, counts, G, U, L), words)
    assert np.array_equal(capi.compute_signatures(toc, capi.make_counts(genes, counts), G, U, L), words)
    exact, tier, listed = device_run(case, aux=False)
    assert np.array_equal(exact, words)
    assert tier == "exact" and listed == {"words": 0, "bits": 0, "exact": 0}
    got, tier, listed = device_run(case, aux=True)
    assert np.array_equal(got, words)
    assert tier == EXPECTED_TIER[key] == cases.first_tier(case)
    expected = cases.expected_listed(case, mdl)
    print("%s: listed %s, the model's certain and possible counts %s" % (case["name"], listed, expected))
    for name in ("words", "bits", "exact"):
        assert expected[name][0] <= listed[name] <= expected[name][1], name
    cells = len(toc) - 1
    engineered = np.zeros((cells, capi.word_count(L) * 64), dtype=bool)
    engineered[:, :L] = case["engineered"]
    engineered_words = int(engineered.reshape(cells, -1, 64).any(axis=2).sum())
    if key[0] == "quantisation":
        assert listed["words"] == cells                                     # every word holds many undecided bits
    if key[0] == "float-copy" and key[1] == "all" and L % 64 == 0:
        assert listed["words"] == engineered_words > 0 and listed["exact"] > 0
    if key[0] == "float-copy" and key[1] == "one-per-word":
        undecided = int(((np.abs(mdl["T1"]) < 0.999 * mdl["bound1"]) & case["engineered"]).sum())      # one trap per (cell, word)
        assert undecided == engineered_words == cells * 16
        assert listed["bits"] >= undecided and listed["words"] == 0
        assert 0 < listed["exact"] < listed["bits"]                         # the per-bit form decides some and leaves some
    if key[0] == "flip" and L % 4 == 0:
        assert listed["exact"] >= engineered_words
    if key[0] == "entry-counts":
        assert listed["bits"] >= 200 and listed["words"] >= 200 and 50 <= listed["exact"] <= 400
