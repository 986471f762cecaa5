"""em2_dev_ingest_count and em2_dev_ingest_fill where no feature test reaches them (the cases of tests/ingest_limit_cases.py, each
proven to reach its branch by tests/test_ingest_limit_cases_cpu.py), bit for bit against the restatement of addCell's storing
part (ingest_binding.assert_same); the two device guards, which the restatement does not have, by hand:

  I1  a block of the global-memory kernel takes a second row (1100 listed rows, 1024 blocks): the per-row reset of the smallest
      duplicated gene, the barrier before the next row, scratch of another length
  I2  the same for the LDS workgroup kernel (4200 listed rows, 4096 blocks): the buffer is reused behind a longer row
  I3  the same for the wave kernel (2^20 + 70 rows, 2^20 blocks): block i takes row i (512 entries) and row 2^20 + i (3 entries)
  I4  status 3: an index at or beyond indexCount, before anything is read from the map
  I5  the fill's check of d_outToc against the rows: every inner boundary moved by one, both ways
  I6  largest^2 * kept at 2^52, the switch between the parallel and the sequential sums

The issue's "2^22 copies of 2^15" is cut down to 2^12 copies of 2^20 (LDS kernel) and 2^16 copies of 2^18 (global memory): the
same product, rows the restatement sorts in milliseconds.  2^26 + 4 is no float (float32 rounds it to 2^26); its successor
2^26 + 8 stands next to it.  I3 runs three times: duplicates in the first rows, duplicates in the second rows, and none (the fill).

Wall time on an MI355X: 2.9 s for the 12 tests of this file (restatement included); I2, 2.3 million entries, 0.24 s; each I3
variant, 2^20 + 70 rows, 0.1 s.

Checked against mutated libraries (built outside the tree, selected with EM2_LIBRARY): the reset of sU32[8] only in a block's
first trip fails I1, I2 and I3 "first"; index <= indexCount fails all four I4 variants (the map's buffer has a guard behind it,
so the mutant read stays inside the buffer)."""
import numpy as np
import pytest

import ingest_binding as ib
import ingest_limit_cases as lc
from expressionmatrix2_amd import capi

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch():
    import torch
    capi.load()
    return torch


@pytest.fixture(scope="module")
def gene_map():
    return lc.gene_map()


@pytest.fixture()
def lds_limit():
    """The LDS row limit for one test; the default comes back behind it."""
    yield capi.load().em2_set_ingest_lds_row_limit
    capi.load().em2_set_ingest_lds_row_limit(0)


@pytest.mark.parametrize("case", ["i1", "i2"])
def test_a_workgroup_takes_a_second_row(torch, gene_map, lds_limit, case):
    build, limit = {"i1": (lc.i1, lc.I1_LIMIT), "i2": (lc.i2, lc.I2_LIMIT)}[case]
    lds_limit(limit)
    indptr, indices, values, plants = build(True)
    expected = ib.assert_same(torch, ib.Csr.from_arrays(indptr, indices, values), gene_map, case + ", duplicates planted")
    assert (expected["status"][plants["duplicate"]] == ib.DUPLICATE).all() and expected["status"].sum() == 2 * len(plants["duplicate"])
    indptr, indices, values, _ = build(False)
    expected = ib.assert_same(torch, ib.Csr.from_arrays(indptr, indices, values), gene_map, case + ", clean")
    assert not expected["status"].any() and int(expected["toc"][-1]) == len(values)


@pytest.mark.parametrize("variant", ["first", "swapped", "clean"])
def test_a_wave_takes_a_second_row(torch, gene_map, variant):
    indptr, indices, values, duplicate = lc.i3(variant)
    expected = ib.assert_same(torch, ib.Csr.from_arrays(indptr, indices, values), gene_map, "I3 " + variant)
    assert expected["status"].sum() == 2 * len(duplicate) and (expected["status"][duplicate] == ib.DUPLICATE).all()


@pytest.mark.parametrize("limit", [0, 16])
@pytest.mark.parametrize("told", ["the map's length", "less than the buffer holds"])
def test_an_index_outside_the_map_is_status_3(torch, gene_map, lds_limit, limit, told):
    lds_limit(limit)
    index_count = lc.GENES if told == "the map's length" else lc.GENES - 40
    rows = lc.i4_rows(index_count)
    csr = ib.Csr([entries for entries, _, _ in rows], skip=[skipped for _, skipped, _ in rows])
    got, _ = ib.device_count(torch, csr, gene_map, index_count=index_count)                # the guards are checked inside
    assert ib.BAD_INDEX == 3 and got["status"].tolist() == [status for _, _, status in rows]
    assert (got["duplicate"] == ib.NO_GENE).all()
    kept = [0 if skipped else sum(1 for _, value in entries if value != 0) for entries, skipped, _ in rows]
    assert got["kept"].tolist() == kept and got["toc"].tolist() == np.concatenate([[0], np.cumsum(kept)]).tolist()
    # the same rows with the bad indices put right: the restatement can follow, and everything is equal
    fixed = [[(index if index < index_count else (7 * i + 1) % index_count, value) for i, (index, value) in enumerate(entries)]
             for entries, _, _ in rows]
    good = [0, 3, 7, 9]
    ib.assert_same(torch, ib.Csr([fixed[i] for i in good], skip=[rows[i][1] for i in good]), gene_map, "I4, the rows without a bad index")


@pytest.mark.parametrize("limit", [0, 16])
def test_the_fill_checks_its_toc(torch, gene_map, lds_limit, limit):
    lds_limit(limit)
    indptr, indices, values = lc.i5()
    csr = ib.Csr.from_arrays(indptr, indices, values)
    expected = ib.assert_same(torch, csr, gene_map, "I5")     # the count pass's own toc: the fill succeeds
    entry_count = int(expected["toc"][-1])
    got, d = ib.device_count(torch, csr, gene_map)
    for boundary, shift, toc in lc.i5_moved_tocs(expected["toc"]):
        with pytest.raises(RuntimeError, match="d_outToc is not what the count pass gives for these rows"):
            ib.device_fill(torch, csr, d, entry_count, toc=toc)                            # the guards are checked before the answer
        data, cells = ib.device_fill(torch, csr, d, entry_count)                           # ... and the next correct call is whole
        assert np.array_equal(data, expected["data"]) and np.array_equal(cells, expected["cells"]), (boundary, shift)
    data, cells = ib.device_fill(torch, csr, d, entry_count, toc=expected["toc"])          # the override with the true toc
    assert np.array_equal(data, expected["data"]) and np.array_equal(cells, expected["cells"])


def test_the_sums_at_the_switch(torch):
    indptr, indices, values, genes = lc.i6()
    expected = ib.assert_same(torch, ib.Csr.from_arrays(indptr, indices, values), genes, "I6")
    assert not expected["status"].any()
    cells = expected["cells"].view(ib.CELL_DTYPE)
    assert cells["sum2"][0] == 2.0 ** 52 and np.isnan(cells["sum1"][15]) and np.isinf(cells["sum1"][14])
