"""The values per cell of a list on the GPU (csrc/em2_cell_values.hip): em2_cell_similarities_to_cell bit-equal to
em2_matrix_compute_cell_similarity (host code, one pair) pair by pair and to the restatement
(tests/native/em2_draw_restatement.cpp, the reference's merge loop), and em2_gene_expression_of_cells bit-equal to column
localGene of getDenseExpressionMatrix(dtype=float32) and to the restatement.  NaNs must sit at the same places (their sign and
payload are the hardware's); everything else is compared bit for bit, with no tolerance.
70 cells (more than one wave, a partial last wave) x 40 genes; rows of 0, 1, 33 and, in a second store of 300 genes, 200 entries;
the gene as the first and as the last entry of a row and absent from it; a cell whose kept entries are all stored zeros; a gene
set that drops genes; a gene outside it; cellId0 inside and outside the list; a repeated id; one gene set too large for the
row vector's LDS home (the limit is the code's: em2_cell_similarities_row_in_lds)."""
import numpy as np
import pytest

import draw_binding as db
from expressionmatrix2_amd import ExpressionMatrix, capi, files

pytestmark = pytest.mark.gpu

CELLS = 70
GENE = 5                                   # the gene the column is taken of
DROPPED = (0, 3, 10, 39)


def rows_to_csr(rows):
    toc = np.zeros(len(rows) + 1, dtype=np.uint64)
    toc[1:] = np.cumsum([len(r[0]) for r in rows])
    data = np.zeros(int(toc[-1]), dtype=db.COUNT_DTYPE)
    data["gene"] = np.concatenate([np.asarray(r[0], dtype=np.uint32) for r in rows])
    data["count"] = np.concatenate([np.asarray(r[1], dtype=np.float32) for r in rows])
    return toc, data


def random_row(rng, genes, length):
    ids = np.sort(rng.choice(genes, size=length, replace=False))
    return ids, (rng.random(length) * 9. + 0.37).astype(np.float32)


def store_rows(genes, lengths, seed):
    rng = np.random.default_rng(seed)
    rows = [random_row(rng, genes, int(rng.integers(2, min(genes, 30)))) for _ in range(CELLS)]
    for cell, length in lengths.items():
        rows[cell] = random_row(rng, genes, length)
    return rng, rows


def planted_store():
    """40 genes.  Cell 0: no entry.  1: only the gene.  2: 33 entries.  4: zeros on kept genes, numbers on dropped ones.
    5: the gene first.  6: the gene last.  7: without the gene.  8: only dropped genes.  9: all 40 genes."""
    rng, rows = store_rows(40, {2: 33}, 21)
    rows[0] = (np.zeros(0, dtype=np.uint32), np.zeros(0, dtype=np.float32))
    rows[1] = ([GENE], [2.75])
    rows[4] = ([0, 1, 3, GENE, 9], [1.5, 0., 2.5, 0., 0.])
    rows[5] = ([GENE, 8, 20, 31], [1.25, 3.5, 0.7, 4.1])
    rows[6] = ([1, 2, 4, GENE], [2.2, 0.3, 5.9, 7.7])
    rows[7] = ([1, 2, 4, 6, 38], [1.1, 2.3, 0.9, 3.3, 1.7])
    rows[8] = ([0, 3, 39], [1., 2., 3.])
    rows[9] = (np.arange(40), (rng.random(40) * 5. + 0.1).astype(np.float32))
    return 40, rows


def long_store():
    """300 genes, rows of 200 entries among short ones (cells 3, 40 and 69), the gene in some of them."""
    _, rows = store_rows(300, {3: 200, 40: 200, 69: 200, 12: 1, 13: 33}, 22)
    return 300, rows


def scratch_gene_count():
    """The smallest gene count whose row vector does not fit LDS."""
    low, high = 1, 1 << 20
    assert capi.cell_similarities_row_in_lds(low) and not capi.cell_similarities_row_in_lds(high)
    while low + 1 < high:
        middle = (low + high) // 2
        if capi.cell_similarities_row_in_lds(middle):
            low = middle
        else:
            high = middle
    return high


class Store:
    def __init__(self, path, genes, rows, gene_set):
        self.genes, self.rows = genes, rows
        self.toc, self.data = rows_to_csr(rows)
        files.create_directory(path, genes, self.toc, self.data)
        self.gene_set = np.asarray(gene_set, dtype=np.uint32)
        files.add_gene_set(path, "Some", self.gene_set)
        self.matrix = ExpressionMatrix(path)
        self.local = {"AllGenes": None, "Some": np.full(genes, 0xffffffff, dtype=np.uint32)}
        self.local["Some"][self.gene_set] = np.arange(len(self.gene_set), dtype=np.uint32)
        self.sizes = {"AllGenes": genes, "Some": len(self.gene_set)}


@pytest.fixture(scope="module")
def restatement():
    return db.load()


@pytest.fixture(scope="module")
def stores(tmp_path_factory):
    root = tmp_path_factory.mktemp("values")
    genes, rows = planted_store()
    planted = Store(str(root / "planted"), genes, rows, [g for g in range(genes) if g not in DROPPED])
    genes, rows = long_store()
    long = Store(str(root / "long"), genes, rows, [g for g in range(genes) if g % 7 != 3])
    yield {"planted": planted, "long": long}
    planted.matrix.close()
    long.matrix.close()


def same_with_nans(got, expected, what):
    got, expected = np.asarray(got), np.asarray(expected)
    assert got.dtype == expected.dtype and got.shape == expected.shape, what
    assert np.array_equal(np.isnan(got), np.isnan(expected)), "%s: NaNs at other places" % what
    bits = np.uint64 if got.dtype == np.float64 else np.uint32
    keep = ~np.isnan(got)
    assert np.array_equal(got[keep].view(bits), expected[keep].view(bits)), what


def matrix_similarities(store, gene_set, cell0, ids):
    ids = np.ascontiguousarray(ids, dtype=np.uint32)
    out = np.zeros(len(ids), dtype=np.float64)
    capi.check(capi.load().em2_matrix_cell_similarities_to_cell(store.matrix._handle, gene_set.encode(), cell0, capi._ptr(ids), len(ids),
                                                                capi._ptr(out)))
    return out


def matrix_gene_expression(store, gene_set, gene, method, ids):
    ids = np.ascontiguousarray(ids, dtype=np.uint32)
    out = np.zeros(len(ids), dtype=np.float32)
    capi.check(capi.load().em2_matrix_gene_expression_of_cells(store.matrix._handle, gene_set.encode(), gene, method, capi._ptr(ids),
                                                               len(ids), capi._ptr(out)))
    return out


LISTS = {
    "all": list(range(CELLS)),                                   # cellId0 inside
    "without-cell0": [c for c in range(CELLS) if c not in (2, 9, 4)],
    "repeated": [9, 2, 9, 69, 0, 0, 4, 8, 9, 68, 1],
    "one": [7],
}


@pytest.mark.parametrize("which", ("planted", "long"))
@pytest.mark.parametrize("gene_set", ("AllGenes", "Some"))
def test_similarities_equal_the_host_pair_by_pair_and_the_restatement(stores, restatement, which, gene_set):
    store = stores[which]
    for cell0 in (2, 9, 4, 0, 8) if which == "planted" else (3, 12):
        for name, ids in LISTS.items():
            got = matrix_similarities(store, gene_set, cell0, ids)
            pairs = np.array([store.matrix.computeCellSimilarity(gene_set, cell0, c) for c in ids], dtype=np.float64)
            what = "%s %s cell0 %d list %s" % (which, gene_set, cell0, name)
            same_with_nans(got, pairs, what + " (host pairs)")
            same_with_nans(got, restatement.cell_similarities(store.toc, store.data, store.sizes[gene_set], cell0, ids,
                                                              store.local[gene_set]), what + " (restatement)")
            # the host form on the whole CSR, the gene set by its table
            same_with_nans(capi.cell_similarities_to_cell(store.toc, store.data, store.sizes[gene_set], cell0, ids,
                                                          store.local[gene_set]), got, what + " (host form)")
    if which == "planted":
        all_of = matrix_similarities(store, "Some", 2, LISTS["all"])
        assert np.isnan(all_of[0]) and np.isnan(all_of[8]) and np.isnan(all_of[4]) and not np.isnan(all_of[[1, 2, 5, 6, 7, 9]]).any()
        assert np.isnan(matrix_similarities(store, "Some", 8, LISTS["all"])).all()          # cell 0 of the call keeps nothing


@pytest.mark.parametrize("method", (0, 1, 2))
@pytest.mark.parametrize("which", ("planted", "long"))
@pytest.mark.parametrize("gene_set", ("AllGenes", "Some"))
def test_gene_column_equals_the_dense_matrix_and_the_restatement(stores, restatement, which, gene_set, method):
    store = stores[which]
    dense = store.matrix.getDenseExpressionMatrix(gene_set, "AllCells", method, dtype=np.float32)
    local = store.local[gene_set]
    genes = (GENE, 1, 38) if which == "planted" else (GENE, 0, 299, 151)
    for gene in genes:
        column = dense[:, gene if local is None else int(local[gene])]
        for name, ids in LISTS.items():
            got = matrix_gene_expression(store, gene_set, gene, method, ids)
            what = "%s %s gene %d method %d list %s" % (which, gene_set, gene, method, name)
            same_with_nans(got, np.ascontiguousarray(column[ids]), what + " (dense column)")
            same_with_nans(got, restatement.gene_expression(store.toc, store.data, gene, method, ids, local), what + " (restatement)")
            same_with_nans(capi.gene_expression_of_cells(store.toc, store.data, store.sizes[gene_set], gene, method, ids, local), got,
                           what + " (host form)")
    if which == "planted" and method != 0:
        got = matrix_gene_expression(store, "Some", GENE, method, LISTS["all"])
        assert np.isnan(got[4]) and got[0] == 0. and got[7] == 0. and got[8] == 0. and got[1] != 0. and got[5] != 0. and got[6] != 0.


def test_errors(stores):
    store = stores["planted"]
    lib = capi.load()
    ids = np.arange(3, dtype=np.uint32)
    out32, out64 = np.full(3, 7., dtype=np.float32), np.full(3, 7., dtype=np.float64)
    for gene in DROPPED + (40, 0xffffffff):                        # outside the gene set: the reference's assertion
        rc = lib.em2_matrix_gene_expression_of_cells(store.matrix._handle, b"Some", gene, 2, capi._ptr(ids), 3, capi._ptr(out32))
        assert rc not in (capi.EM2_OK, capi.EM2_ERROR_INVALID_ARGUMENT) and "localGeneId != invalidGeneId" in capi.last_error()
        with pytest.raises(RuntimeError, match="localGeneId != invalidGeneId"):
            capi.gene_expression_of_cells(store.toc, store.data, 36, gene, 2, ids, store.local["Some"])
    assert (out32 == 7.).all()
    bad = np.array([0, CELLS, 1], dtype=np.uint32)
    assert lib.em2_matrix_gene_expression_of_cells(store.matrix._handle, b"Some", GENE, 2, capi._ptr(bad), 3,
                                                   capi._ptr(out32)) == capi.EM2_ERROR_INVALID_ARGUMENT
    assert lib.em2_matrix_cell_similarities_to_cell(store.matrix._handle, b"Some", 0, capi._ptr(bad), 3,
                                                    capi._ptr(out64)) == capi.EM2_ERROR_INVALID_ARGUMENT
    assert lib.em2_matrix_cell_similarities_to_cell(store.matrix._handle, b"Some", CELLS, capi._ptr(ids), 3,
                                                    capi._ptr(out64)) == capi.EM2_ERROR_INVALID_ARGUMENT
    assert (out64 == 7.).all() and (out32 == 7.).all()
    with pytest.raises(RuntimeError, match="not below the cell count"):
        capi.cell_similarities_to_cell(store.toc, store.data, 40, 0, bad)
    with pytest.raises(RuntimeError, match="not below the cell count"):
        capi.gene_expression_of_cells(store.toc, store.data, 40, GENE, 1, bad)
    with pytest.raises(RuntimeError, match="Gene set Nope does not exist."):
        matrix_similarities(store, "Nope", 0, [0])
    with pytest.raises(RuntimeError, match="Invalid normalization method."):
        matrix_gene_expression(store, "Some", GENE, 3, [0])
    # an empty list is no error
    assert len(matrix_similarities(store, "Some", 0, [])) == 0 and len(matrix_gene_expression(store, "Some", GENE, 2, [])) == 0


def test_a_gene_set_too_large_for_lds_takes_the_global_scratch(restatement):
    genes = scratch_gene_count()
    assert capi.cell_similarities_row_in_lds(genes - 1) and not capi.cell_similarities_row_in_lds(genes)
    rng = np.random.default_rng(23)
    rows = [random_row(rng, genes, int(rng.integers(1, 40))) for _ in range(CELLS)]
    rows[0] = (np.zeros(0, dtype=np.uint32), np.zeros(0, dtype=np.float32))
    rows[1] = (np.array([0, genes - 1]), np.array([1.5, 2.5], dtype=np.float32))            # both ends of the row vector
    rows[2] = (np.array([0, 7, genes - 1]), np.array([3.25, 1., 0.75], dtype=np.float32))
    shared = np.sort(rng.choice(genes, size=300, replace=False))                              # so that the products are not all zero
    for cell in range(3, CELLS):
        ids = np.unique(np.concatenate([rows[cell][0], rng.choice(shared, size=25, replace=False)]))
        rows[cell] = (ids, (rng.random(len(ids)) * 4. + 0.3).astype(np.float32))
    toc, data = rows_to_csr(rows)
    # one gene set as large as the store, and the table of one that drops every fifth gene but is sized for LDS no more
    for local, size in ((None, genes), ):
        for cell0 in (1, 5, 0):
            for ids in (list(range(CELLS)), [2, 2, 69, 1]):
                got = capi.cell_similarities_to_cell(toc, data, size, cell0, ids, local)
                same_with_nans(got, restatement.cell_similarities(toc, data, size, cell0, ids, local), "scratch cell0 %d" % cell0)
    got = capi.cell_similarities_to_cell(toc, data, genes, 1, list(range(CELLS)))
    assert np.isnan(got[0]) and np.isfinite(got[1:]).all() and abs(got[1] - 1.) < 1e-12 and len(set(got[3:].tolist())) > 50
    # the same cells through the LDS home: a gene set of one gene fewer, the last gene dropped
    local = np.full(genes, 0xffffffff, dtype=np.uint32)
    local[:genes - 1] = np.arange(genes - 1, dtype=np.uint32)
    got = capi.cell_similarities_to_cell(toc, data, genes - 1, 2, list(range(CELLS)), local)
    same_with_nans(got, restatement.cell_similarities(toc, data, genes - 1, 2, list(range(CELLS)), local), "lds at the limit")


def test_device_entries_equal_the_host_forms_and_check_the_ids_themselves(stores):
    """Everything in device memory; a listed cell id not below the cell count is found by the kernel, not by the host."""
    import torch
    store = stores["planted"]
    lib = capi.load()
    d_toc = torch.from_numpy(store.toc.view(np.int64).copy()).cuda()
    d_data = torch.from_numpy(store.data.view(np.uint8).reshape(-1).copy()).cuda()
    d_local = torch.from_numpy(store.local["Some"].view(np.int32).copy()).cuda()
    ids = np.array(LISTS["repeated"], dtype=np.uint32)
    d_ids = torch.from_numpy(ids.view(np.int32).copy()).cuda()
    genes = store.sizes["Some"]
    bytes_needed = max(lib.em2_dev_cell_similarities_to_cell_workspace(genes, len(ids)), lib.em2_dev_gene_expression_of_cells_workspace())
    d_workspace = torch.zeros(bytes_needed, dtype=torch.uint8, device="cuda")
    d_similarity = torch.zeros(len(ids), dtype=torch.float64, device="cuda")
    d_column = torch.zeros(len(ids), dtype=torch.float32, device="cuda")

    def similarities(d_list, count):
        return lib.em2_dev_cell_similarities_to_cell(d_toc.data_ptr(), d_data.data_ptr(), CELLS, d_local.data_ptr(), 40, genes, 9,
                                                     d_list.data_ptr() if d_list is not None else None, count, d_similarity.data_ptr(),
                                                     d_workspace.data_ptr(), bytes_needed, None)

    def column(d_list, count, gene=GENE):
        return lib.em2_dev_gene_expression_of_cells(d_toc.data_ptr(), d_data.data_ptr(), CELLS, d_local.data_ptr(), 40, genes, gene, 2,
                                                    d_list.data_ptr() if d_list is not None else None, count, d_column.data_ptr(),
                                                    d_workspace.data_ptr(), bytes_needed, None)

    capi.check(similarities(d_ids, len(ids)))
    same_with_nans(d_similarity.cpu().numpy(), capi.cell_similarities_to_cell(store.toc, store.data, genes, 9, ids, store.local["Some"]),
                   "device similarities")
    capi.check(column(d_ids, len(ids)))
    same_with_nans(d_column.cpu().numpy(), capi.gene_expression_of_cells(store.toc, store.data, genes, GENE, 2, ids, store.local["Some"]),
                   "device column")
    # without a list: the cells 0 .. count - 1
    capi.check(similarities(None, len(ids)))
    same_with_nans(d_similarity.cpu().numpy(), capi.cell_similarities_to_cell(store.toc, store.data, genes, 9, np.arange(len(ids)),
                                                                              store.local["Some"]), "device similarities, no list")
    bad = ids.copy()
    bad[4] = CELLS
    d_bad = torch.from_numpy(bad.view(np.int32).copy()).cuda()
    assert similarities(d_bad, len(ids)) == capi.EM2_ERROR_INVALID_ARGUMENT and "not below the cell count" in capi.last_error()
    assert column(d_bad, len(ids)) == capi.EM2_ERROR_INVALID_ARGUMENT and "not below the cell count" in capi.last_error()
    assert column(d_ids, len(ids), gene=DROPPED[1]) not in (capi.EM2_OK, capi.EM2_ERROR_INVALID_ARGUMENT)
    assert similarities(None, CELLS + 1) == capi.EM2_ERROR_INVALID_ARGUMENT
    assert lib.em2_dev_cell_similarities_to_cell(d_toc.data_ptr(), d_data.data_ptr(), CELLS, d_local.data_ptr(), 40, genes, 9, d_ids.data_ptr(),
                                                 len(ids), d_similarity.data_ptr(), d_workspace.data_ptr(), 8, None) == capi.EM2_ERROR_INVALID_ARGUMENT
    capi.check(similarities(d_ids, len(ids)))                       # and the next call is right again
    same_with_nans(d_similarity.cpu().numpy(), capi.cell_similarities_to_cell(store.toc, store.data, genes, 9, ids, store.local["Some"]),
                   "device similarities after the errors")
