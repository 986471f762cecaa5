"""The bulk add on the GPU: em2_dev_ingest_count and em2_dev_ingest_fill against the restatement of addCell's storing part
(tests/native/em2_ingest_restatement.cpp) bit for bit -- counts, statuses, the reported gene, toc, the entries and the Cell
records as bytes, nothing discarded, no tolerance -- and ExpressionMatrix.addCellsFromCsr end to end."""
import numpy as np
import pytest

import dense_binding as db
import ingest_binding as ib
from expressionmatrix2_amd import ExpressionMatrix, capi, files
import expressionmatrix2_amd.expression_matrix as facade

pytestmark = pytest.mark.gpu

GENES = 9000                       # names in the batch; the gene map scatters them over a store that had some of them


@pytest.fixture(scope="module")
def torch():
    import torch
    capi.load()
    return torch


@pytest.fixture(scope="module")
def gene_map():
    """Not monotone: the store already had some of the genes, in another order."""
    return np.random.default_rng(5).permutation(GENES + 500).astype(np.uint32)[:GENES]


@pytest.fixture()
def lds_limit():
    """The LDS row limit for one test; the default comes back behind it."""
    yield capi.load().em2_set_ingest_lds_row_limit
    capi.load().em2_set_ingest_lds_row_limit(0)


def values_of(kind, n, rng):
    if kind == "integers":
        return rng.integers(1, 60, n).astype(np.float32)
    if kind == "fractions":                                  # magnitudes apart: the double sums depend on the order
        return (rng.random(n) * 10.0 ** rng.integers(-6, 7, n)).astype(np.float32) + np.float32(1e-3)
    if kind == "large":                                      # above 2^24: the float squares round
        return (rng.integers(2 ** 24 + 1, 2 ** 26, n)).astype(np.float32)
    raise ValueError(kind)


def row_of(length, rng, gene_map, order="shuffled", kind="integers"):
    """`length` entries of distinct genes, none zero."""
    index = rng.choice(len(gene_map), size=length, replace=False)
    by_gene = index[np.argsort(gene_map[index], kind="stable")]
    index = {"ascending": by_gene, "descending": by_gene[::-1], "shuffled": index}[order]
    return list(zip(index.tolist(), values_of(kind, length, rng).tolist()))


LENGTHS = [0, 1, 2, 63, 64, 65, 255, 256, 257, 1023, 1025]


@pytest.mark.parametrize("order", ["ascending", "descending", "shuffled"])
@pytest.mark.parametrize("kind", ["integers", "fractions", "large"])
def test_row_lengths_on_both_lds_paths(torch, gene_map, order, kind):
    """A wave for the rows up to 512 entries, a workgroup for 1023 and 1025, in one call."""
    rng = np.random.default_rng(11)
    rows = [row_of(n, rng, gene_map, order, kind) for n in LENGTHS]
    expected = ib.assert_same(torch, ib.Csr(rows), gene_map, "%s %s" % (order, kind))
    assert expected["kept"].tolist() == LENGTHS
    assert np.isinf(expected["cells"].view(ib.CELL_DTYPE)["norm1Inverse"][0])           # the empty cell: 1 / 0


def test_the_thresholds_between_the_kernels(torch, gene_map):
    """512 | 513: wave and workgroup; 8192 | 8193: LDS and global memory."""
    rng = np.random.default_rng(12)
    rows = [row_of(n, rng, gene_map, "shuffled", kind) for n in (512, 513, 8192, 8193) for kind in ("integers", "fractions")]
    ib.assert_same(torch, ib.Csr(rows), gene_map, "thresholds")


def test_the_fallback_with_a_small_limit(torch, gene_map, lds_limit):
    lds_limit(128)
    rng = np.random.default_rng(13)
    lengths = [127, 128, 129, 2049, 5, 0, 300]                # 129, 2049 and 300 in global memory, the others by a wave
    for kind in ("integers", "fractions", "large"):
        rows = [row_of(n, rng, gene_map, order, kind) for n in lengths for order in ("shuffled", "descending")]
        ib.assert_same(torch, ib.Csr(rows), gene_map, "limit 128 " + kind)
    lds_limit(600)                                            # the workgroup in LDS between 513 and 600, above it global memory
    rows = [row_of(n, rng, gene_map, "shuffled", "fractions") for n in (512, 513, 600, 601, 40)]
    ib.assert_same(torch, ib.Csr(rows), gene_map, "limit 600")


@pytest.mark.parametrize("cells", [1, 63, 65, 1025])
def test_cell_counts(torch, gene_map, cells):
    rng = np.random.default_rng(cells)
    rows = [row_of(int(n), rng, gene_map, "shuffled", "integers" if i % 2 else "fractions") for i, n in enumerate(rng.integers(0, 40, cells))]
    skip = (rng.random(cells) < 0.2).astype(np.uint8) if cells > 1 else None
    ib.assert_same(torch, ib.Csr(rows, skip), gene_map, "%d cells" % cells)


def test_zeros_nan_and_inf(torch, gene_map):
    rng = np.random.default_rng(14)
    base = row_of(70, rng, gene_map, "shuffled", "fractions")
    with_zeros = []
    for i, (index, value) in enumerate(base):                 # zeros and -0.0 between kept entries
        with_zeros.append((index, value))
        with_zeros.append((int(rng.integers(0, GENES)), 0.0 if i % 2 else -0.0))
    zero_duplicate = base[:10] + [(base[3][0], 0.0)] + base[10:] + [(base[3][0], -0.0)]          # no error: the zero is dropped first
    special = [(1, float("nan")), (2, 3.0), (3, float("inf")), (4, 0.0), (5, 1.5)]
    rows = [[(7, 0.0), (8, -0.0), (7, 0.0)], with_zeros, zero_duplicate, special, [(9, float("inf"))], [(9, float("nan"))],
            [(i, 0.0) for i in range(300)]]
    expected = ib.assert_same(torch, ib.Csr(rows), gene_map, "zeros")
    assert expected["kept"].tolist() == [0, 70, 70, 4, 1, 1, 0] and not expected["status"].any()


def test_sums_depend_on_the_order_and_follow_it(torch, gene_map):
    """The reversed row gives other bits in the restatement, so a device sum in another order could not pass by accident."""
    rng = np.random.default_rng(15)
    differing = 0
    for length in (40, 300, 700):
        row = row_of(length, rng, gene_map, "shuffled", "fractions")
        forward = ib.assert_same(torch, ib.Csr([row]), gene_map, "forward")
        backward = ib.assert_same(torch, ib.Csr([row[::-1]]), gene_map, "backward")
        assert forward["data"].tobytes() == backward["data"].tobytes()
        a, b = forward["cells"].view(ib.CELL_DTYPE), backward["cells"].view(ib.CELL_DTYPE)
        differing += int(a["sum1"].tobytes() != b["sum1"].tobytes() or a["sum2"].tobytes() != b["sum2"].tobytes())
    assert differing == 3
    # integers above 2^24 whose squares round as floats: few of them take the order-free path, many the sequential lane
    for length in (3, 8, 9, 400):
        ib.assert_same(torch, ib.Csr([row_of(length, rng, gene_map, "shuffled", "large")]), gene_map, "large %d" % length)
    mixed = row_of(100, rng, gene_map, "shuffled", "integers")
    mixed[50] = (mixed[50][0], 0.5)                           # one value that is no integer
    ib.assert_same(torch, ib.Csr([mixed]), gene_map, "one fraction among integers")


def error_rows(rng, gene_map):
    good = row_of(30, rng, gene_map)
    negative = good[:12] + [(good[12][0], -2.0)] + good[13:]
    low, high = sorted(good[:2], key=lambda e: gene_map[e[0]])
    duplicate = good + [(high[0], 5.0), (low[0], 7.0), (high[0], 1.0)]         # two duplicated genes: the smaller one is reported
    both = duplicate[:5] + [(good[20][0], -1.0)] + duplicate[5:]
    return good, negative, duplicate, both, int(gene_map[low[0]])


def test_errors_on_the_device(torch, gene_map, lds_limit):
    rng = np.random.default_rng(16)
    good, negative, duplicate, both, smallest = error_rows(rng, gene_map)
    long_duplicate = row_of(700, rng, gene_map)
    long_duplicate += [long_duplicate[3]]
    for limit in (0, 16):                                     # the LDS paths, then everything above 16 entries in global memory
        lds_limit(limit)
        csr = ib.Csr([good, negative, duplicate, both, good, negative, long_duplicate], skip=[0, 0, 0, 0, 0, 1, 0])
        expected = ib.assert_same(torch, csr, gene_map, "errors, limit %d" % limit)
        assert expected["status"].tolist() == [ib.OK, ib.NEGATIVE, ib.DUPLICATE, ib.NEGATIVE, ib.OK, ib.OK, ib.DUPLICATE]
        assert expected["duplicate"][2] == smallest and expected["duplicate"][3] == ib.NO_GENE
        assert expected["duplicate"][6] == gene_map[long_duplicate[3][0]]


def names(prefix, n):
    return ["%s%d" % (prefix, i) for i in range(n)]


def small_batch(rng, genes, cells, max_length=30):
    identity = np.arange(genes, dtype=np.uint32)
    return [row_of(int(n), rng, identity) for n in rng.integers(0, max_length, cells)]


def test_errors_through_the_facade_leave_the_files_unchanged(tmp_path, gene_map):
    rng = np.random.default_rng(17)
    identity = np.arange(GENES, dtype=np.uint32)
    good, negative, duplicate, both, smallest = error_rows(rng, identity)
    e = ExpressionMatrix.create(str(tmp_path / "store"))
    e.addGene("g5")                                           # the store has a gene of the batch: ids are not positions
    e.addCellsFromCsr(names("g", GENES), ["first"], [0, len(good)], [i for i, _ in good], np.asarray([v for _, v in good], np.float32), "p")
    e.flush()
    before = ib.file_bytes(e.directoryName)

    def attempt(rows, cell_names, text, data_type=np.float32, threshold=0., gene_names=None):
        csr = ib.Csr(rows)
        with pytest.raises(RuntimeError, match=text):
            e.addCellsFromCsr(gene_names or names("g", GENES) + ["new"], cell_names, csr.indptr, csr.indices, csr.values.astype(data_type),
                              "p", [("k", "v")], threshold)
        e.flush()
        assert ib.file_bytes(e.directoryName) == before, text

    attempt([good, negative], ["a", "b"], "Negative expression count encountered")
    gene_name = "g%d" % smallest
    attempt([good, duplicate], ["a", "b"], "Duplicate expression count for cell p-b gene %s$" % gene_name)
    attempt([good, both], ["a", "b"], "Negative expression count encountered")
    attempt([good, duplicate, negative], ["a", "b", "c"], "Duplicate expression count for cell p-b")       # the lower cell wins
    attempt([good, negative, duplicate], ["a", "b", "c"], "Negative expression count")
    attempt([negative, good], ["b", "first"], "Negative expression count")                # ... over a name that exists in a later cell
    attempt([good, negative], ["first", "b"], "Cell name p-first already exists")
    attempt([negative], ["first"], "Cell name p-first already exists")                    # within a cell the name comes first
    attempt([good, good], ["a", "a"], "Cell name p-a already exists")
    attempt([good], ["a"], "Duplicate gene name g7 in geneNames", gene_names=names("g", GENES) + ["g7"])
    # an error in a skipped barcode is ignored: integer data, a threshold above the small cell's sum
    tiny_negative_free = [(1, 1.0), (2, 1.0)]
    csr = ib.Csr([good, tiny_negative_free + [(2, 3.0)]])     # the second barcode has a duplicate and is skipped (sum 5 < 6)
    added = e.addCellsFromCsr(names("g", GENES), ["a", "b"], csr.indptr, csr.indices, csr.values.astype(np.int32), "p", [], 6.)
    assert list(added) == [1] and e.cellCount() == 2 and e.cellIdFromString("p-b") == facade.INVALID_ID
    with pytest.raises(RuntimeError):                         # EM2_ERROR_INVALID_ARGUMENT before any work
        e.addCellsFromCsr(["x"], ["c"], [0, 1], [1], np.ones(1, np.float32))
    with pytest.raises(RuntimeError, match="indptr"):
        capi.check(capi.load().em2_matrix_add_cells_csr(e._handle, b"x\0", 2, 1, b"c\0", 2, 1, capi._ptr(np.array([1, 1], np.uint64)), None, None,
                                                        0, None, b"", b"", 0, 0, 0, capi.ctypes.byref(capi.ctypes.c_uint32()),
                                                        capi.ctypes.byref(capi.ctypes.c_uint32())))
    assert e.geneIdFromName("x") == facade.INVALID_ID
    e.close()


def test_two_chunks_equal_one(tmp_path, monkeypatch):
    rng = np.random.default_rng(18)
    genes, cells = 200, 90
    csr = ib.Csr(small_batch(rng, genes, cells))
    stores = []
    for name, budget in (("one", 1 << 30), ("many", 4096)):
        monkeypatch.setattr(facade, "INGEST_CHUNK_BYTES", budget)
        e = ExpressionMatrix.create(str(tmp_path / name))
        e.addCellsFromCsr(names("g", genes), names("c", cells), csr.indptr, csr.indices, csr.values, "x", [("batch", "1")])
        e.close()
        stores.append(ib.read_store(str(tmp_path / name)))
    assert (int(csr.indptr[-1]) * 16 + cells * 96) // 4096 >= 5           # several chunks indeed
    assert stores[0] == stores[1]


def test_end_to_end(tmp_path, oracle):
    rng = np.random.default_rng(19)
    genes, cells = 300, 260
    rows = small_batch(rng, genes, cells, 60)
    rows[7] = [(3, 1.0)]                                      # total count 1: below the threshold
    csr = ib.Csr(rows)
    data = csr.values.astype(np.uint32)
    directory = str(tmp_path / "store")
    e = ExpressionMatrix.create(directory)
    added = e.addCellsFromCsr(names("gene", genes), names("bc", cells), csr.indptr, csr.indices, data, cellNamePrefix="run1",
                              cellMetaData=[("tissue", "lung"), ("donor", "d1")], totalExpressionCountThreshold=2.)
    kept_barcodes = [i for i in range(cells) if sum(v for _, v in rows[i]) >= 2.]
    assert 7 not in kept_barcodes and any(not r for r in rows) and len(kept_barcodes) > 200
    assert list(added) == list(range(len(kept_barcodes))) and e.cellCount() == len(kept_barcodes) and e.geneCount() == genes
    assert [e.geneName(g) for g in (0, 17, genes - 1)] == ["gene0", "gene17", "gene%d" % (genes - 1)]
    skip = np.ones(cells, np.uint8)
    skip[kept_barcodes] = 0
    expected = ib.restate(ib.Csr(rows, skip), np.arange(genes, dtype=np.uint32))
    entries = expected["data"].view(capi.COUNT_DTYPE)
    for cell, barcode in enumerate(kept_barcodes):
        assert e.getCellMetaData(cell) == [("CellName", "run1-bc%d" % barcode), ("tissue", "lung"), ("donor", "d1")]
        mine = entries[int(expected["toc"][barcode]):int(expected["toc"][barcode + 1])]
        assert e.getCellExpressionCounts(cell) == list(zip(mine["gene"].tolist(), mine["count"].tolist()))
        assert e.cellIdFromString("run1-bc%d" % barcode) == cell
    e.flush()
    store = ib.read_store(directory)
    records = np.frombuffer(store["cells"], dtype=ib.CELL_DTYPE)
    assert records.tobytes() == expected["cells"].view(ib.CELL_DTYPE)[kept_barcodes].tobytes()

    # getDenseExpressionMatrix L2 against the restatement's entries and norms
    toc = np.concatenate([[0], np.cumsum([int(expected["kept"][b]) for b in kept_barcodes])]).astype(np.uint64)
    flat = np.concatenate([entries[int(expected["toc"][b]):int(expected["toc"][b + 1])] for b in kept_barcodes])
    dense = e.getDenseExpressionMatrix(normalizationMethod=facade.NormalizationMethod.L2)
    theirs = db.load().dense_expression(toc, flat, genes, 2)
    assert db.dense_difference("L2 of the ingested store", dense, theirs) is None

    # findSimilarPairs4 at 128 bits equals the same matrix written by files.create_directory
    tool = str(tmp_path / "tool")
    files.create_directory(tool, genes, toc, flat)
    t = ExpressionMatrix(tool)
    for matrix in (e, t):
        matrix.findSimilarPairs4(similarPairsName="P", k=10, similarityThreshold=0.2, lshCount=128, seed=231)
    k0, pairs0, used0 = files.read_similar_pairs(directory, "P")
    k1, pairs1, used1 = files.read_similar_pairs(tool, "P")
    assert k0 == k1 and np.array_equal(used0, used1) and pairs0.tobytes() == pairs1.tobytes() and used0.sum() > 0
    t.close()

    # a second batch into the same store: overlapping genes in another order, new genes between them
    second_names = ["gene5", "extra0", "gene299", "gene0", "extra1", "gene150"]
    second = ib.Csr([[(0, 2.0), (1, 3.0), (3, 4.0)], [(5, 1.0), (4, 1.0), (2, 9.0)]])
    more = e.addCellsFromCsr(second_names, ["a", "b"], second.indptr, second.indices, second.values.astype(np.int64), "run2")
    assert list(more) == [len(kept_barcodes), len(kept_barcodes) + 1] and e.geneCount() == genes + 2
    assert e.geneIdFromName("extra0") == genes and e.geneIdFromName("extra1") == genes + 1
    assert e.getCellExpressionCounts(more[0]) == [(0, 4.0), (5, 2.0), (genes, 3.0)]
    assert e.getCellExpressionCounts(more[1]) == [(150, 1.0), (299, 9.0), (genes + 1, 1.0)]
    assert e.getDenseExpressionMatrix().shape == (len(kept_barcodes) + 2, genes + 2)
    e.close()
    again = ExpressionMatrix(directory)
    assert again.cellCount() == len(kept_barcodes) + 2 and again.getCellMetaData(more[1]) == [("CellName", "run2-b")]
    again.close()
