"""findSimilarPairs0 on the GPU (em2_fsp0.hip) against the C++ restatement of
src/ExpressionMatrixFindSimilarPairs.cpp:16-99 (tests/native/em2_fsp0_restatement.cpp): every cell, bit for bit -- cell
ids, float similarity bits, usedCount, lowestSimilarityIndex and lowestSimilarity; no tolerance anywhere."""
import os

import numpy as np
import pytest

import expression_cases as ec
import fsp0_binding
import synth
from expressionmatrix2_amd import ExpressionMatrix, capi, files

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def restatement():
    return fsp0_binding.load()


def assert_equal(device, expected, label=""):
    pairs, used, low_index, low = device
    cell, sim, e_used, e_low_index, e_low = expected
    assert np.array_equal(used, e_used), label
    assert np.array_equal(pairs["cell"], cell), label
    assert np.array_equal(pairs["similarity"].view(np.uint32), sim.view(np.uint32)), label
    assert np.array_equal(low_index, e_low_index), label
    assert np.array_equal(low.view(np.uint32), e_low.view(np.uint32)), label


@pytest.mark.parametrize("cells,genes,density,k,thr,non_integer", [
    (700, 900, 0.03, 20, 0.2, False),
    (1000, 2000, 0.0125, 100, 0.2, False),       # the defaults; 1000 is no multiple of a batch of 256, 512 or 1024 columns
    (513, 300, 0.1, 7, -0.1, True),              # a threshold below zero: nearly every pair survives
    (300, 5000, 0.01, 50, 0.0, True),
    (257, 12000, 0.004, 10, 0.1, False),         # 512 threads per block
    (130, 30000, 0.002, 5, 0.05, True),          # 1024 threads per block
    (90, 36864, 0.001, 3, -1.0, False),          # the largest gene set the LDS form is sized for; threshold -1
    (260, 40000, 0.002, 12, 0.0, True),          # more genes than LDS holds: the global-memory form
    (50, 400, 0.1, 1000, -1.0, True),            # k larger than the cell count
    (2, 40, 0.5, 3, -1.0, False),
    (1, 40, 0.5, 3, 0.2, False),
    (400, 600, 0.05, 1, 0.1, True),
    (300, 600, 0.05, 0, 0.1, True),
])
def test_fsp0_equals_restatement(restatement, cells, genes, density, k, thr, non_integer):
    toc, data = fsp0_binding.clustered(cells, genes, density, seed=cells + k, cluster_count=6, non_integer=non_integer)
    expected = restatement.find_similar_pairs0(toc, data, genes, k, thr)
    assert_equal(capi.find_similar_pairs0(toc, data, genes, k, thr), expected)
    if k and cells > 2:
        assert expected[2].sum() > 0


def test_fsp0_global_form_with_more_rows_than_blocks(restatement):
    toc, data, genes = fsp0_binding.wide_matrix()
    expected = restatement.find_similar_pairs0(toc, data, genes, 12, 0.0)
    assert_equal(capi.find_similar_pairs0(toc, data, genes, 12, 0.0), expected)
    assert expected[2][1024:].sum() > 0                          # the rows a block takes second store pairs


@pytest.mark.parametrize("k,thr", [(3, -1.0), (4, 0.0), (5, 0.05), (2, 0.3)])
def test_fsp0_ties_at_the_eviction_boundary(restatement, k, thr):
    """Every cell 2-3 times, small k, low threshold: tests/test_fsp0_cpu.py::test_tie_input_is_not_a_plain_top_k shows that
    a plain top-k does not give this result."""
    toc, data, genes = fsp0_binding.duplicated_cells_input()
    assert_equal(capi.find_similar_pairs0(toc, data, genes, k, thr), restatement.find_similar_pairs0(toc, data, genes, k, thr))


def test_fsp0_empty_cell_constant_cell_and_stored_zeros(restatement):
    """An empty cell and a cell whose counts are constant over ALL genes have no variance: their similarities are NaN (or
    +-inf where the numerator rounds away from zero), IEEE decides, no pair is stored for NaN and nothing faults.  Stored
    zero counts take part in the products."""
    genes = 64
    toc, data = fsp0_binding.clustered(40, genes, 0.2, seed=9, cluster_count=2, non_integer=True)
    pieces = [data, np.zeros(0, dtype=fsp0_binding.COUNT_DTYPE),
              fsp0_binding.counts_of(np.arange(genes, dtype=np.uint32), np.full(genes, 2.5, dtype=np.float32)),
              fsp0_binding.counts_of(np.array([1, 5, 9, 30], dtype=np.uint32), np.array([0., 3., 0., 1.5], dtype=np.float32))]
    lengths = list(np.diff(toc.astype(np.int64))) + [0, genes, 4]
    toc2 = np.zeros(len(lengths) + 1, dtype=np.uint64)
    toc2[1:] = np.cumsum(lengths)
    data2 = np.concatenate(pieces)
    for k, thr in [(5, 0.1), (50, -1.0)]:
        expected = restatement.find_similar_pairs0(toc2, data2, genes, k, thr)
        device = capi.find_similar_pairs0(toc2, data2, genes, k, thr)
        assert_equal(device, expected)
        assert device[1][40] == 0                                 # the empty cell: every similarity is NaN


def test_fsp0_row_range_of_the_device_entry(restatement):
    import torch
    cells, genes, k, thr = 600, 800, 9, 0.1
    toc, data = fsp0_binding.clustered(cells, genes, 0.04, seed=77, cluster_count=5, non_integer=True)
    cell, sim, used, low_index, low = restatement.find_similar_pairs0(toc, data, genes, k, thr)
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).copy()).cuda()
    d_toc, d_data = d(toc), d(data)
    stream = torch.cuda.current_stream().cuda_stream
    for begin, end in [(0, cells), (100, 357), (599, 600), (256, 512)]:
        rows = end - begin
        ws_bytes = capi.dev_find_similar_pairs0_workspace(cells, rows, genes, k)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device="cuda")
        out_pairs = torch.empty(rows * k * 8, dtype=torch.uint8, device="cuda")
        out_used, out_index, out_low = (torch.empty(rows * 4, dtype=torch.uint8, device="cuda") for _ in range(3))
        capi.dev_find_similar_pairs0(d_toc.data_ptr(), d_data.data_ptr(), cells, genes, begin, end, k, thr, out_pairs.data_ptr(),
                                     out_used.data_ptr(), out_index.data_ptr(), out_low.data_ptr(), ws.data_ptr(), ws_bytes, stream)
        torch.cuda.synchronize()
        device = (out_pairs.cpu().numpy().view(capi.PAIR_DTYPE).reshape(rows, k), out_used.cpu().numpy().view(np.uint32),
                  out_index.cpu().numpy().view(np.uint32), out_low.cpu().numpy().view(np.float32))
        assert_equal(device, (cell[begin:end], sim[begin:end], used[begin:end], low_index[begin:end], low[begin:end]), (begin, end))


@pytest.mark.parametrize("cells,genes,density,k,thr,threads", [
    (1100, 12000, 0.004, 6, 0.0, 512),
    (2100, 30000, 0.002, 5, 0.0, 1024),
    (2100, 30000, 0.002, 300, -1.0, 1024),
])
def test_fsp0_second_and_third_batch_of_the_wider_blocks(restatement, cells, genes, density, k, thr, threads):
    """The 512- and the 1024-thread form with more cells than twice the threads: three column batches per row, the last one
    ragged, every row full after the first batch, so that the later batches replace (and, with k = 300, rescan 300 slots)."""
    form = ec.fsp0_form(cells, genes, k)
    assert form["in_lds"] and form["threads"] == threads and form["batches"] == 3
    toc, data = fsp0_binding.clustered(cells, genes, density, seed=cells + k, cluster_count=6, non_integer=True)
    expected = restatement.find_similar_pairs0(toc, data, genes, k, thr)
    assert (expected[2] == k).all()
    assert_equal(capi.find_similar_pairs0(toc, data, genes, k, thr), expected)


def slots_input(cells):
    """`cells` cells over 20 genes with about six non-integer counts each: thousands of candidates per cell at threshold -1 for next
    to no arithmetic."""
    toc, data = fsp0_binding.clustered(cells, 20, 0.3, seed=cells, cluster_count=6, non_integer=True)
    return toc, data, 20


@pytest.mark.parametrize("cells", [2060, 2300])
def test_fsp0_4096_slots_with_evictions(restatement, cells):
    """k = 2049, threshold -1: slotCapacity is 4096, every row takes all its candidates, those behind the 2049th against full
    slots, so the rescan after a replacement walks 2049 slots (33 per lane) and the bitonic sort runs over 4096 entries of which
    2047 are padding.  With 2060 cells a row sees 10 evictions, and slot 2048 never holds a row's minimum; with 2300 cells it sees
    250, and in half the rows (rows 0 to 6 among them) a rescan that stopped at slot 2047 would choose another slot.  The device
    computes all rows; the restatement, whose add() looks through the used slots at every offer (5 s and more for all rows),
    restates three ranges of 40 rows: the first rows, rows in the middle and the last rows."""
    k, thr = 2049, -1.0
    toc, data, genes = slots_input(cells)
    assert ec.fsp0_form(cells, genes, k)["slot_capacity"] == 4096
    device = capi.find_similar_pairs0(toc, data, genes, k, thr)
    assert (device[1] == k).all()
    for begin, end in [(0, 40), (cells // 2 - 20, cells // 2 + 20), (cells - 40, cells)]:
        expected = restatement.find_similar_pairs0(toc, data, genes, k, thr, rows=(begin, end))
        assert (expected[2] == k).all()
        assert_equal(tuple(a[begin:end] for a in device), expected, (begin, end))


@pytest.mark.parametrize("cells,k", [(4100, 4096), (4097, 5000)])
def test_fsp0_at_the_limit_of_support(restatement, cells, k):
    """min(k, cells - 1) = 4096 is the most the kernel holds.  4100 cells with k = 4096: every slot is used and three candidates
    meet full slots (a rescan over 4096 slots, a sort of 4096 without padding).  4097 cells with k = 5000: supported, since a cell
    has 4096 candidates; nothing is replaced and the 904 slots behind the used ones are zero.  The device entry on the first and
    the last rows against the ranged restatement."""
    toc, data, genes = slots_input(cells)
    form = ec.fsp0_form(cells, genes, k)
    assert form["supported"] and form["slot_capacity"] == 4096
    for begin, end in [(0, 8), (cells - 8, cells)]:
        expected = restatement.find_similar_pairs0(toc, data, genes, k, -1.0, rows=(begin, end))
        assert (expected[2] == 4096).all()
        assert_equal(ec.fsp0_device_rows(toc, data, genes, k, -1.0, begin, end), expected, (begin, end))


def test_fsp0_one_slot_more_is_not_supported():
    toc, data, genes = slots_input(4098)
    assert not ec.fsp0_form(4098, genes, 4097)["supported"]
    with pytest.raises(RuntimeError, match="not supported"):
        capi.find_similar_pairs0(toc, data, genes, 4097, -1.0)


@pytest.mark.parametrize("beyond", [0, 1])
@pytest.mark.parametrize("k", [1, 50])
def test_fsp0_at_the_lds_limit_next_to_its_own_lds(restatement, k, beyond):
    """The largest gene count whose row vector fits the 160 KiB of a workgroup NEXT TO the slots, the survivors and the state of
    fsp0RowsKernel (csrc/em2_expression.h rowVectorBytes, csrc/em2_fsp0.hip fsp0Lds, restated in tests/expression_cases.py), and
    one gene more, which takes the global-memory form: the workspace the library asks for grows by the row scratch exactly there."""
    cells = 130
    capacity = ec.slot_capacity(cells, k)
    own = ec.fsp0_own_lds_bytes(capacity)
    limit = ec.largest_gene_count_in_lds(own)
    assert capacity == (1 if k == 1 else 64) and ec.row_vector_bytes(limit) + own <= 160 * 1024 < ec.row_vector_bytes(limit + 1) + own
    small = capi.dev_find_similar_pairs0_workspace(cells, cells, 100, k)
    assert capi.dev_find_similar_pairs0_workspace(cells, cells, limit, k) == small
    scratch = capi.dev_find_similar_pairs0_workspace(cells, cells, limit + 1, k) - small
    assert 0 <= scratch - ec.row_vector_bytes(limit + 1) * cells < 256
    genes = limit + beyond
    assert ec.fsp0_form(cells, genes, k)["in_lds"] == (beyond == 0)
    toc, data = ec.lds_limit_input(cells, genes)
    expected = restatement.find_similar_pairs0(toc, data, genes, k, 0.0)
    assert expected[2].sum() > 0
    assert_equal(capi.find_similar_pairs0(toc, data, genes, k, 0.0), expected)


def test_fsp0_errors():
    toc, data = fsp0_binding.clustered(30, 50, 0.2, seed=2)
    with pytest.raises(RuntimeError, match="similarityThreshold <= 1"):
        capi.find_similar_pairs0(toc, data, 50, 3, 1.0000001)
    capi.find_similar_pairs0(toc, data, 50, 3, 1.0)                  # exactly 1 is allowed (CZI_ASSERT(similarityThreshold <= 1.))
    bad = data.copy()
    bad["gene"][5] = 50
    with pytest.raises(RuntimeError, match="not below geneCount"):
        capi.find_similar_pairs0(toc, bad, 50, 3, 0.2)
    unsorted = data.copy()
    first = int(toc[3])
    unsorted["gene"][first], unsorted["gene"][first + 1] = data["gene"][first + 1], data["gene"][first]
    with pytest.raises(RuntimeError, match="strictly ascending"):
        capi.find_similar_pairs0(toc, unsorted, 50, 3, 0.2)
    big_toc, big_data = fsp0_binding.clustered(4200, 20, 0.3, seed=2)
    with pytest.raises(RuntimeError, match="not supported"):
        capi.find_similar_pairs0(big_toc, big_data, 20, 4100, 0.2)


@pytest.fixture()
def data_dir(tmp_path):
    d = str(tmp_path / "data")
    cells, genes = 700, 900
    toc, data = fsp0_binding.clustered(cells, genes, 0.03, seed=21, cluster_count=5)
    files.create_directory(d, genes, toc, data)
    files.add_gene_set(d, "HighInformationGenes", np.unique((np.arange(300) * 7) % genes).astype(np.uint32))
    files.add_cell_set(d, "Subset", np.arange(3, cells, 2, dtype=np.uint32))
    files.add_gene_set(d, "NoGenes", np.zeros(0, dtype=np.uint32))
    files.add_cell_set(d, "NoCells", np.zeros(0, dtype=np.uint32))
    return d


def read_cell_info(directory, name):
    """SimilarPairs-<name>-CellInfo raw: a 256-byte header (objectCount at byte 16), then {usedCount, lowestSimilarityIndex,
    lowestSimilarity} per cell (src/SimilarPairs.hpp)."""
    raw = open(os.path.join(directory, "SimilarPairs-%s-CellInfo" % name), "rb").read()
    count = int(np.frombuffer(raw, dtype="<u8", count=1, offset=16)[0])
    records = np.frombuffer(raw, dtype=np.dtype([("used", "<u4"), ("index", "<u4"), ("lowest", "<f4")]), count=count, offset=256)
    return records


@pytest.mark.parametrize("gene_set,cell_set,k,thr", [("HighInformationGenes", "Subset", 12, 0.15), ("AllGenes", "AllCells", 100, 0.2)])
def test_facade_writes_the_three_files(restatement, data_dir, gene_set, cell_set, k, thr):
    e = ExpressionMatrix(data_dir)
    if (k, thr) == (100, 0.2):
        e.findSimilarPairs0(similarPairsName="Exact")                  # the binding's defaults
    else:
        e.findSimilarPairs0(geneSetName=gene_set, cellSetName=cell_set, similarPairsName="Exact", k=k, similarityThreshold=thr)
    for part in ("Info", "Pairs", "CellInfo"):
        assert os.path.exists(os.path.join(data_dir, "SimilarPairs-Exact-" + part))
    n_genes, toc, data = e._subset(gene_set, cell_set)
    cell, sim, used, low_index, low = restatement.find_similar_pairs0(toc, data, n_genes, k, thr)
    k2, pairs, used2 = files.read_similar_pairs(data_dir, "Exact")
    info = read_cell_info(data_dir, "Exact")
    assert k2 == k and files.similar_pairs_info(data_dir, "Exact")[2:] == (gene_set, cell_set)
    assert_equal((pairs, used2, info["index"], info["lowest"]), (cell, sim, used, low_index, low))
    assert np.array_equal(info["used"], used) and used.sum() > 0
    # usable downstream
    e.createCellGraph(graphName="G", cellSetName=cell_set, similarPairsName="Exact", similarityThreshold=0.3, k=5)
    assert len(e.getCellGraphEdges("G")) > 0
    # spot check with the host function, global ids
    ids = np.arange(700, dtype=np.uint32) if cell_set == "AllCells" else np.arange(3, 700, 2, dtype=np.uint32)
    c0 = int(np.argmax(used > 0))
    got = e.computeCellSimilarity(gene_set, int(ids[c0]), int(ids[cell[c0, 0]]))
    assert np.float32(got).view(np.uint32) == sim[c0, 0].view(np.uint32)


def test_facade_errors_use_the_reference_texts(data_dir):
    e = ExpressionMatrix(data_dir)
    for kwargs, text in [(dict(geneSetName="Nope"), "Gene set Nope does not exist."),
                         (dict(geneSetName="NoGenes"), "Gene set NoGenes is empty."),
                         (dict(cellSetName="Nope"), "Cell set Nope does not exist."),
                         (dict(cellSetName="NoCells"), "Cell set NoCells is empty."),
                         (dict(similarityThreshold=1.5), "similarityThreshold <= 1")]:
        with pytest.raises(RuntimeError, match=text):
            e.findSimilarPairs0(similarPairsName="X", **kwargs)
        assert not os.path.exists(os.path.join(data_dir, "SimilarPairs-X-Info"))
    with pytest.raises(TypeError):
        e.findSimilarPairs0()


def test_fsp0_20000_cells_every_row(restatement):
    """20 000 cells x 2 000 genes at density 0.0125 (the size SURVEY.md 6 probed the reference at), defaults k=100 and
    threshold 0.2: all rows, none sampled.  The restatement walks 2*10^8 pairs on one thread (about 40 s)."""
    cells, genes = 20000, 2000
    toc, data = fsp0_binding.clustered(cells, genes, 0.0125, cluster_count=64)
    device = capi.find_similar_pairs0(toc, data, genes, 100, 0.2)
    assert_equal(device, restatement.find_similar_pairs0(toc, data, genes, 100, 0.2))
    assert (device[1] == 100).sum() > cells // 2
