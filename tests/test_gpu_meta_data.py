"""The contingency table of two labelings on the GPU (csrc/em2_contingency.hip) against numpy's np.unique / np.bincount and
against tests/native/em2_meta_data_restatement.cpp -- every array and the three sums equal, on both paths wherever both apply
-- and the meta data methods that stand on it through the facade: computeMetaDataRandIndex bit for bit against the
restatement's dense table and computeRandIndex, the histograms' and the table's order, and the chain createClusterGraph ->
createMetaDataFromClusterGraph -> computeMetaDataRandIndex."""
import functools

import numpy as np
import pytest

import meta_data_binding as mb
import synth
from expressionmatrix2_amd import ExpressionMatrix, capi, files

pytestmark = pytest.mark.gpu

LDS, SORT = capi.CONTINGENCY_LDS, capi.CONTINGENCY_SORT


def random_ids(seed, n, n0, n1):
    """Skewed ids that reach n0 - 1 and n1 - 1 (where n allows), most values of a large range unused."""
    rng = np.random.default_rng(seed)
    id0 = np.minimum((rng.random(n) ** 2 * n0).astype(np.uint32), n0 - 1)
    id1 = ((id0 * 3 + rng.integers(0, max(1, n1 // 2 + 1), n)) % n1).astype(np.uint32)
    id0[-1], id1[-1] = n0 - 1, n1 - 1
    if n > 1:
        id0[0], id1[0] = 0, 0
    return id0, id1


# name -> (id0, id1, n0, n1); built once, never modified
@functools.lru_cache(maxsize=None)
def case(name):
    kind, *numbers = name.split("-")
    numbers = [int(x) for x in numbers]
    if kind == "n":                                             # n-<n>: a small table, n around the wave, the block, the slices
        out = random_ids(100 + numbers[0], numbers[0], 7, 5) + (7, 5)
    elif kind == "onecell":                                     # every element in one table cell: one counter takes them all
        n = numbers[0]
        out = (np.full(n, 2, dtype=np.uint32), np.full(n, 3, dtype=np.uint32), 5, 4)
    elif kind == "table":                                       # table-<n0>-<n1>-<n>
        n0, n1, n = numbers
        out = random_ids(200 + n0 + n1, n, n0, n1) + (n0, n1)
    elif kind == "singletons":                                  # singletons-<n>: n table cells of one element
        n = numbers[0]
        out = (np.random.default_rng(5).permutation(n).astype(np.uint32), (np.arange(n) % 3).astype(np.uint32), n, 3)
    else:
        raise ValueError(name)
    for a in out[:2]:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def expected(name):
    """The restatement's table of a named case, held against numpy's; computed once and shared."""
    id0, id1, n0, n1 = case(name)
    theirs = mb.load().contingency(id0, id1, n0, n1)
    mb.assert_same_contingency(theirs, mb.numpy_contingency(id0, id1, n0, n1), name + " (restatement against numpy)")
    return theirs


def paths_of(n0, n1):
    return (LDS, SORT) if n0 * n1 <= capi.CONTINGENCY_LDS_CELLS else (SORT,)


CASES = ["n-%d" % n for n in (1, 2, 63, 64, 65, 255, 256, 257, 1000, 70000)] + [
    "onecell-70000",                                            # count > 2^16, v (v - 1) > 2^32
    "table-1-1-1000",
    "table-128-128-70000", "table-145-113-70000",               # 16384 and 16385 cells: either side of the automatic choice
    "table-256-3-1000", "table-257-3-1000", "table-3-256-1000", "table-3-257-1000",      # the key's bit counts
    "table-65536-65537-1000", "table-65537-65536-1000", "table-65536-1-1000", "table-1-65537-1000",
    "singletons-1000",
]


@pytest.mark.parametrize("name", CASES)
def test_table_equals_numpy_and_the_restatement(name):
    id0, id1, n0, n1 = case(name)
    for path in paths_of(n0, n1):
        mine = capi.contingency(id0, id1, n0, n1, path)
        assert mine["path"] == path and mine["n"] == len(id0)
        mb.assert_same_contingency(mine, expected(name), "%s, path %d" % (name, path))
    automatic = capi.contingency(id0, id1, n0, n1)
    assert automatic["path"] == (LDS if n0 * n1 <= 16384 else SORT), name
    mb.assert_same_contingency(automatic, expected(name), name + ", automatic")


def test_the_shapes_are_what_they_are_meant_to_be():
    one = expected("onecell-70000")
    assert one["count"].tolist() == [70000] and one["sumCells"] == 70000 * 69999 > 2 ** 32
    assert case("table-128-128-70000")[2] * case("table-128-128-70000")[3] == 16384
    assert case("table-145-113-70000")[2] * case("table-145-113-70000")[3] == 16385
    assert len(expected("singletons-1000")["count"]) == 1000 and expected("singletons-1000")["sumCells"] == 0
    assert (expected("table-65536-65537-1000")["rowTotals"] == 0).sum() > 60000        # most ids are unused
    assert expected("table-65537-65536-1000")["rowTotals"][65536] >= 1


def test_the_lds_path_refuses_a_table_that_does_not_fit():
    id0, id1, n0, n1 = case("table-145-113-70000")
    with pytest.raises(RuntimeError, match="at most 16384 cells"):
        capi.contingency(id0, id1, n0, n1, LDS)
    with pytest.raises(RuntimeError, match="path must be"):
        capi.contingency(id0, id1, n0, n1, 3)
    with pytest.raises(RuntimeError, match="must be positive"):
        capi.contingency(id0, id1, 0, n1)
    empty = capi.contingency([], [], 3, 2)
    assert empty["rowTotals"].tolist() == [0, 0, 0] and len(empty["count"]) == 0 and empty["sumCells"] == 0


@pytest.mark.parametrize("path", [LDS, SORT])
@pytest.mark.parametrize("which", [0, 1])
def test_an_id_out_of_range_is_refused_and_the_next_call_is_correct(path, which):
    """An input check: the kernels test the id before they form an address with it and write nothing for that element."""
    name = "n-1000"
    id0, id1, n0, n1 = case(name)
    bad = [id0.copy(), id1.copy()]
    bad[which][-1] = (n0, n1)[which]                            # equal to its count, in the last position
    with pytest.raises(RuntimeError, match="an id is not below its count"):
        capi.contingency(bad[0], bad[1], n0, n1, path)
    mb.assert_same_contingency(capi.contingency(id0, id1, n0, n1, path), expected(name), "after the refused call")


@pytest.mark.parametrize("name", ["n-65", "n-70000", "table-128-128-70000", "table-145-113-70000", "singletons-1000"])
def test_device_entry_equals_the_host_entry(name):
    """Ids that are on the device already; a second time at an address that is not 16-byte aligned, which takes the LDS path's
    4-byte loads."""
    import torch
    id0, id1, n0, n1 = case(name)
    n = len(id0)
    device = torch.device("cuda")
    d0 = torch.from_numpy(np.concatenate([[0], id0]).astype(np.uint32).view(np.int32)).to(device)
    d1 = torch.from_numpy(np.concatenate([[0], id1]).astype(np.uint32).view(np.int32)).to(device)
    aligned0, aligned1 = d0[1:].clone(), d1[1:].clone()
    torch.cuda.synchronize()
    assert aligned0.data_ptr() % 16 == 0 and d0[1:].data_ptr() % 16 == 4
    for path in paths_of(n0, n1):
        mine = capi.dev_contingency(aligned0.data_ptr(), aligned1.data_ptr(), n, n0, n1, path)
        mb.assert_same_contingency(mine, expected(name), "%s on the device, path %d" % (name, path))
        shifted = capi.dev_contingency(d0[1:].data_ptr(), d1[1:].data_ptr(), n, n0, n1, path)
        mb.assert_same_contingency(shifted, expected(name), "%s on the device, unaligned, path %d" % (name, path))


def test_the_scratch_cache_is_only_a_cache():
    for name in ("table-145-113-70000", "n-2", "n-70000"):
        mb.assert_same_contingency(capi.contingency(*case(name)), expected(name), name)
    capi.load().em2_dev_release_scratch()
    for name in ("n-2", "table-145-113-70000"):
        mb.assert_same_contingency(capi.contingency(*case(name)), expected(name), name + " after the release")


# ---- through the facade ----

CELLS, GENES, TRUE_CLUSTERS, SEED = 3000, 600, 12, 77


class Both:
    """The facade and the restated store, written alike."""

    def __init__(self, matrix, store):
        self.e, self.r = matrix, store

    def set(self, cell, name, value):
        self.e.setCellMetaData(cell, name, value)
        self.r.set(cell, name, value)


@pytest.fixture(scope="module")
def both(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("meta") / "data")
    toc, g, c = synth.expression_matrix(CELLS, GENES, density=0.05, cluster_count=TRUE_CLUSTERS, seed=SEED)
    files.create_directory(d, GENES, toc, capi.make_counts(g, c))
    files.add_cell_set(d, "Subset", np.arange(0, CELLS, 3, dtype=np.uint32))
    files.add_cell_set(d, "Empty", np.zeros(0, dtype=np.uint32))
    b = Both(ExpressionMatrix(d), mb.load().store(CELLS))
    tissues = ["brain", "liver", "heart", "lung", "brain stem"]
    for cell in range(CELLS):
        b.set(cell, "Tissue", tissues[(cell * cell) % 5])
        b.set(cell, "Plate", "P%d" % ((cell // 7) % 11))
        # Holes: absent on a third of the cells, a stored "" on some, values on the others
        if cell % 3 != 1:
            b.set(cell, "Holes", "" if cell % 5 == 0 else "h%d" % (cell % 4))
    return b


def check_fields(b, cell_set_name, name0, name1):
    """computeMetaDataRandIndex, _meta_data_histogram and _meta_data_contingency_table against the restatement."""
    cells = b.e._cell_set(cell_set_name)
    theirs = b.r.table(cells, name0, name1)
    mine = b.e.computeMetaDataRandIndex(cell_set_name, name0, name1)
    assert [mb.double_bits(x) for x in mine] == [mb.double_bits(theirs["randIndex"]), mb.double_bits(theirs["adjustedRandIndex"])], (
        mine, theirs["randIndex"], theirs["adjustedRandIndex"])
    assert b.e._meta_data_histogram(cell_set_name, name0) == theirs["histogram0"] == b.r.table(cells, name0)["histogram0"]
    assert b.e._meta_data_histogram(cell_set_name, name1) == theirs["histogram1"]
    triples, histogram0, histogram1, path = b.e._meta_data_contingency_table(cell_set_name, name0, name1)
    assert histogram0 == theirs["histogram0"] and histogram1 == theirs["histogram1"]
    rows, columns = np.nonzero(theirs["dense"])
    assert triples == list(zip(rows.tolist(), columns.tolist(), theirs["dense"][rows, columns].tolist()))
    return mine, theirs, path


def test_rand_index_of_two_fields(both):
    mine, theirs, path = check_fields(both, "AllCells", "Tissue", "Plate")
    assert path == LDS and 0. < mine[0] < 1.
    assert [count for _, count in theirs["histogram0"]] == sorted((count for _, count in theirs["histogram0"]), reverse=True)
    assert both.e.computeMetaDataRandIndex(metaDataName0="Tissue", metaDataName1="Tissue") == (1.0, 1.0)    # cellSetName="AllCells"


def test_an_absent_field_and_a_stored_empty_string_are_one_value(both):
    mine, theirs, _ = check_fields(both, "AllCells", "Holes", "Tissue")
    values = dict(theirs["histogram0"])
    assert values[""] == sum(1 for cell in range(CELLS) if cell % 3 == 1 or cell % 5 == 0)
    assert both.e._meta_data_histogram("AllCells", "Holes")[0][0] == ""             # the most frequent value
    check_fields(both, "AllCells", "Tissue", "Holes")


def test_a_subset_cell_set(both):
    mine, _, _ = check_fields(both, "Subset", "Plate", "Holes")
    assert mine != both.e.computeMetaDataRandIndex("AllCells", "Plate", "Holes")


def test_the_reference_s_checks_in_its_order(both):
    e = both.e
    for call in (e.computeMetaDataRandIndex, e._meta_data_contingency_table):
        with pytest.raises(RuntimeError, match=r"^Cell set NoSuchSet not found\.$"):
            call("NoSuchSet", "NoSuchField", "Tissue")
        with pytest.raises(RuntimeError, match=r"^Meta data field NoSuchField not found\.$"):
            call("AllCells", "NoSuchField", "AlsoNot")
        with pytest.raises(RuntimeError, match=r"^Meta data field AlsoNot not found\.$"):
            call("AllCells", "Tissue", "AlsoNot")
        with pytest.raises(RuntimeError, match=r"rowCount > 0"):
            call("Empty", "Tissue", "Plate")
    with pytest.raises(TypeError):
        e.computeMetaDataRandIndex("AllCells", "Tissue")


def test_clusters_become_meta_data_and_are_judged_against_the_truth(both):
    """findSimilarPairs4 -> createCellGraph -> createClusterGraph -> createMetaDataFromClusterGraph -> computeMetaDataRandIndex."""
    e = both.e
    e.findSimilarPairs4(similarPairsName="P", k=20, similarityThreshold=0.2)
    e.createCellGraph("G", "AllCells", "P", similarityThreshold=0.3, k=10)
    _, labels = e.labelPropagationClustering("G")
    sizes = np.sort(np.bincount(labels))[::-1]
    assert len(sizes) > 4
    e.createClusterGraph("G", "C", minClusterSize=int(sizes[3]))      # about the four largest stay
    with pytest.raises(RuntimeError, match=r"^Cluster graph Nope does not exist\.$"):
        e.createMetaDataFromClusterGraph("Nope", "Cluster")
    e.createMetaDataFromClusterGraph("C", "Cluster")
    # the same writes, in the reference's order, into the restated store
    clustered = 0
    for cluster_id in e.getClusterGraphVertices("C"):
        for cell in e.getClusterCells("C", cluster_id):
            both.r.set(cell, "Cluster", str(cluster_id))
            clustered += 1
    unclustered = e._cluster_graph_unclustered_cells("C")
    for cell in unclustered:
        both.r.set(cell, "Cluster", "Unclustered-%d" % cell)
    assert clustered > 0 and len(unclustered) > 1400
    for cell in range(CELLS):
        assert e.getCellMetaData(cell) == both.r.pairs(cell), cell
    assert e.getCellMetaDataValue(unclustered[0], "Cluster") == "Unclustered-%d" % unclustered[0]
    assert e.computeMetaDataRandIndex("AllCells", "Cluster", "Cluster")[0] == 1.0
    check_fields(both, "AllCells", "Cluster", "Cluster")
    # the generator's clusters as a field
    truth = (synth.hash_u64(SEED, 11, np.arange(CELLS, dtype=np.uint64)) % np.uint64(TRUE_CLUSTERS)).tolist()
    for cell in range(CELLS):
        both.set(cell, "Truth", "T%d" % truth[cell])
    mine, theirs, path = check_fields(both, "AllCells", "Cluster", "Truth")
    # every unclustered cell has a value of its own: (clusters + unclustered cells) x 12 is past the LDS path's table
    assert len(theirs["histogram0"]) * len(theirs["histogram1"]) > capi.CONTINGENCY_LDS_CELLS and path == SORT
    assert mine[0] > 0.5
    # the clusters as a cell set for the next search
    e.createCellSetUsingMetaData("Cluster0", "Cluster", "0", False)
    assert e.getCellSet("Cluster0") == sorted(e.getClusterCells("C", 0)) == both.r.select("Cluster", "0", False)
    e.createCellSetUsingMetaData("Unclustered", "Cluster", "Unclustered-[0-9]+", True)
    assert e.getCellSet("Unclustered") == sorted(unclustered)
