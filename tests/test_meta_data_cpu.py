"""Cell meta data without a GPU: the store in the reference's file formats (read from, and replayed against, a store the
reference's own MemoryMapped::VectorOfLists and StringTable wrote: tests/golden/meta_data_reference), setCellMetaData,
getCellMetaData*, removeCellMetaData and createCellSetUsingMetaData against the C++ restatement
(tests/native/em2_meta_data_restatement.cpp), and the function that forms the two Rand indices from the three integer sums,
bit for bit against the restatement's computeRandIndex."""
import json
import math
import os
import shutil
import struct

import numpy as np
import pytest

import fsp0_binding
import meta_data_binding as mb
from expressionmatrix2_amd import ExpressionMatrix, capi, files

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "meta_data_reference")
STORE_FILES = ("CellMetaData.toc", "CellMetaData.data", "CellMetaData.freeSlots", "CellMetaDataNamesUsageCount",
               "CellMetaDataNames-strings.toc", "CellMetaDataNames-strings.data", "CellMetaDataNames-hashTable",
               "CellMetaDataValues-strings.toc", "CellMetaDataValues-strings.data", "CellMetaDataValues-hashTable")
OBJECT_SIZES = {"CellMetaData.toc": 8, "CellMetaData.data": 24, "CellMetaData.freeSlots": 8, "CellMetaDataNamesUsageCount": 4,
                "CellMetaDataNames-strings.toc": 4, "CellMetaDataNames-strings.data": 1, "CellMetaDataNames-hashTable": 4,
                "CellMetaDataValues-strings.toc": 4, "CellMetaDataValues-strings.data": 1, "CellMetaDataValues-hashTable": 4}
VECTOR_MAGIC = 0xa3756fd4b5d8bcc1
GENES = 12


@pytest.fixture(scope="module")
def restatement():
    return mb.load()


@pytest.fixture(scope="module")
def recorded():
    with open(os.path.join(GOLDEN, "calls_and_reads.json")) as f:
        return json.load(f)


def new_directory(path, cells):
    toc, data = fsp0_binding.clustered(cells, GENES, 0.3, seed=5, cluster_count=3, non_integer=True)
    files.create_directory(path, GENES, toc, data)
    return path


def raises(text, call, *arguments):
    with pytest.raises(RuntimeError) as error:
        call(*arguments)
    assert str(error.value) == text, str(error.value)


def header_and_objects(path):
    """(objectSize, objectCount, the bytes of the objects) of a MemoryMapped::Vector file, after the reference's open checks
    (src/MemoryMappedVector.hpp:497-499) and the bound on the count."""
    raw = open(path, "rb").read()
    header_size, object_size, object_count, page_count, file_size, capacity, magic = struct.unpack("<7Q", raw[:56])
    assert magic == VECTOR_MAGIC and file_size == len(raw) and header_size == 256, path
    assert 256 + object_size * object_count <= len(raw) and object_count <= capacity, path
    return object_size, object_count, raw[256:256 + object_size * object_count]


def replay(matrix, calls):
    for i, call in enumerate(calls):
        if call[0] == "set":
            matrix.setCellMetaData(call[1], call[2], call[3])
        else:
            matrix.createCellSet("Removal%d" % i, call[1])
            matrix.removeCellMetaData("Removal%d" % i, call[2])


def test_symbols_are_declared():
    for name in ("em2_matrix_set_cell_meta_data", "em2_matrix_get_cell_meta_data_value", "em2_matrix_get_cell_meta_data",
                 "em2_matrix_remove_cell_meta_data", "em2_matrix_create_cell_set_using_meta_data",
                 "em2_matrix_compute_meta_data_rand_index", "em2_matrix_meta_data_table", "em2_meta_data_table_sizes",
                 "em2_meta_data_table_get", "em2_meta_data_table_free", "em2_matrix_flush", "em2_tool_create_meta_data",
                 "em2_contingency_create", "em2_dev_contingency", "em2_contingency_sizes", "em2_contingency_get",
                 "em2_contingency_free", "em2_rand_index"):
        assert name in capi.SYMBOLS and hasattr(capi.load(), name)
    for method in ("setCellMetaData", "getCellMetaDataValue", "getCellMetaData", "getCellsMetaData", "removeCellMetaData",
                   "createCellSetUsingMetaData", "createMetaDataFromClusterGraph", "computeMetaDataRandIndex",
                   "_meta_data_histogram", "_meta_data_contingency_table"):
        assert callable(getattr(ExpressionMatrix, method))


# ---- the reference's own files ----

def test_the_reference_store_reads_as_recorded(tmp_path, recorded):
    d = new_directory(str(tmp_path / "data"), recorded["cellCount"])
    for name in STORE_FILES:
        shutil.copy(os.path.join(GOLDEN, name), os.path.join(d, name))
    e = ExpressionMatrix(d)
    for cell, pairs in enumerate(recorded["cells"]):
        assert e.getCellMetaData(cell) == [tuple(p) for p in pairs], cell
        for name in recorded["usageCounts"]:
            expected = next((value for n, value in pairs if n == name), "")
            assert e.getCellMetaDataValue(cell, name) == expected, (cell, name)
        assert e.getCellMetaDataValue(cell, "NoSuchField") == ""
    assert e.getCellsMetaData([9, 0]) == [[tuple(p) for p in recorded["cells"][c]] for c in (9, 0)]
    before = {name: open(os.path.join(d, name), "rb").read() for name in STORE_FILES}
    e.close()                                                   # nothing was written: the files stay as they were
    assert before == {name: open(os.path.join(d, name), "rb").read() for name in STORE_FILES}


def test_replaying_the_calls_writes_the_reference_files(tmp_path, recorded):
    d = new_directory(str(tmp_path / "data"), recorded["cellCount"])
    capi.check(capi.load().em2_tool_create_meta_data(d.encode(), recorded["cellCount"], recorded["nameCapacity"],
                                                     recorded["valueCapacity"]))
    e = ExpressionMatrix(d)
    replay(e, recorded["calls"])
    for cell, pairs in enumerate(recorded["cells"]):
        assert e.getCellMetaData(cell) == [tuple(p) for p in pairs], cell
    e.close()
    for name in STORE_FILES:
        ours = header_and_objects(os.path.join(d, name))
        theirs = header_and_objects(os.path.join(GOLDEN, name))
        assert ours[0] == theirs[0] == OBJECT_SIZES[name], name
        assert ours[1] == theirs[1], "%s: %d objects, the reference wrote %d" % (name, ours[1], theirs[1])
        assert ours[2] == theirs[2], name + ": the objects differ from the reference's"
    # both string tables doubled on the way (8 -> 32 and 8 -> 64), and freed slots were reused
    assert [header_and_objects(os.path.join(d, "CellMetaData%s-hashTable" % t))[1] for t in ("Names", "Values")] == recorded["finalCapacities"]
    assert recorded["finalCapacities"] == [32, 64]
    assert header_and_objects(os.path.join(d, "CellMetaData.freeSlots"))[1] > 0


def test_a_damaged_store_is_an_io_error(tmp_path, recorded):
    d = new_directory(str(tmp_path / "data"), recorded["cellCount"])
    for name in STORE_FILES:
        shutil.copy(os.path.join(GOLDEN, name), os.path.join(d, name))
    path = os.path.join(d, "CellMetaData.data")
    raw = bytearray(open(path, "rb").read())
    # node 0 is the end node of cell 0: its `next` leaves the node store
    struct.pack_into("<Q", raw, 256 + 16, 1 << 40)
    open(path, "wb").write(bytes(raw))
    e = ExpressionMatrix(d)
    with pytest.raises(RuntimeError, match="The cell meta data store is damaged"):
        e.getCellMetaData(0)
    assert e.getCellMetaData(1) == [tuple(p) for p in recorded["cells"][1]]
    # a list that does not come back to its end node: cell 1's end node points at itself through node 2 <-> 2
    raw = bytearray(open(os.path.join(GOLDEN, "CellMetaData.data"), "rb").read())
    first = struct.unpack_from("<Q", raw, 256 + 24 * 1 + 16)[0]
    struct.pack_into("<Q", raw, 256 + 24 * first + 16, first)
    open(path, "wb").write(bytes(raw))
    e2 = ExpressionMatrix(d)
    with pytest.raises(RuntimeError, match="does not come back to its end node"):
        e2.getCellMetaData(1)


# ---- the methods ----

CELLS = 40


def filled(tmp_path, restatement):
    """A tool-made directory (no store) and the restated store, filled alike: Tissue on most cells, Plate on some."""
    e = ExpressionMatrix(new_directory(str(tmp_path / "data"), CELLS))
    r = restatement.store(CELLS)
    tissues = ["brain", "liver", "heart", "brain stem", "", "Brain"]
    for cell in range(CELLS):
        if cell % 7 != 3:                                       # (some cells lack the field)
            for s in (e, r):
                (s.setCellMetaData if s is e else s.set)(cell, "Tissue", tissues[(cell * 5) % 6])
        if cell % 3 == 0:
            for s in (e, r):
                (s.setCellMetaData if s is e else s.set)(cell, "Plate", "P%d" % (cell % 4))
    return e, r


def same_store(e, r):
    for cell in range(CELLS):
        assert e.getCellMetaData(cell) == r.pairs(cell), cell
        for name in ("Tissue", "Plate", "Other", "NoSuchField"):
            assert e.getCellMetaDataValue(cell, name) == r.value(cell, name), (cell, name)


def usage_counts(directory):
    """{name: count} from the files."""
    _, count, toc = header_and_objects(os.path.join(directory, "CellMetaDataNames-strings.toc"))
    _, _, data = header_and_objects(os.path.join(directory, "CellMetaDataNames-strings.data"))
    _, usage_count, usage = header_and_objects(os.path.join(directory, "CellMetaDataNamesUsageCount"))
    offsets = struct.unpack("<%dI" % count, toc)
    assert usage_count == count - 1
    return {data[offsets[i]:offsets[i + 1]].decode(): struct.unpack_from("<I", usage, 4 * i)[0] for i in range(count - 1)}


def test_a_directory_without_a_store(tmp_path):
    e = ExpressionMatrix(new_directory(str(tmp_path / "data"), CELLS))
    assert e.getCellMetaData(0) == [] and e.getCellMetaDataValue(CELLS - 1, "Tissue") == ""
    assert e.removeCellMetaData("AllCells", "Tissue") is None
    e.createCellSetUsingMetaData("Nobody", "Tissue", ".*", True)
    assert e.getCellSet("Nobody") == []
    raises("Meta data field Tissue not found.", e.computeMetaDataRandIndex, "AllCells", "Tissue", "Tissue")
    e.close()
    assert not any(name.startswith("CellMetaData") for name in os.listdir(e.directoryName))      # reads create nothing
    with pytest.raises(RuntimeError, match="not below the cell count"):
        ExpressionMatrix(e.directoryName).setCellMetaData(CELLS, "Tissue", "brain")


def test_set_replaces_or_appends_and_survives_reopening(tmp_path, restatement):
    e, r = filled(tmp_path, restatement)
    same_store(e, r)
    assert e.getCellMetaData(0) == [("Tissue", "brain"), ("Plate", "P0")]
    for s in (e, r):
        put = s.setCellMetaData if s is e else s.set
        put(0, "Tissue", "spleen")                              # replaced in place: the list keeps its order
        put(0, "Other", "x")                                    # appended
        put(3, "Tissue", "brain")                               # a cell that lacked the field
    assert e.getCellMetaData(0) == [("Tissue", "spleen"), ("Plate", "P0"), ("Other", "x")]
    same_store(e, r)
    e.close()
    counts = usage_counts(e.directoryName)
    assert counts == {name: r.usage(name) for name in ("Tissue", "Plate", "Other")}
    assert counts["Other"] == 1 and counts["Plate"] == len(range(0, CELLS, 3))
    # the lazily created tables: 1 << 12 slots each, and files the reference's open checks accept
    for name in STORE_FILES:
        assert header_and_objects(os.path.join(e.directoryName, name))[0] == OBJECT_SIZES[name]
    assert header_and_objects(os.path.join(e.directoryName, "CellMetaDataValues-hashTable"))[1] == 1 << 12
    assert header_and_objects(os.path.join(e.directoryName, "CellMetaData.toc"))[1] == CELLS
    e2 = ExpressionMatrix(e.directoryName)
    same_store(e2, r)
    e2.setCellMetaData(1, "Other", "y")
    r.set(1, "Other", "y")
    e2.flush()
    same_store(ExpressionMatrix(e.directoryName), r)


def test_the_string_table_grows_past_its_first_capacity(tmp_path, restatement):
    e = ExpressionMatrix(new_directory(str(tmp_path / "data"), CELLS))
    r = restatement.store(CELLS)
    for i in range(2100):                                       # more than (1 << 12) / 2 values: one doubling
        e.setCellMetaData(i % CELLS, "Field%d" % (i % 3), "value-%d" % i)
        r.set(i % CELLS, "Field%d" % (i % 3), "value-%d" % i)
    e.close()
    assert header_and_objects(os.path.join(e.directoryName, "CellMetaDataValues-hashTable"))[1] == 1 << 13
    e2 = ExpressionMatrix(e.directoryName)
    for cell in range(CELLS):
        assert e2.getCellMetaData(cell) == r.pairs(cell)


def test_remove_cell_meta_data(tmp_path, restatement):
    e, r = filled(tmp_path, restatement)
    e.setCellMetaData(6, "Tissue2", "a")                        # cell 6: Tissue, Plate, Tissue2
    r.set(6, "Tissue2", "a")
    some = [0, 3, 6, 9, 10, 39]
    e.createCellSet("Some", some)
    raises("Cell set NoSuchSet not found.", e.removeCellMetaData, "NoSuchSet", "Tissue")
    assert e.removeCellMetaData("Some", "NoSuchField") is None  # an unknown name: nothing happens
    same_store(e, r)
    e.removeCellMetaData("Some", "Plate")
    r.remove(some, "Plate")
    same_store(e, r)
    assert e.getCellMetaData(6) == [("Tissue", r.value(6, "Tissue")), ("Tissue2", "a")]       # the first node of that name only
    assert e.getCellMetaData(12) == r.pairs(12) and ("Plate", "P0") in e.getCellMetaData(12)   # outside the set: untouched
    e.flush()
    assert usage_counts(e.directoryName)["Plate"] == r.usage("Plate") == len(range(0, CELLS, 3)) - 5     # 0, 3, 6, 9, 39
    _, free_before, slots = header_and_objects(os.path.join(e.directoryName, "CellMetaData.freeSlots"))
    _, nodes_before, _ = header_and_objects(os.path.join(e.directoryName, "CellMetaData.data"))
    assert free_before == 5
    last_freed = struct.unpack_from("<Q", slots, 8 * 4)[0]
    e.setCellMetaData(20, "New", "n")                           # takes the slot freed last; the node store does not grow
    r.set(20, "New", "n")
    e.flush()
    _, free_after, _ = header_and_objects(os.path.join(e.directoryName, "CellMetaData.freeSlots"))
    _, nodes_after, nodes = header_and_objects(os.path.join(e.directoryName, "CellMetaData.data"))
    assert (free_after, nodes_after) == (4, nodes_before)
    name_id, value_id, previous, following = struct.unpack_from("<IIQQ", nodes, 24 * last_freed)
    assert following == 20                                      # the new node is the last of cell 20's list: next = its end node
    same_store(e, r)
    # removing everything, then writing again
    e.removeCellMetaData("AllCells", "Tissue")
    r.remove(list(range(CELLS)), "Tissue")
    same_store(e, r)
    e.flush()
    assert usage_counts(e.directoryName)["Tissue"] == 0 == r.usage("Tissue")


@pytest.mark.parametrize("match, use_regex", [
    ("brain", False), ("brain", True), ("Brain", False), ("", False), ("", True), ("bra", False),
    ("bra", True),                                              # matches a part of "brain" only: regex_match must not select
    ("bra.*", True), ("brain( stem)?", True), ("[bB]rain", True), (".*", True), ("liver|heart", True), ("b.*n", False),
    ("NoSuchValue", False),
])
def test_create_cell_set_using_meta_data(tmp_path, restatement, match, use_regex):
    e, r = filled(tmp_path, restatement)
    e.createCellSetUsingMetaData("Selected", "Tissue", match, use_regex)
    expected = r.select("Tissue", match, use_regex)
    assert e.getCellSet("Selected") == expected
    if (match, use_regex) == ("bra", True):
        assert expected == []
    if (match, use_regex) == (".*", True):
        assert expected == [c for c in range(CELLS) if c % 7 != 3]           # the cells without the field stay out
    if (match, use_regex) == ("", False):
        assert expected == [c for c in range(CELLS) if c % 7 != 3 and (c * 5) % 6 == 4]   # a stored "", not an absent field
    # the file is what createCellSet writes for the same cells
    e.createCellSet("ByHand", expected)
    read = lambda name: open(os.path.join(e.directoryName, "CellSet-" + name), "rb").read()
    assert read("Selected") == read("ByHand")


def test_create_cell_set_using_meta_data_checks(tmp_path, restatement):
    e, r = filled(tmp_path, restatement)
    raises("Cell set AllCells already exists.", e.createCellSetUsingMetaData, "AllCells", "Tissue", "(", True)   # the name first
    assert r.select("Tissue", "(", True) is None
    with pytest.raises(RuntimeError):
        e.createCellSetUsingMetaData("Bad", "Tissue", "(", True)
    assert "Bad" not in e.getCellSetNames() and not os.path.exists(os.path.join(e.directoryName, "CellSet-Bad"))
    e.createCellSetUsingMetaData("Literal", "Tissue", "(", False)             # not an expression: compared as a string
    assert e.getCellSet("Literal") == []
    e.createCellSetUsingMetaData("UnknownField", "NoSuchField", ".*", True)
    assert e.getCellSet("UnknownField") == r.select("NoSuchField", ".*", True) == []
    e.createCellSetUsingMetaData("Plates", "Plate", "P[02]", True)
    assert e.getCellSet("Plates") == r.select("Plate", "P[02]", True) and e.getCellSet("Plates")
    # usable by name at once, and after reopening
    e.close()
    assert ExpressionMatrix(e.directoryName).getCellSet("Plates") == r.select("Plate", "P[02]", True)


# ---- the doubles ----

LARGEST_N = 94906266                                            # n (n - 1) < 2^53 <= (n + 1) n

RAND_TABLES = {
    "one element": [[1]],
    "one value in both fields": [[1000]],
    "identical labelings": [[5, 0, 0], [0, 7, 0], [0, 0, 11]],
    "identical, singletons": np.eye(9, dtype=np.uint64),
    "independent labelings": [[6, 12, 18], [4, 8, 12], [10, 20, 30]],
    "one row": [[3, 4, 5]],
    "one column": [[3], [4], [5]],
    "zeros": [[0, 3, 0], [0, 0, 0], [2, 0, 1]],
    "odd counts": [[1, 2, 3], [7, 1, 0], [0, 13, 1]],
    "large": [[30000001, 12345677], [2999999, 40000003]],
    "the largest n, one cell": [[LARGEST_N]],
    "the largest n, spread": [[LARGEST_N - 60000003, 20000001], [1, 40000001]],
}


@pytest.mark.parametrize("name", sorted(RAND_TABLES))
def test_rand_index_bits(restatement, name):
    table = np.asarray(RAND_TABLES[name], dtype=np.uint64)
    sum_cells, sum_rows, sum_columns, n = mb.sums_of(table)
    if name.startswith("the largest n"):
        assert n == LARGEST_N
    mine = capi.rand_index(sum_cells, sum_rows, sum_columns, n)
    theirs = restatement.rand_index(table)
    assert [mb.double_bits(x) for x in mine] == [mb.double_bits(x) for x in theirs], (mine, theirs)
    if name == "one element":
        assert all(math.isnan(x) for x in mine)                 # 0 / 0 in both
    if name == "one value in both fields":
        assert mine[0] == 1.0 and math.isnan(mine[1])
    if name == "identical labelings":
        assert mine == (1.0, 1.0)
    if name == "identical, singletons":
        assert mine[0] == 1.0 and math.isnan(mine[1])           # no pair shares a value in either field: 0 / 0 again
    if name == "independent labelings":
        assert abs(mine[1]) < 0.05 and 0. < mine[0] < 1.        # (a table of products: near the chance level, not exactly on it)


def test_rand_index_limits():
    assert LARGEST_N * (LARGEST_N - 1) < 2 ** 53 <= (LARGEST_N + 1) * LARGEST_N
    n = LARGEST_N + 1                                           # the first n beyond the limit: refused, not rounded
    with pytest.raises(RuntimeError, match="2\\^53"):
        capi.rand_index(n * (n - 1), n * (n - 1), n * (n - 1), n)
    with pytest.raises(RuntimeError, match="rowCount > 0"):
        capi.rand_index(0, 0, 0, 0)
