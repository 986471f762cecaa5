"""The cell set operations of the facade (createCellSet, createCellSetIntersection / Union / Difference, downsampleCellSet,
removeCellSet, getCellSet, getCellSetNames) without a GPU: every result against the C++ restatement
(tests/native/em2_dense_restatement.cpp) and against an independent numpy statement, every error text in the reference's order
of checks (src/ExpressionMatrix.cpp:1626-1777, src/CellSets.cpp:65-97), the files, and the use of a new set by name."""
import os

import numpy as np
import pytest

import dense_binding as db
import fsp0_binding
from expressionmatrix2_amd import ExpressionMatrix, capi, files

CELLS, GENES = 60, 50
A = [41, 3, 17, 3, 59, 0, 17, 22, 8]                 # unsorted and repeated
B = [8, 9, 22, 30, 41, 58]
SETS = {"A": np.unique(A), "B": np.array(B), "Empty": np.zeros(0, dtype=np.int64), "AllCells": np.arange(CELLS)}


@pytest.fixture(scope="module")
def restatement():
    return db.load()


@pytest.fixture()
def matrix(tmp_path):
    d = str(tmp_path / "data")
    toc, data = fsp0_binding.clustered(CELLS, GENES, 0.2, seed=5, cluster_count=3, non_integer=True)
    files.create_directory(d, GENES, toc, data)
    e = ExpressionMatrix(d)
    e.createCellSet("A", A)
    e.createCellSet("B", B)
    e.createCellSet("Empty", [])
    return e


def raises(text, call, *arguments):
    with pytest.raises(RuntimeError) as error:
        call(*arguments)
    assert str(error.value) == text, str(error.value)


def test_symbols_are_declared():
    for name in ("em2_matrix_create_cell_set", "em2_matrix_create_cell_set_intersection", "em2_matrix_create_cell_set_union",
                 "em2_matrix_create_cell_set_difference", "em2_matrix_downsample_cell_set", "em2_matrix_remove_cell_set",
                 "em2_matrix_cell_set_names"):
        assert name in capi.SYMBOLS and hasattr(capi.load(), name)
    assert capi.load().em2_abi_version() == 1


def test_create_cell_set_sorts_and_deduplicates(matrix, restatement):
    assert matrix.createCellSet("C", [5, 5, 1]) is None
    assert matrix.getCellSet("A") == np.unique(A).tolist() == restatement.deduplicate(A).tolist()
    assert matrix.getCellSet("C") == [1, 5] and matrix.getCellSet("Empty") == []
    assert matrix.getCellSet("NoSuchSet") == []                                 # ExpressionMatrixHttpServerCells.cpp:865-875
    assert matrix.getCellSetNames() == sorted(["A", "AllCells", "B", "C", "Empty"])       # std::map order
    # the file is what em2_tool_add_cell_set writes for the same ids
    files.add_cell_set(matrix.directoryName, "ByTool", np.unique(A).astype(np.uint32))
    read = lambda name: open(os.path.join(matrix.directoryName, "CellSet-" + name), "rb").read()
    assert read("A") == read("ByTool")


def test_create_cell_set_errors(matrix):
    raises("Cell set A already exists.", matrix.createCellSet, "A", [1])
    raises("Cell set AllCells already exists.", matrix.createCellSet, "AllCells", [1])
    with pytest.raises(RuntimeError, match="not below the cell count"):
        matrix.createCellSet("TooFar", [1, CELLS])
    assert "TooFar" not in matrix.getCellSetNames() and not os.path.exists(os.path.join(matrix.directoryName, "CellSet-TooFar"))
    with pytest.raises(ValueError):
        matrix.createCellSet("Negative", [-1])
    # a set that another object wrote into the directory since this one was opened exists too
    other = ExpressionMatrix(matrix.directoryName)
    other.createCellSet("Later", [2])
    raises("Cell set Later already exists.", matrix.createCellSet, "Later", [3])


@pytest.mark.parametrize("names", ["A,B", "B,A", "A,B,Empty", "Empty,A", "A,B,AllCells", "AllCells,B,A", "A", "A,A"])
def test_intersection_and_union(matrix, restatement, names):
    inputs = [SETS[name] for name in names.split(",")]
    for method, operation, numpy_operation in ((matrix.createCellSetUnion, db.UNION, np.union1d),
                                               (matrix.createCellSetIntersection, db.INTERSECTION, np.intersect1d)):
        output = "Out%d" % operation
        assert method(names, output) is None
        folded, independent = inputs[0].astype(np.uint32), inputs[0]
        for following in inputs[1:]:
            folded = restatement.set_operation(operation, folded, following)
            independent = numpy_operation(independent, following)
        assert matrix.getCellSet(output) == folded.tolist() == independent.tolist()


def test_difference(matrix, restatement):
    for name0, name1 in (("A", "B"), ("B", "A"), ("A", "Empty"), ("Empty", "A"), ("AllCells", "A"), ("A", "A")):
        output = "D-%s-%s" % (name0, name1)
        assert matrix.createCellSetDifference(name0, name1, output) is None
        expected = restatement.set_operation(db.DIFFERENCE, SETS[name0], SETS[name1])
        assert matrix.getCellSet(output) == expected.tolist() == np.setdiff1d(SETS[name0], SETS[name1]).tolist()


def test_set_operation_errors_in_the_reference_order(matrix):
    for method in (matrix.createCellSetIntersection, matrix.createCellSetUnion):
        raises("Cell set B already exists.", method, "A,Missing", "B")          # the output's check comes first
        raises("Cell set Missing does not exist.", method, "A,Missing,AlsoMissing", "New")
        raises("Cell set  does not exist.", method, "A,,B", "New")              # a stray comma: an empty name
        raises("Cell set  does not exist.", method, "A,B,", "New")
        raises("Cell set  does not exist.", method, "", "New")
    raises("Cell set B already exists.", matrix.createCellSetDifference, "Missing", "A", "B")
    raises("Cell set Missing does not exists.", matrix.createCellSetDifference, "Missing", "AlsoMissing", "New")       # sic
    raises("Cell set AlsoMissing does not exists.", matrix.createCellSetDifference, "A", "AlsoMissing", "New")
    assert "New" not in matrix.getCellSetNames()


@pytest.mark.parametrize("seed", [0, 231, -1, 2 ** 32 + 5])
@pytest.mark.parametrize("probability", [0., 1., 0.5, 1e-9])
def test_downsample(matrix, restatement, probability, seed):
    for source in ("AllCells", "A", "Empty"):
        output = "Sample-" + source
        if source == "AllCells":
            assert matrix.downsampleCellSet(newCellSetName=output, probability=probability, seed=seed) is None      # the default
        else:
            assert matrix.downsampleCellSet(source, output, probability, seed) is None
        ids = SETS[source]
        expected = restatement.downsample(ids, probability, seed)
        # independently: numpy's MT19937 seeded as init_genrand seeds, one 32-bit draw per cell
        generator = np.random.RandomState(seed % 2 ** 32)
        draws = generator.randint(0, 2 ** 32, size=len(ids), dtype=np.uint32).astype(np.float64) * 2.0 ** -32
        assert matrix.getCellSet(output) == expected.tolist() == ids[draws < probability].tolist()
        if probability == 1.:
            assert matrix.getCellSet(output) == ids.tolist()
        if probability == 0.:
            assert matrix.getCellSet(output) == []


def test_downsample_wraps_the_seed(matrix):
    matrix.downsampleCellSet("AllCells", "S0", 0.5, -1)
    matrix.downsampleCellSet("AllCells", "S1", 0.5, 2 ** 32 - 1)
    matrix.downsampleCellSet("AllCells", "S2", 0.5, 2 ** 32 + 5)
    matrix.downsampleCellSet("AllCells", "S3", 0.5, 5)
    assert matrix.getCellSet("S0") == matrix.getCellSet("S1") and matrix.getCellSet("S2") == matrix.getCellSet("S3")
    assert matrix.getCellSet("S0") != matrix.getCellSet("S2") and 0 < len(matrix.getCellSet("S0")) < CELLS


def test_downsample_errors(matrix):
    raises("Cell set Missing does not exists.", matrix.downsampleCellSet, "Missing", "B", 0.5, 1)                     # sic
    raises("Cell set B already exists.", matrix.downsampleCellSet, "A", "B", 0.5, 1)
    with pytest.raises(TypeError):
        matrix.downsampleCellSet("A")


def test_a_new_set_is_usable_at_once_and_by_a_second_handle(matrix):
    genes, toc, data = matrix._subset("AllGenes", "A")
    whole_genes, whole_toc, whole_data = matrix._subset("AllGenes", "AllCells")
    assert genes == whole_genes == GENES and len(toc) == len(SETS["A"]) + 1
    for row, cell in enumerate(SETS["A"]):
        assert np.array_equal(data[int(toc[row]):int(toc[row + 1])], whole_data[int(whole_toc[cell]):int(whole_toc[cell + 1])])
    other = ExpressionMatrix(matrix.directoryName)
    assert other.getCellSet("A") == SETS["A"].tolist() and "B" in other.getCellSetNames()
    _, other_toc, other_data = other._subset("AllGenes", "A")
    assert np.array_equal(other_toc, toc) and np.array_equal(other_data, data)
    raises("Cell set Empty is empty.", matrix._subset, "AllGenes", "Empty")


def test_remove_cell_set(matrix):
    path = os.path.join(matrix.directoryName, "CellSet-B")
    assert os.path.exists(path)
    assert matrix.removeCellSet("B") is None
    assert not os.path.exists(path) and "B" not in matrix.getCellSetNames() and matrix.getCellSet("B") == []
    raises("Cell set B does not exist.", matrix.removeCellSet, "B")
    raises("Cell set B does not exist.", matrix._subset, "AllGenes", "B")
    raises("Cell set AllCells cannot be removed.", matrix.removeCellSet, "AllCells")
    assert "B" not in ExpressionMatrix(matrix.directoryName).getCellSetNames()
    matrix.createCellSet("B", [4])                                             # the name is free again
    assert matrix.getCellSet("B") == [4]
