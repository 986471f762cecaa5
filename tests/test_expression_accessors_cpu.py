"""The sparse accessors of the facade -- getCellExpressionCount, getCellExpressionCounts, getCellsExpressionCount,
getCellsExpressionCounts, getCellsExpressionCountsForGenes (src/ExpressionMatrix.cpp:1030-1168) -- against the arrays the
directory was made from.  No GPU."""
import numpy as np
import pytest

from expressionmatrix2_amd import ExpressionMatrix, capi, files

GENES = 9
# cell 1 has no entry; cell 2 stores a zero for gene 4; gene 8 is in cell 3 alone
ROWS = [[(0, 1.5), (3, 2.0), (7, 0.25)], [], [(1, 3.0), (4, 0.0), (5, 7.5)], [(8, 1.0)], [(0, 4.0), (1, 5.0), (2, 6.0), (3, 7.0)]]


@pytest.fixture(scope="module")
def matrix(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("accessors") / "data")
    toc = np.cumsum([0] + [len(row) for row in ROWS]).astype(np.uint64)
    data = np.array([entry for row in ROWS for entry in row], dtype=capi.COUNT_DTYPE)
    files.create_directory(d, GENES, toc, data)
    return ExpressionMatrix(d)


def test_symbol_is_declared():
    assert "em2_matrix_cell_expression_counts" in capi.SYMBOLS and hasattr(capi.load(), "em2_matrix_cell_expression_counts")


def test_cell_expression_counts(matrix):
    for cell, row in enumerate(ROWS):
        assert matrix.getCellExpressionCounts(cell) == row
    assert matrix.getCellExpressionCounts(1) == []                              # a cell without entries
    assert (4, 0.0) in matrix.getCellExpressionCounts(2)                        # a stored zero is returned: it is stored


def test_cells_expression_counts_keep_the_order_given(matrix):
    cells = [4, 2, 2, 1, 0]                                                     # repeating and descending
    assert matrix.getCellsExpressionCounts(cells) == [ROWS[cell] for cell in cells]
    assert matrix.getCellsExpressionCounts([]) == []


def test_cell_expression_count(matrix):
    for cell, row in enumerate(ROWS):
        stored = dict(row)
        for gene in range(GENES):
            value = matrix.getCellExpressionCount(cell, gene)
            assert isinstance(value, float) and value == stored.get(gene, 0.0)
    assert matrix.getCellExpressionCount(0, 1) == 0.0                           # a gene absent from the cell
    assert matrix.getCellExpressionCount(1, 0) == 0.0                           # a cell without entries
    assert matrix.getCellExpressionCount(0, GENES + 100) == 0.0                 # behind the last stored gene


def test_cells_expression_count(matrix):
    cells = [4, 4, 3, 0, 1]
    assert matrix.getCellsExpressionCount(cells, 0) == [4.0, 4.0, 0.0, 1.5, 0.0]
    assert matrix.getCellsExpressionCount(cells, 8) == [0.0, 0.0, 1.0, 0.0, 0.0]


def test_cells_expression_counts_for_genes(matrix):
    cells, genes = [4, 2, 0, 1, 2], [3, 0, 4, 4]                                # global gene ids, given unsorted and repeated
    expected = [[(gene, count) for gene, count in ROWS[cell] if gene in genes] for cell in cells]
    assert matrix.getCellsExpressionCountsForGenes(cells, genes) == expected
    assert expected[1] == [(4, 0.0)] and expected[3] == []
    assert matrix.getCellsExpressionCountsForGenes(cells, []) == [[] for _ in cells]


def test_an_id_out_of_range_is_refused(matrix):
    for call in (lambda: matrix.getCellExpressionCounts(len(ROWS)), lambda: matrix.getCellExpressionCount(len(ROWS), 0),
                 lambda: matrix.getCellsExpressionCounts([0, len(ROWS)]), lambda: matrix.getCellsExpressionCount([len(ROWS)], 0),
                 lambda: matrix.getCellsExpressionCountsForGenes([2 ** 32 - 1], [0])):
        with pytest.raises(RuntimeError, match="not below the cell count"):
            call()
    count = capi.ctypes.c_uint64(0)
    assert capi.load().em2_matrix_cell_expression_counts(matrix._handle, len(ROWS), capi.ctypes.byref(count), None) == capi.EM2_ERROR_INVALID_ARGUMENT


def test_gene_names_are_not_offered(matrix):
    for call in (lambda: matrix.getCellExpressionCount(0, "Gene0"), lambda: matrix.getCellsExpressionCount([0], "Gene0"),
                 lambda: matrix.getCellsExpressionCountsForGenes([0], ["Gene0"])):
        with pytest.raises(TypeError, match="GeneNames"):
            call()
