"""What the C entry points say when a required pointer is null and when no HIP device is visible: the return code and the
whole em2_last_error() text, through the raw C ABI.  Two tables.  NULL_CASES: one call per entry point that has a
": null pointer" branch, with tiny valid arguments (1 to 4 cells, lshCount 64, k 1) and one required pointer null; no pointer
handed over is read before the check answers, so the device-level entries get host addresses.  NO_DEVICE_CASES: the same
entries with every argument valid, on a machine without a GPU (skipped where there is one).

The names in front of the messages are written out, not derived from the symbol: em2_contingency_create reports as
"em2_contingency", both label propagation entries as "em2_cell_graph_label_propagation", and the matrix-level calls under the
name of the em2_matrix_* entry that reaches them."""
import ctypes

import numpy as np
import pytest

from expressionmatrix2_amd import capi, files
from expressionmatrix2_amd.expression_matrix import ExpressionMatrix, NormalizationMethod

INVALID, NO_DEVICE = 1, 2
NO_DEVICE_TEXT = ": no HIP device is visible (this library has no CPU path)"

N, G, L, K, THR = 4, 3, 64, 1, 0.2
TOC = np.array([0, 1, 2, 3, 4], dtype=np.uint64)
DATA = np.array([(0, 1.0), (1, 2.0), (2, 1.0), (0, 3.0)], dtype=capi.COUNT_DTYPE)
VECTORS = np.ones((G, L), dtype=np.float64)
SIG = np.zeros((N, 1), dtype=np.uint64)
PAIRS = np.zeros((N, K), dtype=capi.PAIR_DTYPE)
USED = np.zeros(N, dtype=np.uint32)
ONE = np.ones(N, dtype=np.uint32)                            # usedCount with a stored pair per cell (PAIRS names cell 0)
IDS = np.arange(N, dtype=np.uint32)                          # a cell set, a gene set, the vertices' cell ids
E0 = np.array([0, 1], dtype=np.uint32)
E1 = np.array([1, 2], dtype=np.uint32)
ES = np.array([0.5, 0.5], dtype=np.float32)
U32 = np.zeros(16, dtype=np.uint32)
U64 = np.zeros(16, dtype=np.uint64)
F32 = np.zeros(16, dtype=np.float32)
F64 = np.zeros(16, dtype=np.float64)
SLICES = np.array([10, 8], dtype=np.int32)
OFFSETS = np.array([0, 2], dtype=np.uint64)                  # one cluster of the cells 0 and 1
AVERAGES = np.ones((3, G), dtype=np.float64)
LAYOUT = np.zeros(8, dtype=np.uint64)                        # em2_layout_parameters: zeros are valid (tolerance, gravity, step 0)
HANDLE = ctypes.c_void_p(None)
OUT = ctypes.byref(HANDLE)
COUNT = ctypes.c_uint64(0)
ENERGY = ctypes.c_double(0.)
CSV = b"/nonexistent/em2-entry-messages.csv"                 # (never opened: the checks answer first)


def _p(a):
    return a.ctypes.data if isinstance(a, np.ndarray) else a


# entry point -> the arguments of a valid call
VALID = {
    "em2_compute_signatures": (TOC, DATA, N, G, VECTORS, L, SIG),
    "em2_find_similar_pairs4": (SIG, N, L, K, THR, PAIRS, USED),
    "em2_find_similar_pairs5": (SIG, N, L, K, THR, 8, 1000, PAIRS, USED),
    "em2_find_similar_pairs6": (SIG, N, L, K, THR, 4, 10, 64, 231, PAIRS, USED),
    "em2_find_similar_pairs7": (SIG, N, L, K, THR, SLICES, 2, 100, 12, PAIRS, USED),
    "em2_subset_find_similar_pairs4": (TOC, DATA, N, IDS, N, IDS, G, G, VECTORS, L, SIG, K, THR, PAIRS, USED),
    "em2_cell_graph_edges": (PAIRS, USED, N, K, IDS, IDS, N, THR, 0, U32, U32, F32, ctypes.byref(COUNT)),
    "em2_dev_cell_graph_edges": (PAIRS, USED, N, K, IDS, IDS, N, THR, 0, U32, U32, F32, ctypes.byref(COUNT)),
    "em2_analyze_lsh": (TOC, DATA, N, G, SIG, L, IDS, 231, 1., CSV, CSV, U64, F64, F64, None, None),
    "em2_find_similar_pairs0": (TOC, DATA, N, G, K, THR, PAIRS, USED, U32, F32),
    "em2_dev_find_similar_pairs0": (TOC, DATA, N, G, 0, N, K, THR, PAIRS, USED, U32, F32, U64, 1 << 30, None),
    "em2_find_similar_gene_pairs0": (TOC, DATA, N, G, 0, K, THR, PAIRS, USED, None),
    "em2_cell_norm_inverses": (TOC, DATA, N, G, F64, F64),
    "em2_gene_information_content": (TOC, DATA, N, G, None, F32, None, None),
    "em2_dev_gene_information_content": (TOC, DATA, N, G, 4, None, F32, None, None, U64, 1 << 30, None),
    "em2_dense_expression": (TOC, DATA, N, None, N, None, 0, G, 0, 0, F64, G),
    "em2_dev_dense_expression": (TOC, DATA, None, N, None, 0, G, 0, 0, N, 0, F64, G, U64, 1 << 30, None),
    "em2_analyze_similar_pairs": (TOC, DATA, N, G, PAIRS, ONE, K, IDS, 1., CSV, CSV, U64, F64, F64),
    "em2_cell_graph_label_propagation": (IDS, N, E0, E1, ES, 2, 231, 3, 100, U32, ctypes.byref(COUNT)),
    "em2_dev_cell_graph_label_propagation": (IDS, N, E0, E1, ES, 2, 231, 3, 100, U32, ctypes.byref(COUNT)),
    "em2_cluster_average_expression": (TOC, DATA, N, G, IDS, OFFSETS, 1, F64),
    "em2_cluster_similarities": (AVERAGES, 3, G, E0, E1, 2, F64),
    "em2_cluster_graph_create": (TOC, DATA, N, G, None, N, E0, E1, 2, U32, 1, 3, 0.5, 0.9, OUT),
    "em2_signature_graph_create": (SIG, N, L, 0, OUT),
    "em2_dev_signature_graph_create": (SIG, N, L, 0, OUT),
    "em2_lsh_signature_statistics": (SIG, N, L, U64),
    "em2_dev_lsh_signature_statistics": (SIG, N, L, U64),
    "em2_analyze_lsh_signatures": (SIG, N, L, None),
    "em2_gene_graph_create": (PAIRS, USED, N, K, IDS, IDS, N, THR, 0, OUT),
    "em2_dev_gene_graph_create": (PAIRS, USED, N, K, IDS, IDS, N, THR, 0, OUT),
    "em2_graph_layout": (N, E0, E1, 2, LAYOUT, F32, F32, None),
    "em2_dev_graph_layout": (N, E0, E1, 2, LAYOUT, F32, F32, None),
    "em2_graph_layout_forces": (N, E0, E1, 2, 0.5, F32, F32, F32, F32, ctypes.byref(ENERGY)),
    "em2_contingency_create": (IDS, IDS, N, N, N, 0, OUT),
    "em2_dev_contingency": (IDS, IDS, N, N, N, 0, OUT),
    "em2_dev_ingest_count": (TOC, U32, F32, None, N, U32, 16, U32, U32, U32, U64, None),
    "em2_dev_ingest_fill": (TOC, U32, F32, None, N, U32, 16, U64, DATA, F64, None),
    "em2_dev_csv_parse": (b"A,1\n", 4, b",", 1, 2, U32, 0, 4, U32, 4, U64, F32, 4, U32, U64, None),
    # entries that need no device: only the null-pointer table calls them
    "em2_cluster_graph_sizes": (None, None, None, None, None, None),
    "em2_cluster_graph_get": (None,) * 9,
    "em2_cluster_graph_facts": (None, F64, 5),
    "em2_signature_graph_sizes": (None, None, None, None, None, None),
    "em2_signature_graph_get": (None,) * 6,
    "em2_gene_graph_sizes": (None, None, None, None),
    "em2_gene_graph_get": (None,) * 8,
    "em2_contingency_sizes": (None, None, None, None, None, None),
    "em2_contingency_get": (None,) * 7,
    "em2_dev_find_similar_pairs4_last_launch": (None, 9),
    "em2_dev_find_similar_pairs5_last_launch": (None, 12),
    "em2_dev_fsp4_sharded_plan": (N, L, K, 0, 1, None, 12),
    "em2_dev_compute_signatures_listed": (None, N, L, 1, U32),
}

# (entry point, index of the argument that is null, the text in front of ": null pointer")
NULL_CASES = [
    ("em2_compute_signatures", 0, "em2_compute_signatures"),
    ("em2_compute_signatures", 6, "em2_compute_signatures"),
    ("em2_find_similar_pairs4", 0, "em2_find_similar_pairs4"),
    ("em2_find_similar_pairs5", 8, "em2_find_similar_pairs5"),
    ("em2_find_similar_pairs6", 9, "em2_find_similar_pairs6"),
    ("em2_find_similar_pairs7", 0, "em2_find_similar_pairs7"),
    ("em2_subset_find_similar_pairs4", 8, "em2_subset_find_similar_pairs4"),
    ("em2_subset_find_similar_pairs4", 0, "em2_subset_find_similar_pairs4"),
    ("em2_subset_find_similar_pairs4", 5, "em2_subset_find_similar_pairs4"),
    ("em2_cell_graph_edges", 1, "em2_cell_graph_edges"),
    ("em2_cell_graph_edges", 11, "em2_cell_graph_edges"),
    ("em2_dev_cell_graph_edges", 4, "em2_dev_cell_graph_edges"),
    ("em2_analyze_lsh", 4, "em2_analyze_lsh"),
    ("em2_analyze_lsh", 9, "em2_analyze_lsh"),
    ("em2_find_similar_pairs0", 0, "em2_find_similar_pairs0"),
    ("em2_find_similar_pairs0", 9, "em2_find_similar_pairs0"),
    ("em2_dev_find_similar_pairs0", 12, "em2_dev_find_similar_pairs0"),
    ("em2_find_similar_gene_pairs0", 0, "em2_find_similar_gene_pairs0"),
    ("em2_find_similar_gene_pairs0", 8, "em2_find_similar_gene_pairs0"),
    ("em2_cell_norm_inverses", 4, "em2_cell_norm_inverses"),
    ("em2_gene_information_content", 5, "em2_gene_information_content"),
    ("em2_dev_gene_information_content", 9, "em2_dev_gene_information_content"),
    ("em2_dense_expression", 10, "em2_dense_expression"),
    ("em2_dev_dense_expression", 11, "em2_dev_dense_expression"),
    ("em2_analyze_similar_pairs", 5, "em2_analyze_similar_pairs"),
    ("em2_analyze_similar_pairs", 10, "em2_analyze_similar_pairs"),
    ("em2_cell_graph_label_propagation", 9, "em2_cell_graph_label_propagation"),
    ("em2_dev_cell_graph_label_propagation", 2, "em2_cell_graph_label_propagation"),
    ("em2_cluster_average_expression", 7, "em2_cluster_average_expression"),
    ("em2_cluster_similarities", 6, "em2_cluster_similarities"),
    ("em2_cluster_graph_create", 14, "em2_cluster_graph_create"),
    ("em2_cluster_graph_create", 0, "em2_cluster_graph_create"),
    ("em2_cluster_graph_create", 9, "em2_cluster_graph_create"),
    ("em2_cluster_graph_sizes", 0, "em2_cluster_graph_sizes"),
    ("em2_cluster_graph_get", 0, "em2_cluster_graph_get"),
    ("em2_cluster_graph_facts", 0, "em2_cluster_graph_facts"),
    ("em2_signature_graph_create", 4, "em2_signature_graph_create"),
    ("em2_signature_graph_create", 0, "em2_signature_graph_create"),
    ("em2_dev_signature_graph_create", 0, "em2_dev_signature_graph_create"),
    ("em2_signature_graph_sizes", 0, "em2_signature_graph_sizes"),
    ("em2_signature_graph_get", 0, "em2_signature_graph_get"),
    ("em2_lsh_signature_statistics", 3, "em2_lsh_signature_statistics"),
    ("em2_dev_lsh_signature_statistics", 0, "em2_dev_lsh_signature_statistics"),
    ("em2_analyze_lsh_signatures", 0, "em2_analyze_lsh_signatures"),
    ("em2_gene_graph_create", 9, "em2_gene_graph_create"),
    ("em2_gene_graph_create", 5, "em2_gene_graph_create"),
    ("em2_dev_gene_graph_create", 1, "em2_dev_gene_graph_create"),
    ("em2_gene_graph_sizes", 0, "em2_gene_graph_sizes"),
    ("em2_gene_graph_get", 0, "em2_gene_graph_get"),
    ("em2_graph_layout", 4, "em2_graph_layout"),
    ("em2_dev_graph_layout", 5, "em2_dev_graph_layout"),
    ("em2_graph_layout_forces", 7, "em2_graph_layout_forces"),
    ("em2_contingency_create", 6, "em2_contingency"),
    ("em2_contingency_create", 0, "em2_contingency"),
    ("em2_dev_contingency", 1, "em2_dev_contingency"),
    ("em2_contingency_sizes", 0, "em2_contingency_sizes"),
    ("em2_contingency_get", 0, "em2_contingency_get"),
    ("em2_dev_ingest_count", 0, "em2_dev_ingest_count"),
    ("em2_dev_ingest_fill", 8, "em2_dev_ingest_fill"),
    ("em2_dev_csv_parse", 14, "em2_dev_csv_parse"),
    ("em2_dev_find_similar_pairs4_last_launch", 0, "em2_dev_find_similar_pairs4_last_launch"),
    ("em2_dev_find_similar_pairs5_last_launch", 0, "em2_dev_find_similar_pairs5_last_launch"),
    ("em2_dev_fsp4_sharded_plan", 5, "em2_dev_fsp4_sharded_plan"),
    ("em2_dev_compute_signatures_listed", 4, "em2_dev_compute_signatures_listed"),
]


def test_the_read_back_of_the_projection_lists_checks_its_arguments():
    """em2_dev_compute_signatures_listed: its two other refusals, and the zeros it reports without touching the device when the
    call it asks about had no list (no auxiliary block, a width that is no multiple of 4, no cells)."""
    listed = np.full(3, 7, dtype=np.uint32)
    assert call("em2_dev_compute_signatures_listed", (None, N, 0, 1, listed)) == (INVALID, "em2_dev_compute_signatures_listed: bad argument")
    assert call("em2_dev_compute_signatures_listed", (None, N, L, 1, listed)) == (INVALID, "em2_dev_compute_signatures_listed: null workspace")
    for cells, lsh_count, aux in [(N, L, 0), (N, 63, 1), (0, L, 1)]:
        listed[:] = 7
        assert capi.load().em2_dev_compute_signatures_listed(None, cells, lsh_count, aux, listed.ctypes.data) == 0
        assert listed.tolist() == [0, 0, 0]

# (entry point, the text in front of the sentence): every entry point of VALID that looks for the device
NO_DEVICE_CASES = [
    ("em2_compute_signatures", "em2_compute_signatures"),
    ("em2_find_similar_pairs4", "em2_find_similar_pairs4"),
    ("em2_find_similar_pairs5", "em2_find_similar_pairs5"),
    ("em2_find_similar_pairs6", "em2_find_similar_pairs6"),
    ("em2_find_similar_pairs7", "em2_find_similar_pairs7"),
    ("em2_subset_find_similar_pairs4", "em2_subset_find_similar_pairs4"),
    ("em2_cell_graph_edges", "em2_cell_graph_edges"),
    ("em2_dev_cell_graph_edges", "em2_dev_cell_graph_edges"),
    ("em2_analyze_lsh", "em2_analyze_lsh"),
    ("em2_find_similar_pairs0", "em2_find_similar_pairs0"),
    ("em2_find_similar_gene_pairs0", "em2_find_similar_gene_pairs0"),
    ("em2_gene_information_content", "em2_gene_information_content"),
    ("em2_dense_expression", "em2_dense_expression"),
    ("em2_analyze_similar_pairs", "em2_analyze_similar_pairs"),
    ("em2_cell_graph_label_propagation", "em2_cell_graph_label_propagation"),
    ("em2_dev_cell_graph_label_propagation", "em2_cell_graph_label_propagation"),
    ("em2_cluster_average_expression", "em2_cluster_average_expression"),
    ("em2_cluster_similarities", "em2_cluster_similarities"),
    ("em2_cluster_graph_create", "em2_cluster_graph_create"),
    ("em2_signature_graph_create", "em2_signature_graph_create"),
    ("em2_dev_signature_graph_create", "em2_dev_signature_graph_create"),
    ("em2_lsh_signature_statistics", "em2_lsh_signature_statistics"),
    ("em2_dev_lsh_signature_statistics", "em2_dev_lsh_signature_statistics"),
    ("em2_analyze_lsh_signatures", "em2_analyze_lsh_signatures"),
    ("em2_gene_graph_create", "em2_gene_graph_create"),
    ("em2_dev_gene_graph_create", "em2_dev_gene_graph_create"),
    ("em2_graph_layout", "em2_graph_layout"),
    ("em2_dev_graph_layout", "em2_dev_graph_layout"),
    ("em2_graph_layout_forces", "em2_graph_layout_forces"),
    ("em2_contingency_create", "em2_contingency"),
    ("em2_dev_contingency", "em2_dev_contingency"),
    ("em2_dev_ingest_count", "em2_dev_ingest_count"),
    ("em2_dev_ingest_fill", "em2_dev_ingest_fill"),
    ("em2_dev_csv_parse", "em2_dev_csv_parse"),
]


def call(name, arguments):
    lib = capi.load()
    rc = getattr(lib, name)(*[_p(a) for a in arguments])
    return rc, lib.em2_last_error().decode()


def test_the_tables_name_symbols_of_the_library():
    assert set(VALID) <= set(capi.SYMBOLS)
    assert {name for name, _, _ in NULL_CASES} == set(VALID)
    assert {name for name, _ in NO_DEVICE_CASES} <= set(VALID)


@pytest.mark.parametrize("name,index,who", NULL_CASES, ids=["%s-%d" % (name, index) for name, index, _ in NULL_CASES])
def test_a_null_pointer(name, index, who):
    arguments = list(VALID[name])
    arguments[index] = None                                  # (a handle, index 0 of the accessors, cannot exist without a device)
    assert call(name, arguments) == (INVALID, who + ": null pointer")


needs_no_device = pytest.mark.skipif(capi.device_count() > 0, reason="a HIP device is visible")


@needs_no_device
@pytest.mark.parametrize("name,who", NO_DEVICE_CASES, ids=[name for name, _ in NO_DEVICE_CASES])
def test_no_device(name, who):
    assert call(name, VALID[name]) == (NO_DEVICE, who + NO_DEVICE_TEXT)
    assert HANDLE.value is None


@needs_no_device
def test_no_device_behind_the_matrix_level_calls(tmp_path):
    """The three sites a em2_matrix_* entry reaches: the gene information of a stored matrix, the bulk add and the CSV add."""
    directory = str(tmp_path / "tool")
    files.create_directory(directory, G, TOC, DATA)
    e = ExpressionMatrix(directory)
    with pytest.raises(RuntimeError) as error:
        e.computeGeneInformationContent("AllGenes", "AllCells", NormalizationMethod.L2)
    assert str(error.value) == "em2_matrix_gene_information_content" + NO_DEVICE_TEXT
    e.close()
    e = ExpressionMatrix.create(str(tmp_path / "store"))
    with pytest.raises(RuntimeError) as error:
        e.addCellsFromCsr(["g0", "g1"], ["c0", "c1"], [0, 1, 2], [0, 1], np.ones(2, np.float32))
    assert str(error.value) == "em2_matrix_add_cells_csr" + NO_DEVICE_TEXT
    expression, meta = tmp_path / "e.csv", tmp_path / "m.csv"
    expression.write_text("g,c0,c1\nA,1,2\nB,3,4\n")
    meta.write_text("Cell,Organ\nc0,Brain\nc1,Liver\n")
    with pytest.raises(RuntimeError) as error:
        e.addCells(expressionCountsFileName=str(expression), cellMetaDataFileName=str(meta))
    assert str(error.value) == "em2_matrix_add_cells_csv" + NO_DEVICE_TEXT
    e.close()
