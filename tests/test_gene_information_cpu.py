"""Gene information content and gene-set creation without a GPU: the C++ restatement the device is compared with
(tests/native/em2_gene_information_restatement.cpp) meets the error bound against the higher-precision statement R on every
input the GPU tests use (so the inputs and the bound fit together), its counts equal a plain numpy statement and its norms do on a sample of about 300 cells per input, the
library's host norm walk equals it bit for bit, the Cells file has the reference's byte offsets, the gene-set files equal
those of add_gene_set, and the facade reports the reference's errors in the reference's order."""
import inspect
import os

import numpy as np
import pytest

import gene_information_binding as gib
from expressionmatrix2_amd import ExpressionMatrix, NormalizationMethod, capi, files


@pytest.fixture(scope="module")
def restatement():
    return gib.load()


@pytest.fixture
def data_dir(tmp_path):
    toc, data, genes = gib.case("odd")
    directory = str(tmp_path / "data")
    files.create_directory(directory, genes, toc, data)
    return directory


@pytest.mark.parametrize("method", [gib.NONE, gib.L1, gib.L2])
@pytest.mark.parametrize("name", gib.ALL_CASES)
def test_restatement_meets_the_bound(restatement, name, method):
    toc, data, genes = gib.case(name)
    norm = gib.norm_inverse_for(restatement, toc, data, method)
    mine = restatement.gene_information_content(toc, data, genes, norm)
    R, n, weight = gib.higher_precision(toc, data, genes, norm)
    assert np.array_equal(mine["positive"], n)
    gib.assert_within_bound(mine["double"], R, n, weight, "%s method %d" % (name, method))
    assert np.array_equal(mine["single"].view(np.uint32), mine["double"].astype(np.float32).view(np.uint32))
    # a gene without a positive entry: float(log(N) / log(2)) exactly
    none = n == 0
    expected = np.float32(np.log(np.float64(len(toc) - 1)) / np.log(2.))
    assert np.all(mine["single"][none].view(np.uint32) == expected.view(np.uint32))


@pytest.mark.parametrize("name", gib.ALL_CASES)
def test_restatement_counts_and_norms_equal_numpy(restatement, name):
    toc, data, genes = gib.case(name)
    mine = restatement.gene_information_content(toc, data, genes, None)
    assert np.array_equal(mine["expressing"], np.bincount(data["gene"], minlength=genes))
    n1, n2 = restatement.cell_norm_inverses(toc, data)
    with np.errstate(all="ignore"):
        for cell in range(0, len(toc) - 1, max(1, (len(toc) - 1) // 300)):
            v = data["count"][int(toc[cell]):int(toc[cell + 1])]
            sum1, sum2 = np.float64(0.), np.float64(0.)
            for x in v:
                sum1 += np.float64(x)
                sum2 += np.float64(x * x)                       # a float32 product
            assert np.float64(1.) / sum1 == n1[cell] or (np.isnan(n1[cell]) and np.isnan(1. / sum1))
            assert np.float64(1.) / np.sqrt(sum2) == n2[cell] or (np.isnan(n2[cell]) and np.isnan(1. / np.sqrt(sum2)))


@pytest.mark.parametrize("name", ["random-1000x257", "odd", "empty-cell", "genes-65537"])
def test_library_norm_walk_equals_the_restatement(restatement, name):
    toc, data, genes = gib.case(name)
    n1, n2 = restatement.cell_norm_inverses(toc, data)
    m1, m2 = capi.cell_norm_inverses(toc, data, genes)
    assert np.array_equal(n1.view(np.uint64), m1.view(np.uint64)) and np.array_equal(n2.view(np.uint64), m2.view(np.uint64))


def test_norm_walk_checks_the_gene_ids():
    toc, data, genes = gib.case("odd")
    with pytest.raises(RuntimeError, match="not below geneCount"):
        capi.cell_norm_inverses(toc, data, 5)
    unsorted = data.copy()
    unsorted["gene"][[0, 1]] = unsorted["gene"][[1, 0]]
    with pytest.raises(RuntimeError, match="strictly ascending"):
        capi.cell_norm_inverses(toc, unsorted, genes)


def test_cells_file_round_trip(data_dir):
    n1 = np.arange(300, dtype=np.float64) + 0.25
    n2 = -(np.arange(300, dtype=np.float64) + 0.5)
    files.add_cells(data_dir, n1, n2)
    raw = open(os.path.join(data_dir, "Cells"), "rb").read()
    header = np.frombuffer(raw[:56], dtype=np.uint64)
    assert header[0] == 256 and header[1] == 56 and header[2] == 300 and header[6] == 0xa3756fd4b5d8bcc1
    records = np.frombuffer(raw[256:256 + 300 * 56], dtype=np.float64).reshape(300, 7)
    assert np.array_equal(records[:, 3], n1) and np.array_equal(records[:, 4], n2)             # bytes 24 and 32 of every record
    assert not records[:, [0, 1, 2, 5, 6]].any()


def test_host_entry_needs_a_device_or_says_so():
    """The argument checks of em2_gene_information_content that need no device answer before any device call."""
    toc, data, genes = gib.case("odd")
    lib = capi.load()
    out = np.zeros(genes, dtype=np.float32)
    with pytest.raises(RuntimeError, match="geneCount must be positive"):
        capi.check(lib.em2_gene_information_content(capi._ptr(toc), capi._ptr(data), len(toc) - 1, 0, None, capi._ptr(out), None, None))
    with pytest.raises(RuntimeError, match="cellCount must be positive"):
        capi.check(lib.em2_gene_information_content(capi._ptr(toc), capi._ptr(data), 0, genes, None, capi._ptr(out), None, None))
    if capi.device_count() == 0:
        with pytest.raises(RuntimeError, match="no HIP device"):
            capi.gene_information_content(toc, data, genes)


def test_facade_errors_and_their_order(data_dir):
    e = ExpressionMatrix(data_dir)
    files.add_gene_set(data_dir, "Written", [1, 2, 3])
    create = e.createGeneSetUsingInformationContent
    # information content: the existing gene set, the cell set, then the new name (src/ExpressionMatrix.cpp:2030-2046)
    with pytest.raises(RuntimeError, match=r"^Gene set Nope does not exist\.$"):
        create("Nope", "NoCells", NormalizationMethod.L2, 2., "AllGenes")
    with pytest.raises(RuntimeError, match=r"^Cell set NoCells does not exist\.$"):
        create("AllGenes", "NoCells", NormalizationMethod.L2, 2., "AllGenes")
    with pytest.raises(RuntimeError, match=r"^Gene set AllGenes already exists\.$"):
        create("AllGenes", "AllCells", NormalizationMethod.L2, 2., "AllGenes")
    # well expressed: the output name first (src/ExpressionMatrixGeneSets.cpp:322-329)
    with pytest.raises(RuntimeError, match=r"^Gene set AllGenes already exists\.$"):
        e.createWellExpressedGeneSet("Nope", "NoCells", "AllGenes", 1)
    with pytest.raises(RuntimeError, match=r"^Gene set Nope does not exist\.$"):
        e.createWellExpressedGeneSet("Nope", "NoCells", "New", 1)
    with pytest.raises(RuntimeError, match=r"^Cell set NoCells does not exist\.$"):
        e.createWellExpressedGeneSet("AllGenes", "NoCells", "New", 1)
    with pytest.raises(RuntimeError, match=r"^Gene set AllGenes cannot be removed\.$"):
        e.removeGeneSet("AllGenes")
    with pytest.raises(RuntimeError, match=r"^Gene set New does not exist\.$"):
        e.removeGeneSet("New")
    with pytest.raises(RuntimeError, match=r"^Gene set New does not exist\.$"):
        e.getGeneSetGenes("New")
    with pytest.raises(TypeError):
        create(newGeneSetName="X")
    with pytest.raises(ValueError):
        create(normalizationMethod=3, geneInformationContentThreshold=2., newGeneSetName="X")
    assert not os.path.exists(os.path.join(data_dir, "GeneSet-New-GlobalIds"))
    assert not os.path.exists(os.path.join(data_dir, "GeneSet-X-GlobalIds"))
    # the reference's argument names and defaults (src/PythonModule.cpp:506-537, 586-602)
    parameters = inspect.signature(ExpressionMatrix.createGeneSetUsingInformationContent).parameters
    assert list(parameters)[1:] == ["existingGeneSetName", "cellSetName", "normalizationMethod", "geneInformationContentThreshold", "newGeneSetName"]
    assert parameters["existingGeneSetName"].default == "AllGenes" and parameters["cellSetName"].default == "AllCells"
    parameters = inspect.signature(ExpressionMatrix.createWellExpressedGeneSet).parameters
    assert list(parameters)[1:] == ["inputGeneSetName", "inputCellSetName", "outputGeneSetName", "minCellCount"]
    assert parameters["inputGeneSetName"].default == "AllGenes" and parameters["inputCellSetName"].default == "AllCells"
    assert e.getGeneSetGenes("AllGenes") == list(range(12))
    e.close()


def test_empty_inputs_make_sets_without_a_device(data_dir):
    """An empty gene set gives an empty set; an empty cell set gives log(0) / log(2) = -inf for every gene and no expressing
    cell: neither needs the device, and the files equal those add_gene_set writes for the same ids."""
    files.add_gene_set(data_dir, "NoGenes", [])
    files.add_cell_set(data_dir, "NoCells", [])
    e = ExpressionMatrix(data_dir)
    e.createGeneSetUsingInformationContent("NoGenes", "AllCells", NormalizationMethod.L2, 0., "A")
    assert e.getGeneSetGenes("A") == []
    assert np.all(e.computeGeneInformationContent("AllGenes", "NoCells", NormalizationMethod.none) == -np.inf)
    e.createGeneSetUsingInformationContent("AllGenes", "NoCells", NormalizationMethod.none, -1e30, "B")
    assert e.getGeneSetGenes("B") == []
    e.createWellExpressedGeneSet("AllGenes", "NoCells", "C", 0)
    assert e.getGeneSetGenes("C") == list(range(12))
    files.add_gene_set(data_dir, "Written", list(range(12)))
    for part in ("GlobalIds", "LocalIds"):
        mine = open(os.path.join(data_dir, "GeneSet-C-" + part), "rb").read()
        assert mine == open(os.path.join(data_dir, "GeneSet-Written-" + part), "rb").read()
        empty = open(os.path.join(data_dir, "GeneSet-A-" + part), "rb").read()
        assert empty == open(os.path.join(data_dir, "GeneSet-NoGenes-" + part), "rb").read()
    e.removeGeneSet("C")
    assert not os.path.exists(os.path.join(data_dir, "GeneSet-C-GlobalIds")) and not os.path.exists(os.path.join(data_dir, "GeneSet-C-LocalIds"))
    e.createWellExpressedGeneSet("AllGenes", "NoCells", "C", 1)                   # the name is free again
    assert e.getGeneSetGenes("C") == []
    e.close()
    assert ExpressionMatrix(data_dir).getGeneSetGenes("C") == []                  # and a new object finds the set on disk


def test_a_set_written_after_the_open_is_not_overwritten(data_dir):
    """'Gene set X already exists.' also for a set whose files reached the directory after this object was opened."""
    e = ExpressionMatrix(data_dir)
    files.add_gene_set(data_dir, "Later", [2, 3])
    before = open(os.path.join(data_dir, "GeneSet-Later-GlobalIds"), "rb").read()
    with pytest.raises(RuntimeError, match=r"^Gene set Later already exists\.$"):
        e.createWellExpressedGeneSet("AllGenes", "AllCells", "Later", 1)
    with pytest.raises(RuntimeError, match=r"^Gene set Later already exists\.$"):
        e.createGeneSetUsingInformationContent("AllGenes", "AllCells", NormalizationMethod.L2, 2., "Later")
    assert open(os.path.join(data_dir, "GeneSet-Later-GlobalIds"), "rb").read() == before
    e.close()


def test_min_cell_count_is_an_unsigned_32_bit_number(data_dir):
    e = ExpressionMatrix(data_dir)
    for bad in (-1, 2 ** 32):
        with pytest.raises(ValueError):
            e.createWellExpressedGeneSet("AllGenes", "AllCells", "W", bad)
    assert not os.path.exists(os.path.join(data_dir, "GeneSet-W-GlobalIds"))
    e.close()
