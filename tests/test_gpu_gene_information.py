"""Gene information content and the expressing-cell counts on the GPU (csrc/em2_gene_information.hip): the returned doubles
against the higher-precision statement R within |I - R| <= 4 (n + 8) 2^-53 (1 + log2 N + sum |p log2 p|), the floats as roundings
of the doubles, the counts and the genes without a positive entry bit for bit against the C++ restatement
(tests/native/em2_gene_information_restatement.cpp), determinism (the same call twice, the host and the device entry, a grid of
two blocks), and the facade: new gene sets from the returned floats, usable by name at once."""
import os

import numpy as np
import pytest

import gene_information_binding as gib
from expressionmatrix2_amd import ExpressionMatrix, NormalizationMethod, capi, files

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def restatement():
    return gib.load()


def bits(a):
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def check_case(restatement, name, method):
    toc, data, genes = gib.case(name)
    norm = gib.norm_inverse_for(restatement, toc, data, method)
    single, double, expressing = capi.gene_information_content(toc, data, genes, norm)
    R, n, weight = gib.higher_precision(toc, data, genes, norm)
    gib.assert_within_bound(double, R, n, weight, "%s method %d" % (name, method))
    assert np.array_equal(bits(single), bits(double.astype(np.float32)))
    assert np.array_equal(expressing, np.bincount(data["gene"], minlength=genes))
    theirs = restatement.gene_information_content(toc, data, genes, norm)
    assert np.array_equal(expressing, theirs["expressing"])
    none = theirs["positive"] == 0
    assert np.array_equal(bits(single[none]), bits(theirs["single"][none]))
    assert np.array_equal(bits(double[none]), bits(theirs["double"][none]))
    assert np.array_equal(np.isnan(single), np.isnan(theirs["single"]))
    return single, double, expressing, theirs


@pytest.mark.parametrize("method", [gib.NONE, gib.L2])
@pytest.mark.parametrize("name", gib.SHAPE_CASES)
def test_shapes(restatement, name, method):
    single, double, expressing, theirs = check_case(restatement, name, method)
    if name == "random-1x255":                      # one cell: R = 0 for every gene (p = c * (1 / c) may be one unit below 1)
        assert np.all(np.abs(double) <= gib.bound(1, 1.))
        # (and the shape whose cell has more entries than a wave has lanes: entriesKernel's second, third and fourth stride)
        assert np.diff(gib.case(name)[0].astype(np.int64)).max() == 255
    if name == "random-300x600":                    # many cells of 110 to 190 entries: the second and third stride in every wave
        lengths = np.diff(gib.case(name)[0].astype(np.int64))
        assert lengths.min() > 64 and (lengths > 128).sum() > 100
    if name == "segments":
        assert expressing.tolist() == [gib.CHUNK - 1, gib.CHUNK, gib.CHUNK + 1, 3 * gib.CHUNK + 5, 0]
    if name == "everywhere":
        assert expressing.tolist() == [70000, 1, 0]


@pytest.mark.parametrize("method", [gib.NONE, gib.L1, gib.L2])
def test_three_normalizations(restatement, method):
    check_case(restatement, "random-1000x257", method)


@pytest.mark.parametrize("method", [gib.NONE, gib.L1, gib.L2])
def test_odd_content(restatement, method):
    single, double, expressing, theirs = check_case(restatement, "odd", method)
    toc, data, genes = gib.case("odd")
    # a stored zero counts as expressing and adds no term; an inf count gives NaN; one cell gives log2(N); none gives log2(N)
    assert expressing[4] == 3 and theirs["positive"][4] == 0
    assert expressing[3] == theirs["positive"][3] + 1
    assert np.isnan(single[5]) and np.isnan(double[5])
    assert expressing[6] == 1 and abs(double[6] - np.log2(300.)) < 1e-12
    assert expressing[11] == 0 and bits(single[11:12])[0] == bits(np.float32([np.log(300.) / np.log(2.)]))[0]


@pytest.mark.parametrize("method", [gib.NONE, gib.L1, gib.L2])
def test_empty_cell(restatement, method):
    single, double, expressing, theirs = check_case(restatement, "empty-cell", method)
    # (under L1 / L2 the empty cell's inverse is inf: the reference's 0 * inf makes every gene with a positive entry NaN)
    assert np.all(np.isnan(single) == ((method != gib.NONE) & (theirs["positive"] > 0)))


@pytest.mark.parametrize("name", ["everywhere", "random-1000x257", "genes-65537"])
def test_determinism(restatement, name):
    toc, data, genes = gib.case(name)
    norm = gib.norm_inverse_for(restatement, toc, data, gib.L2)
    first = capi.gene_information_content(toc, data, genes, norm)
    again = capi.gene_information_content(toc, data, genes, norm)
    device = capi.dev_gene_information_content(toc, data, genes, norm)
    capi.load().em2_set_gene_information_max_blocks(2)              # 8 waves stride over the cells and over the chunks
    try:
        small = capi.gene_information_content(toc, data, genes, norm)
    finally:
        capi.load().em2_set_gene_information_max_blocks(0)
    for other in (again, device, small):
        assert np.array_equal(bits(first[0]), bits(other[0])) and np.array_equal(bits(first[1]), bits(other[1]))
        assert np.array_equal(first[2], other[2])


def test_bad_input_is_an_argument_error():
    toc, data, genes = gib.case("odd")
    with pytest.raises(RuntimeError, match="em2_gene_information_content: a local gene id is not below geneCount"):
        capi.gene_information_content(toc, data, 5)
    unsorted = data.copy()
    unsorted["gene"][[0, 1]] = unsorted["gene"][[1, 0]]
    with pytest.raises(RuntimeError, match="not strictly ascending"):
        capi.gene_information_content(toc, unsorted, genes)


# ---- the facade ----

GENE_IDS = np.array([0, 2, 3, 5, 8, 13, 21, 34, 55, 89, 144, 200, 233, 256], dtype=np.uint32)


@pytest.fixture
def matrix(tmp_path):
    """The 1000 x 257 input as a data directory with a proper subset of the genes and of the cells."""
    toc, data, genes = gib.case("random-1000x257")
    directory = str(tmp_path / "data")
    files.create_directory(directory, genes, toc, data)
    files.add_gene_set(directory, "Some", GENE_IDS)
    files.add_cell_set(directory, "Odd", np.arange(1, 1000, 2, dtype=np.uint32))
    return directory


def subset_csr(directory, gene_set, cell_set):
    e = ExpressionMatrix(directory)
    genes, toc, data = e._subset(gene_set, cell_set)
    cells = e._cell_set(cell_set)
    e.close()
    return genes, toc, data, cells


@pytest.mark.parametrize("method", [NormalizationMethod.none, NormalizationMethod.L1, NormalizationMethod.L2])
def test_information_content_gene_set(restatement, matrix, method):
    toc, data, _ = gib.case("random-1000x257")
    genes, sub_toc, sub_data, cells = subset_csr(matrix, "Some", "Odd")
    n1, n2 = restatement.cell_norm_inverses(toc, data)                    # of the WHOLE cells, all 257 genes
    norm = None if method == 0 else (n1 if method == 1 else n2)[cells]
    e = ExpressionMatrix(matrix)
    floats = e.computeGeneInformationContent("Some", "Odd", method)
    single, _, _ = capi.gene_information_content(sub_toc, sub_data, genes, norm)
    assert np.array_equal(bits(floats), bits(single))
    # the threshold in the middle of the widest gap between neighbouring R values
    R, n, weight = gib.higher_precision(sub_toc, sub_data, genes, norm)
    ordered = np.sort(R)
    at = int(np.argmax(np.diff(ordered)))
    threshold = float(ordered[at] + ordered[at + 1]) / 2
    assert ordered[at + 1] - ordered[at] > 2 * np.spacing(np.float32(ordered[at + 1]))
    e.createGeneSetUsingInformationContent("Some", "Odd", method, threshold, "High")
    created = e.getGeneSetGenes("High")
    assert created == GENE_IDS[floats.astype(np.float64) > threshold].tolist()
    theirs = restatement.gene_information_content(sub_toc, sub_data, genes, norm)
    assert created == GENE_IDS[theirs["single"].astype(np.float64) > threshold].tolist()
    assert 0 < len(created) < len(GENE_IDS)
    # the files are those add_gene_set writes for the same ids
    files.add_gene_set(matrix, "Written", created)
    for part in ("GlobalIds", "LocalIds"):
        assert open(os.path.join(matrix, "GeneSet-High-" + part), "rb").read() == open(os.path.join(matrix, "GeneSet-Written-" + part), "rb").read()
    e.close()


def test_well_expressed_gene_set(matrix):
    genes, sub_toc, sub_data, cells = subset_csr(matrix, "Some", "Odd")
    counts = np.bincount(sub_data["gene"], minlength=genes)
    middle = int(np.sort(counts)[len(counts) // 2])
    e = ExpressionMatrix(matrix)
    for i, minimum in enumerate((0, 1, middle, len(cells) + 1)):
        e.createWellExpressedGeneSet("Some", "Odd", "W%d" % i, minimum)
        assert e.getGeneSetGenes("W%d" % i) == GENE_IDS[counts >= minimum].tolist()
    assert e.getGeneSetGenes("W0") == GENE_IDS.tolist() and e.getGeneSetGenes("W3") == []
    assert 0 < len(e.getGeneSetGenes("W2")) < len(GENE_IDS)
    e.close()


def test_created_set_feeds_a_search_and_can_be_removed(matrix):
    genes, sub_toc, sub_data, cells = subset_csr(matrix, "AllGenes", "Odd")
    median = int(np.median(np.bincount(sub_data["gene"], minlength=genes)))
    e = ExpressionMatrix(matrix)
    e.createWellExpressedGeneSet("AllGenes", "Odd", "Well", median)
    ids = e.getGeneSetGenes("Well")
    assert 0 < len(ids) < 257
    files.add_gene_set(matrix, "Written", ids)
    e.findSimilarPairs4(geneSetName="Well", cellSetName="Odd", similarPairsName="A", k=10, lshCount=256)      # by name, same object
    e.close()
    e = ExpressionMatrix(matrix)
    e.findSimilarPairs4(geneSetName="Written", cellSetName="Odd", similarPairsName="B", k=10, lshCount=256)
    kA, pairsA, usedA = files.read_similar_pairs(matrix, "A")
    kB, pairsB, usedB = files.read_similar_pairs(matrix, "B")
    assert usedA.sum() > 0 and np.array_equal(usedA, usedB) and pairsA.tobytes() == pairsB.tobytes()
    with pytest.raises(RuntimeError, match=r"^Gene set Well already exists\.$"):
        e.createWellExpressedGeneSet("AllGenes", "Odd", "Well", 1)
    e.removeGeneSet("Well")
    for part in ("GlobalIds", "LocalIds"):
        assert not os.path.exists(os.path.join(matrix, "GeneSet-Well-" + part))
    e.createWellExpressedGeneSet("AllGenes", "Odd", "Well", 1)             # the name is free
    e.close()


def test_cells_file_decides_the_norms(restatement, matrix):
    toc, data, _ = gib.case("random-1000x257")
    genes, sub_toc, sub_data, cells = subset_csr(matrix, "Some", "Odd")
    n1, n2 = restatement.cell_norm_inverses(toc, data)
    rng = np.random.default_rng(2)
    file1, file2 = n1 * rng.uniform(0.5, 2.0, 1000), n2 * rng.uniform(0.5, 2.0, 1000)
    e = ExpressionMatrix(matrix)
    recomputed = e.computeGeneInformationContent("Some", "Odd", NormalizationMethod.L2)
    files.add_cells(matrix, file1, file2)
    for method, norm in ((NormalizationMethod.L1, file1), (NormalizationMethod.L2, file2)):
        floats = e.computeGeneInformationContent("Some", "Odd", method)
        single, _, _ = capi.gene_information_content(sub_toc, sub_data, genes, norm[cells])
        assert np.array_equal(bits(floats), bits(single))
    assert not np.array_equal(bits(floats), bits(recomputed))
    e.close()


@pytest.mark.parametrize("name,method", [("odd", NormalizationMethod.none), ("odd", NormalizationMethod.L1), ("odd", NormalizationMethod.L2),
                                         ("empty-cell", NormalizationMethod.L2)])
def test_nan_passes_no_threshold(restatement, tmp_path, name, method):
    """An inf count (gene 5 of 'odd') and, under L2, the empty cell's 0 * inf (every expressed gene of 'empty-cell') give NaN on
    both sides; the float > double comparison of src/ExpressionMatrix.cpp:2077 is false for NaN, so even the lowest threshold
    leaves those genes out and takes every other gene."""
    toc, data, genes = gib.case(name)
    directory = str(tmp_path / "data")
    files.create_directory(directory, genes, toc, data)
    e = ExpressionMatrix(directory)
    floats = e.computeGeneInformationContent("AllGenes", "AllCells", method)
    theirs = restatement.gene_information_content(toc, data, genes, gib.norm_inverse_for(restatement, toc, data, int(method)))
    assert np.array_equal(np.isnan(floats), np.isnan(theirs["single"])) and np.isnan(floats).any()
    e.createGeneSetUsingInformationContent("AllGenes", "AllCells", method, -1e30, "NotNaN")
    assert e.getGeneSetGenes("NotNaN") == np.nonzero(~np.isnan(theirs["single"]))[0].tolist()
    if name == "odd":
        assert 5 not in e.getGeneSetGenes("NotNaN") and len(e.getGeneSetGenes("NotNaN")) == genes - 1
    else:
        assert e.getGeneSetGenes("NotNaN") == np.nonzero(theirs["positive"] == 0)[0].tolist()
    e.close()


def test_cell_set_with_a_repeated_id(restatement, matrix):
    """A sorted cell set may name a cell twice (the reference's sets are only sorted): the rows are those the ids name."""
    toc, data, _ = gib.case("random-1000x257")
    files.add_cell_set(matrix, "Twice", np.array([4, 4, 6, 7, 7, 9], dtype=np.uint32))
    genes, sub_toc, sub_data, cells = subset_csr(matrix, "Some", "Twice")
    assert cells.tolist() == [4, 4, 6, 7, 7, 9]
    _, n2 = restatement.cell_norm_inverses(toc, data)
    e = ExpressionMatrix(matrix)
    floats = e.computeGeneInformationContent("Some", "Twice", NormalizationMethod.L2)
    single, _, _ = capi.gene_information_content(sub_toc, sub_data, genes, n2[cells])
    assert np.array_equal(bits(floats), bits(single))
    e.close()


def test_device_entry_refuses_a_toc_that_descends():
    toc, data, genes = gib.case("odd")
    descending = toc.copy()
    descending[[1, 2]] = descending[[2, 1]]
    assert descending[1] > descending[2]
    with pytest.raises(RuntimeError, match="em2_dev_gene_information_content: toc .* not ascending"):
        capi.dev_gene_information_content(descending, data, genes)
