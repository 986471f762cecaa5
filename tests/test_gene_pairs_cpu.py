"""findSimilarGenePairs0 without a GPU: the C++ restatement the device is compared with
(tests/native/em2_gene_pairs_restatement.cpp) is itself checked against an independent numpy statement of
src/ExpressionMatrixFindSimilarGenePairs.cpp:77-188 (r bit for bit; the stored pairs exactly on an input without ties), a tie
input shows that its selection is not a plain top-k, and the SimilarGenePairs-* files, the facade's argument errors and
writeCsv are checked through the library."""
import inspect
import os

import numpy as np
import pytest

import fsp0_binding
import gene_pairs_binding as gpb
from expressionmatrix2_amd import ExpressionMatrix, NormalizationMethod, capi, files


@pytest.fixture(scope="module")
def restatement():
    return gpb.load()


def numpy_gene_correlations(toc, data, gene_count, method):
    """Steps 1-5 written from the reference's lines alone: every float operation is a numpy float32 operation (one rounding
    each, products and sums separate), every double sum runs over the cells or entries in ascending order."""
    cells = len(toc) - 1
    f32, f64 = np.float32, np.float64
    dense = gpb.to_dense(toc, data, gene_count)
    with np.errstate(all="ignore"):
        for cell in range(cells):
            sum1, sum2 = f64(0.), f64(0.)
            for p in range(int(toc[cell]), int(toc[cell + 1])):
                count = f32(data["count"][p])
                sum1 = sum1 + f64(count)
                sum2 = sum2 + f64(f32(count * count))
            if method != gpb.NONE:
                scaling = sum1 if method == gpb.L1 else np.sqrt(sum2)
                if scaling != 0.:
                    dense[cell, :] = dense[cell, :] * f32(f64(1.) / scaling)
        total = np.zeros(gene_count, dtype=f64)
        for cell in range(cells):
            total = total + dense[cell].astype(f64)
        average = (total / f64(cells)).astype(f32)
        x = dense - average[None, :]
        squares = np.zeros(gene_count, dtype=f64)
        for cell in range(cells):
            squares = squares + (x[cell] * x[cell]).astype(f64)
        x = x * (f64(1.) / np.sqrt(squares)).astype(f32)[None, :]
        r = np.zeros((gene_count, gene_count), dtype=f32)
        for cell in range(cells):
            r = r + np.outer(x[cell], x[cell])                   # float32 products, then float32 sums
    assert x.dtype == f32 and r.dtype == f32
    np.fill_diagonal(r, 0.)
    return r


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize("cells,genes,density,seed,method", [
    (37, 50, 0.3, 3, gpb.L2),
    (64, 33, 0.2, 8, gpb.L1),
    (130, 70, 0.1, 21, gpb.NONE),
    (1, 12, 0.9, 5, gpb.L2),                       # one cell: no gene has variance
])
def test_restatement_equals_numpy_bit_for_bit(restatement, cells, genes, density, seed, method):
    toc, data = fsp0_binding.clustered(cells, genes, density, seed=seed, cluster_count=3, non_integer=True)
    gene, sim, used, r = restatement.find_similar_gene_pairs0(toc, data, genes, method, 5, 0.1)
    expected = numpy_gene_correlations(toc, data, genes, method)
    assert np.array_equal(bits(r), bits(expected))
    assert np.array_equal(bits(r), bits(r.T))                    # symmetric bit for bit
    if cells > 1:
        finite = r[np.isfinite(r)]
        assert len(finite) > genes and np.abs(finite).max() <= 1.0 + 1e-5


@pytest.mark.parametrize("k,thr,method", [(4, 0.1, gpb.L2), (100, 0.2, gpb.L2), (7, -1.0, gpb.L1), (3, 0.0, gpb.NONE), (0, 0.1, gpb.L2)])
def test_stored_pairs_on_an_input_without_ties(restatement, k, thr, method):
    """Without ties among a gene's candidates keepBest and sort have one possible outcome: the k largest, descending."""
    genes = 60
    toc, data = fsp0_binding.clustered(90, genes, 0.25, seed=11, cluster_count=4, non_integer=True)
    gene, sim, used, r = restatement.find_similar_gene_pairs0(toc, data, genes, method, k, thr)
    expected = numpy_gene_correlations(toc, data, genes, method)
    stored = 0
    for g0 in range(genes):
        candidates = [(float(expected[g0, g1]), g1) for g1 in range(genes) if g1 != g0 and np.float64(expected[g0, g1]) > thr]
        assert len(set(value for value, _ in candidates)) == len(candidates)           # (the input has no ties)
        candidates.sort(reverse=True)
        candidates = candidates[:k]
        assert used[g0] == len(candidates)
        assert gene[g0, :used[g0]].tolist() == [g1 for _, g1 in candidates]
        assert np.array_equal(bits(sim[g0, :used[g0]]), bits(np.array([v for v, _ in candidates], dtype=np.float32)))
        assert not gene[g0, used[g0]:].any() and not bits(sim[g0, used[g0]:]).any()
        stored += len(candidates)
    assert stored > 0 or k == 0


def test_tie_input_is_not_a_plain_top_k(restatement):
    """On the tie input the result of nth_element + sort is NOT 'the k best by (similarity desc, id asc)': which of several
    tied partners survive and in what order they are stored is the algorithms' business.  Otherwise the GPU tie cases would
    prove nothing."""
    toc, data, genes = gpb.tie_input()
    for k, thr in [(3, 0.0), (5, 0.2), (12, -1.0)]:
        gene, sim, used, r = restatement.find_similar_gene_pairs0(toc, data, genes, gpb.L2, k, thr)
        top_gene, top_sim, top_used = gpb.best_k_by_similarity_then_id(r, k, thr)
        assert np.array_equal(used, top_used)                                   # the counts agree
        assert np.array_equal(bits(sim), bits(top_sim))                         # and the stored values, as multisets in order
        differing = [g for g in range(genes) if not np.array_equal(gene[g], top_gene[g])]
        assert len(differing) >= 5, (k, thr, len(differing))
        assert (used == k).sum() > genes // 2


def test_no_variance_genes_store_nothing(restatement):
    """An all-zero gene and a gene with the same count in every cell have no variance: NaN (or inf) by IEEE rules, nothing is
    special-cased, and NaN passes no threshold."""
    toc, data = fsp0_binding.clustered(30, 20, 0.3, seed=2, cluster_count=2, non_integer=True)
    dense = gpb.to_dense(toc, data, 20)
    dense[:, 4] = 0.
    dense[:, 9] = 3.25
    toc, data = gpb.dense_to_csr(dense)
    gene, sim, used, r = restatement.find_similar_gene_pairs0(toc, data, 20, gpb.NONE, 50, -1.0)
    assert np.isnan(r[4, [g for g in range(20) if g != 4]]).all() and used[4] == 0
    assert used[9] == 0 and not np.isin(gene[:, :], [4, 9])[used[:, None] > np.arange(50)[None, :]].any()
    assert np.array_equal(bits(r), bits(numpy_gene_correlations(toc, data, 20, gpb.NONE)))


# ---- files and facade ----

@pytest.fixture()
def data_dir(tmp_path):
    d = str(tmp_path / "data")
    cells, genes = 40, 120
    toc, data = fsp0_binding.clustered(cells, genes, 0.1, seed=33, cluster_count=3, non_integer=True)
    files.create_directory(d, genes, toc, data)
    files.add_gene_set(d, "Some", np.unique((np.arange(70) * 5) % genes).astype(np.uint32))
    files.add_cell_set(d, "Odd", np.arange(1, cells, 2, dtype=np.uint32))
    files.add_gene_set(d, "NoGenes", np.zeros(0, dtype=np.uint32))
    files.add_cell_set(d, "NoCells", np.zeros(0, dtype=np.uint32))
    return d


def test_similar_gene_pairs_files_round_trip(restatement, data_dir):
    e = ExpressionMatrix(data_dir)
    n_genes, toc, data = e._subset("Some", "Odd")
    k = 6
    gene, sim, used, _ = restatement.find_similar_gene_pairs0(toc, data, n_genes, gpb.L1, k, 0.1)
    pairs = np.zeros((n_genes, k), dtype=capi.PAIR_DTYPE)
    pairs["cell"], pairs["similarity"] = gene, sim
    files.write_similar_gene_pairs(data_dir, "G", "Some", "Odd", k, NormalizationMethod.L1, pairs, used)
    for part in ("Info", "Pairs", "GeneInfo"):
        assert os.path.exists(os.path.join(data_dir, "SimilarGenePairs-G-" + part))
    k2, pairs2, used2 = files.read_similar_gene_pairs(data_dir, "G")
    assert k2 == k and np.array_equal(used2, used) and used.sum() > 0
    assert np.array_equal(pairs2["cell"], gene) and np.array_equal(bits(pairs2["similarity"]), bits(sim))
    info = files.similar_gene_pairs_info(data_dir, "G")
    gene_ids = np.unique((np.arange(70) * 5) % 120).astype(np.uint32)
    cell_ids = np.arange(1, 40, 2, dtype=np.uint32)
    assert info == {"k": k, "geneCount": n_genes, "geneSetName": "Some", "geneSetHash": capi.murmur_hash_64a(gene_ids),
                    "cellSetName": "Odd", "cellSetHash": capi.murmur_hash_64a(cell_ids),
                    "normalizationMethod": int(NormalizationMethod.L1)}
    # the Info object on disk: a 256-byte header (objectSize at byte 8), then SimilarGenePairs::Info: 544 bytes, k at 0, the
    # names as {length byte, 255 characters} at 8 and 272, the hashes at 264 and 528, the enum at 536, zero padding after it
    raw = open(os.path.join(data_dir, "SimilarGenePairs-G-Info"), "rb").read()
    assert int(np.frombuffer(raw, dtype="<u8", count=1, offset=8)[0]) == 544
    record = raw[256:256 + 544]
    assert int(np.frombuffer(record, dtype="<u8", count=1, offset=0)[0]) == k
    assert record[8] == 4 and record[9:13] == b"Some" and record[272] == 3 and record[273:276] == b"Odd"
    assert int(np.frombuffer(record, dtype="<u8", count=1, offset=264)[0]) == info["geneSetHash"]
    assert int(np.frombuffer(record, dtype="<u8", count=1, offset=528)[0]) == info["cellSetHash"]
    assert int(np.frombuffer(record, dtype="<i4", count=1, offset=536)[0]) == 1 and record[540:544] == b"\0\0\0\0"
    # the consistency checks of the existing-object constructor, and removal
    with pytest.raises(RuntimeError, match="length inconsistent with gene set AllGenes"):
        files.write_similar_gene_pairs(data_dir, "H", "AllGenes", "Odd", k, 0, pairs, used)
    files.add_gene_set(data_dir, "Some", gene_ids[:-1])                       # the gene set changes under the object
    with pytest.raises(RuntimeError, match="Hash for gene set Some is not consistent"):
        files.read_similar_gene_pairs(data_dir, "G")
    with pytest.raises(RuntimeError, match="Error removing similar gene pairs object G"):
        e.removeSimilarGenePairs("G")
    files.add_gene_set(data_dir, "Some", gene_ids)
    e.removeSimilarGenePairs("G")
    for part in ("Info", "Pairs", "GeneInfo"):
        assert not os.path.exists(os.path.join(data_dir, "SimilarGenePairs-G-" + part))
    with pytest.raises(RuntimeError, match="Error removing similar gene pairs object G"):
        e.removeSimilarGenePairs("G")


def test_facade_argument_errors(data_dir):
    e = ExpressionMatrix(data_dir)
    assert [m.name for m in NormalizationMethod] == ["none", "L1", "L2"] and int(NormalizationMethod.L2) == 2
    for kwargs, text in [(dict(geneSetName="Nope"), "Gene set Nope does not exist."),
                         (dict(geneSetName="NoGenes"), "Gene set NoGenes is empty."),
                         (dict(cellSetName="Nope"), "Cell set Nope does not exist."),
                         (dict(cellSetName="NoCells"), "Cell set NoCells is empty."),
                         (dict(geneSetName="Nope", cellSetName="Nope"), "Gene set Nope does not exist.")]:
        with pytest.raises(RuntimeError, match=text):
            e.findSimilarGenePairs0(similarGenePairsName="X", **kwargs)
        assert not os.path.exists(os.path.join(data_dir, "SimilarGenePairs-X-Info"))
    with pytest.raises(TypeError):
        e.findSimilarGenePairs0()
    with pytest.raises(NotImplementedError, match="writeCsv"):
        e.findSimilarGenePairs0(similarGenePairsName="X", writeCsv=True)
    with pytest.raises(ValueError):
        e.findSimilarGenePairs0(similarGenePairsName="X", normalizationMethod=3)
    with pytest.raises(ValueError):
        e.findSimilarGenePairs0(similarGenePairsName="X", normalizationMethod=None)
    default = inspect.signature(ExpressionMatrix.findSimilarGenePairs0).parameters["normalizationMethod"].default
    assert default is NormalizationMethod.L2
    assert not os.path.exists(os.path.join(data_dir, "SimilarGenePairs-X-Info"))


def test_host_entry_argument_checks():
    """The checks of em2_find_similar_gene_pairs0 that need no device answer before any device call."""
    toc, data = fsp0_binding.clustered(8, 30, 0.3, seed=1)
    with pytest.raises(RuntimeError, match="invalid normalization method"):
        capi.find_similar_gene_pairs0(toc, data, 30, normalization_method=3)
    with pytest.raises(RuntimeError, match="allSimilarities is an aid for at most 8192 genes"):
        toc1 = np.array([0, 0], dtype=np.uint64)
        pairs = np.zeros((8193, 1), dtype=capi.PAIR_DTYPE)
        used = np.zeros(8193, dtype=np.uint32)
        dummy = np.zeros(1, dtype=np.float32)                    # (refused before anything is written)
        capi.check(capi.load().em2_find_similar_gene_pairs0(capi._ptr(toc1), None, 1, 8193, 2, 1, 0.2, capi._ptr(pairs),
                                                            capi._ptr(used), capi._ptr(dummy)))
    if capi.device_count() == 0:
        with pytest.raises(RuntimeError, match="no HIP device"):
            capi.find_similar_gene_pairs0(toc, data, 30)
