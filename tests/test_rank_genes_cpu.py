"""The rank-sum marker genes on the CPU: the one-thread C++ restatement (tests/native/em2_rank_genes_restatement.cpp, a sort of
all N values per gene) against an independent numpy statement (dense columns, np.unique), integers and doubles bit for bit;
both against scipy where it imports; the stand-alone program of the statistics header; the argument checks of
the C entries that answer without a device; the facade's signatures."""
import inspect
import os
import subprocess

import numpy as np
import pytest

import rank_genes_binding as rgb
from expressionmatrix2_amd import capi
from expressionmatrix2_amd.expression_matrix import ExpressionMatrix, NormalizationMethod

INVALID = 1

CASES = ["random-1x1x1", "random-2x3x2", "random-63x33x3", "random-64x1x2", "random-65x70x65", "random-300x33x3", "odd", "chunks"]


@pytest.fixture(scope="module")
def restatement():
    return rgb.load()


@pytest.mark.parametrize("name", CASES)
def test_the_restatement_equals_the_numpy_statement(restatement, name):
    toc, data, genes, group, groups = rgb.case(name)
    mine = restatement.rank_genes(toc, data, genes, group, groups)
    rgb.assert_same(mine, rgb.numpy_statement(toc, data, genes, group, groups), name)


@pytest.mark.parametrize("method", [1, 2])
@pytest.mark.parametrize("name", ["random-65x70x65", "random-300x33x3"])
def test_normalised_values_and_an_empty_cell(restatement, name, method):
    """Cell 1 stores nothing: its norm inverse is inf, and its values are +0 all the same."""
    toc, data, genes, group, groups = rgb.case(name)
    norm = rgb.norm_inverses(toc, data)[method - 1]
    assert np.isinf(norm[1]) and toc[1] == toc[2]
    mine = restatement.rank_genes(toc, data, genes, group, groups, norm)
    rgb.assert_same(mine, rgb.numpy_statement(toc, data, genes, group, groups, norm), name)
    assert not np.array_equal(mine["rankSum2"], restatement.rank_genes(toc, data, genes, group, groups)["rankSum2"])


def test_the_odd_case_holds_what_it_says():
    toc, data, genes, group, groups = rgb.case("odd")
    dense = np.zeros((len(toc) - 1, genes), dtype=np.float32)
    rows = np.repeat(np.arange(len(toc) - 1), np.diff(toc.astype(np.int64)))
    dense[rows, data["gene"]] = data["count"]
    stored = np.zeros(dense.shape, dtype=bool)
    stored[rows, data["gene"]] = True
    assert (stored[:, 0] & (dense[:, 0] == 0)).any() and (dense[:, 0] > 0).any()
    assert (dense[:, 1] < 0).any() and np.signbit(dense[2, 1]) and dense[2, 1] == 0 and stored[3, 1]
    assert np.isposinf(dense[4, 2]) and np.isneginf(dense[5, 2])
    assert not stored[:, 3].any() and stored[:, 4].any() and not dense[:, 4].any()
    assert stored[np.arange(120) != 7, 5].all() and len(np.unique(dense[:, 5])) == 2 and len(np.unique(dense[:, 6])) == dense.shape[0]
    assert toc[7] == toc[8] and (group == rgb.NO_GROUP).any() and not (group == 3).any()
    theirs = rgb.numpy_statement(toc, data, genes, group, groups)
    # a gene stored nowhere or of zeros only: one tie group of N, no variance
    N = dense.shape[0]
    assert theirs["tieSum"][5] == (N - 1) ** 3 - (N - 1)
    for g in (3, 4):
        assert theirs["tieSum"][g] == N ** 3 - N and not theirs["zScore"][g].any() and np.all(theirs["auc"][g][:3] == 0.5)
    assert theirs["groupSize"][3] == 0 and not theirs["zScore"][:, 3].any() and np.all(theirs["auc"][:, 3] == 0.5)
    assert theirs["tieSum"][6] == 0


def test_one_group_that_is_the_whole_universe(restatement):
    toc, data, genes, _, _ = rgb.case("random-63x33x3")
    group = np.zeros(63, dtype=np.uint32)
    mine = restatement.rank_genes(toc, data, genes, group, 1)
    rgb.assert_same(mine, rgb.numpy_statement(toc, data, genes, group, 1), "K = 1")
    assert mine["groupSize"].tolist() == [63] and not mine["zScore"].any() and np.all(mine["auc"] == 0.5)
    assert np.all(mine["rankSum2"] == 63 * 64)                           # twice 1 + ... + N, whatever the ties


def test_nan_is_refused(restatement):
    toc, data, genes, group, groups = rgb.case("random-63x33x3")
    data = data.copy()
    data["count"][5] = np.nan
    with pytest.raises(ValueError):
        restatement.rank_genes(toc, data, genes, group, groups)
    with pytest.raises(ValueError):
        rgb.numpy_statement(toc, data, genes, group, groups)


@pytest.mark.parametrize("name", ["random-63x33x3", "odd", "chunks"])
def test_against_scipy(restatement, name):
    """scipy.stats.mannwhitneyu(use_continuity=False, method="asymptotic") per gene and group: U, and the two-sided p at a
    relative 1e-12 (the formula has under ten roundings after exact integers).  z itself is not among scipy's results: its
    sign is that of U - n m / 2, and |z| is held against isf(p / 2) of scipy's p, which turns a relative error d of p into
    d sf(z) / (z pdf(z)) of z -- under 12 d for p < 0.9, so the relative 1e-12 holds there; above (|z| < 0.13) the same error
    is under 1.3 d in absolute terms, and the bound is an absolute 1e-12."""
    stats = pytest.importorskip("scipy.stats")
    toc, data, genes, group, groups = rgb.case(name)
    mine = restatement.rank_genes(toc, data, genes, group, groups)
    dense = rgb.dense_values(toc, data, genes)
    p_mine = rgb.p_values(mine["zScore"])
    checked = 0
    for g in range(genes):
        for k in range(groups):
            x, y = dense[group == k, g].astype(np.float64), dense[group != k, g].astype(np.float64)
            if len(x) == 0 or len(y) == 0:
                continue
            n, m = len(x), len(y)
            u2 = int(mine["rankSum2"][g, k]) - n * (n + 1)
            if len(np.unique(dense[:, g])) == 1:                         # no variance: scipy divides by zero, here z = 0
                assert mine["zScore"][g, k] == 0. and p_mine[g, k] == 1.
                continue
            theirs = stats.mannwhitneyu(x, y, use_continuity=False, method="asymptotic", alternative="two-sided")
            assert 2. * theirs.statistic == u2
            assert mine["auc"][g, k] == pytest.approx(theirs.statistic / (n * m), rel=1e-15)
            assert p_mine[g, k] == pytest.approx(theirs.pvalue, rel=1e-12, abs=0.)
            assert np.sign(mine["zScore"][g, k]) == np.sign(2 * u2 - 2 * n * m)
            z_theirs = stats.norm.isf(theirs.pvalue / 2.)
            if theirs.pvalue < 0.9:
                assert abs(mine["zScore"][g, k]) == pytest.approx(z_theirs, rel=1e-12, abs=0.)
            else:
                assert abs(mine["zScore"][g, k]) == pytest.approx(z_theirs, rel=0., abs=1e-12)
            checked += 1
    assert checked >= genes


def test_the_stand_alone_program_of_the_statistics_header(tmp_path):
    """tests/native/em2_rank_genes_host_main.cpp runs the header over its edge cases.  Built plainly here; the build line in
    its header comment adds the sanitizers, for a run by hand on a CPU."""
    source = os.path.join(rgb.NATIVE_DIR, "em2_rank_genes_host_main.cpp")
    program = str(tmp_path / "em2_rank_genes_host_main")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-o", program, source], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([program], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "rank genes host checks ok" in run.stdout
    assert "-fsanitize=address,undefined" in open(source).read()


def call(name, *arguments):
    lib = capi.load()
    rc = getattr(lib, name)(*[a.ctypes.data if isinstance(a, np.ndarray) else a for a in arguments])
    return rc, lib.em2_last_error().decode()


TOC = np.array([0, 1, 2, 3, 4], dtype=np.uint64)
DATA = np.array([(0, 1.0), (1, 2.0), (2, 1.0), (0, 3.0)], dtype=capi.COUNT_DTYPE)
GROUP = np.array([0, 1, 0, 1], dtype=np.uint32)
U32, U64 = np.zeros(64, dtype=np.uint32), np.zeros(64, dtype=np.uint64)


def test_the_argument_checks_answer_without_a_device():
    host = lambda *a: call("em2_rank_genes", *a)
    assert host(TOC, DATA, 4, 0, None, GROUP, 2, U32, U32, U64, U64, None, None) == (INVALID, "em2_rank_genes: geneCount must be positive")
    assert host(TOC, DATA, 0, 3, None, GROUP, 2, U32, U32, U64, U64, None, None) == (INVALID, "em2_rank_genes: cellCount must be positive")
    assert host(TOC, DATA, 4, 3, None, GROUP, 0, U32, U32, U64, U64, None, None) == (INVALID, "em2_rank_genes: groupCount must be positive")
    assert host(TOC, DATA, 4, 3, None, None, 2, U32, U32, U64, U64, None, None) == (INVALID, "em2_rank_genes: null pointer")
    assert host(TOC, DATA, 4, 3, None, GROUP, 2, U32, U32, None, U64, None, None) == (INVALID, "em2_rank_genes: null pointer")
    descending = np.array([0, 2, 1, 3, 4], dtype=np.uint64)
    assert host(descending, DATA, 4, 3, None, GROUP, 2, U32, U32, U64, U64, None, None) == (INVALID, "em2_rank_genes: toc is not ascending")
    dev = lambda *a: call("em2_dev_rank_genes", *a)
    assert dev(TOC, DATA, 4, 3, 4, None, None, 2, U32, U32, U64, U64, U64, 1 << 30, None) == (INVALID, "em2_dev_rank_genes: null pointer")
    assert dev(TOC, DATA, 4, 3, 4, None, GROUP, 0, U32, U32, U64, U64, U64, 1 << 30, None) == (INVALID, "em2_dev_rank_genes: groupCount must be positive")


def test_the_limits_are_refused_before_anything_is_read():
    """More than 2^21 cells, 2^32 entries, geneCount * groupCount above 2^28: EM2_ERROR_UNSUPPORTED from both entries, whatever
    the pointers hold (the device entry reads none of them, the host entry its toc alone)."""
    unsupported = capi.EM2_ERROR_UNSUPPORTED
    cells = (1 << 21) + 1
    for args, text in [((cells, 3, 4, None, GROUP, 2), "more than 2^21 cells"), ((4, 3, 1 << 32, None, GROUP, 2), "2^32 entries or more"),
                       ((4, 1 << 20, 4, None, GROUP, 257), "geneCount * groupCount is above 2^28")]:
        rc, message = call("em2_dev_rank_genes", TOC, DATA, *args, U32, U32, U64, U64, U64, 1 << 30, None)
        assert rc == unsupported and message.startswith("em2_dev_rank_genes: " + text)
        assert capi.load().em2_dev_rank_genes_workspace(args[0], args[1], args[2], args[5]) == 0
    long_toc = np.zeros(cells + 1, dtype=np.uint64)
    rc, message = call("em2_rank_genes", long_toc, DATA, cells, 3, None, GROUP, 2, U32, U32, U64, U64, None, None)
    assert rc == unsupported and message.startswith("em2_rank_genes: more than 2^21 cells")
    rc, message = call("em2_rank_genes", np.array([0, 1 << 32], dtype=np.uint64), DATA, 1, 3, None, GROUP, 2, U32, U32, U64, U64, None, None)
    assert rc == unsupported and message.startswith("em2_rank_genes: 2^32 entries or more")
    rc, message = call("em2_rank_genes", TOC, DATA, 4, 1 << 20, None, GROUP, 257, U32, U32, U64, U64, None, None)
    assert rc == unsupported and message.startswith("em2_rank_genes: geneCount * groupCount is above 2^28")


def test_the_facade_signatures():
    parameters = lambda f: list(inspect.signature(f).parameters)[1:]
    assert parameters(ExpressionMatrix.rankGenesByMetaData) == ["geneSetName", "cellSetName", "metaDataName", "normalizationMethod"]
    assert parameters(ExpressionMatrix.rankGenesByClusterGraph) == ["clusterGraphName", "geneSetName", "normalizationMethod"]
    assert parameters(ExpressionMatrix.compareCellSets) == ["geneSetName", "cellSetName0", "cellSetName1", "normalizationMethod"]
    defaults = inspect.signature(ExpressionMatrix.rankGenesByMetaData).parameters
    assert defaults["geneSetName"].default == "AllGenes" and defaults["cellSetName"].default == "AllCells"
    assert defaults["normalizationMethod"].default == NormalizationMethod.L2


def test_top_genes():
    from expressionmatrix2_amd.expression_matrix import topGenes
    result = {"groupNames": ["a", "b"], "geneIds": np.array([10, 20, 30, 40], dtype=np.uint32),
              "zScore": np.array([[1., 3., 3., -2.], [0., 0., -1., 5.]])}
    assert topGenes(result, 2) == {"a": [20, 30], "b": [40, 10]}
    assert topGenes(result, 9)["b"] == [40, 10, 20, 30]
