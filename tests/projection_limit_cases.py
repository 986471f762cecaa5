"""Inputs that put the signature projection (csrc/em2_project.hip) where a sign is nearly undecidable, the reference
value they are judged by, and a CPU model of the screening tiers that CHOOSES and CERTIFIES them -- the GPU result is never
compared with the model, only with the reference (and the oracle).  No GPU here; everything deterministic from fixed seeds.

reference_values    Lsh::computeCellLshSignatures (src/Lsh.cpp:118-224) and the per-cell sum it reads
                    (src/ExpressionMatrixSubset.cpp:46-58) in numpy float64: every product rounded, then added, in stored order;
                    the mean from the sequential double += float sum.  Returns the words and the values sp[c, i].
                    tests/test_signatures_independent_numpy.py holds the oracle to it.
model               what the tiers compute and the bounds they hold it against, written from the comments and formulas of
                    em2_project.hip: T1 = scale * sum x * q - mean * S on the 16-bit copy, T2 = sum x * float(U) - mean * S on the
                    float copy, and expected_listed(): how many list entries each tier must and may leave.
(a) quantisation_case   every rounding error of the 16-bit copy points the same way: T1 has the wrong sign at up to 0.99 of its bound
(b) float_copy_case     the same for the float copy: T2 has the wrong sign at up to 0.97 of its bound
(c) flip_case           one hyperplane entry per bit bisected to the reference's own sign flip and set -3..4 ulps from it: the
                        exact tier must round every product and add in stored order, the mean must be the sequential sum
(d) entry_count_case    cells of 0..260 entries: every part, chunk and prefetch boundary of the kernels' entry loops"""
from fractions import Fraction

import numpy as np

TWO24 = 2.0 ** -24          # 5.9604644775390625e-08 in the kernels
TWO52 = 2.0 ** -52          # 2.220446049250313e-16


# ---------------------------------------------------------------------------------------------------------------------------------
# the reference
# ---------------------------------------------------------------------------------------------------------------------------------

def pack(bits):
    """(cells, lshCount) booleans -> (cells, words) uint64, bit i at position 63 - (i & 63) of word i >> 6 (src/BitSet.hpp:48-62)."""
    cells, L = bits.shape
    words = (L - 1) // 64 + 1                                               # Lsh.cpp:127
    padded = np.zeros((cells, words * 64), dtype=np.uint8)
    padded[:, :L] = bits
    return np.ascontiguousarray(np.packbits(padded, axis=1)).view(">u8").astype(np.uint64).reshape(cells, words)


def vector_sums(vectors, gene_count, lsh_count):
    sums = np.zeros(lsh_count, dtype=np.float64)
    for g in range(gene_count):                                             # Lsh.cpp:137-144, ascending gene id
        sums = sums + vectors[g]
    return sums


def cell_mean(counts, gene_count):
    sum1 = np.float64(0.0)
    for x in counts:                                                        # computeSums: double += float, stored order
        sum1 = sum1 + np.float64(x)
    return sum1 / np.float64(gene_count)                                    # Lsh.cpp:167-168


def reference_values(toc, genes, counts, gene_count, vectors, lsh_count):
    """(signature words, sp): sp[c, i] is the reference's scalar product of cell c with hyperplane i, bit i is sp > 0."""
    cells = len(toc) - 1
    sums = vector_sums(vectors, gene_count, lsh_count)
    values = np.zeros((cells, lsh_count), dtype=np.float64)
    for c in range(cells):
        lo, hi = int(toc[c]), int(toc[c + 1])
        mean = cell_mean(counts[lo:hi], gene_count)
        sp = -mean * sums                                                   # :180-182
        for g, x in zip(genes[lo:hi], counts[lo:hi]):                       # :188-198, stored (ascending local gene id) order
            sp = sp + np.float64(x) * vectors[int(g)]
        values[c] = sp
    return pack(values > 0.0), values                                       # :201-206


def compute_signatures(toc, genes, counts, gene_count, vectors, lsh_count):
    return reference_values(toc, genes, counts, gene_count, vectors, lsh_count)[0]


def reference(case):
    return reference_values(case["toc"], case["genes"], case["counts"], case["gene_count"], case["vectors"], case["L"])


# ---------------------------------------------------------------------------------------------------------------------------------
# the model of the tiers
# ---------------------------------------------------------------------------------------------------------------------------------

def integer_form_cells(toc, counts):
    """Per cell: every count an integer of at most 15 bits and sum|count| <= 65535 (cellStatsKernel; include/em2_lsh.h,
    EM2_TIER_FIXED16_INTEGER).  A cell without counts qualifies."""
    out = np.zeros(len(toc) - 1, dtype=bool)
    for c in range(len(toc) - 1):
        x = counts[int(toc[c]):int(toc[c + 1])].astype(np.float64)
        out[c] = bool(np.all(x == np.trunc(x)) and np.all(np.abs(x) <= 32767.0) and np.abs(x).sum() <= 65535.0)
    return out


def first_tier(case, aux=True):
    L = case["L"]
    if not aux or L % 4:
        return "exact"
    if L % 64:
        return "float"
    return "fixed16-integer" if integer_form_cells(case["toc"], case["counts"]).all() else "fixed16-float"


def model(case):
    """The tiers' values and bounds for every (cell, bit).  T1/bound1: the 16-bit tier in the form the matrix takes (None where the
    width has no such tier); T2: the float copy's value; bound2(k): its bound with (n + k) 2^-52, k = 2 (the word form behind the
    16-bit tier and the one-block-per-1024-bits first tier), 8 (the sliced first tier), 10 (the per-bit form)."""
    toc, genes, counts, G, U, L = (case[k] for k in ("toc", "genes", "counts", "gene_count", "vectors", "L"))
    cells = len(toc) - 1
    S = vector_sums(U, G, L)
    maxabs = np.abs(U).max(axis=0)
    U32 = U.astype(np.float32).astype(np.float64)
    quantized = L % 64 == 0
    integer = bool(integer_form_cells(toc, counts).all())
    if quantized:
        scale = maxabs / 32767.0
        safe = np.where(scale > 0.0, scale, 1.0)
        q = np.where(scale > 0.0, np.clip(np.rint(U / safe), -32767.0, 32767.0), 0.0)
    n = np.zeros(cells)
    mean = np.zeros(cells)
    absx = np.zeros(cells)
    sum_q = np.zeros((cells, L))
    sum_f = np.zeros((cells, L))
    for c in range(cells):
        lo, hi = int(toc[c]), int(toc[c + 1])
        x = counts[lo:hi].astype(np.float64)
        n[c] = hi - lo
        mean[c] = cell_mean(counts[lo:hi], G)
        absx[c] = np.abs(x).sum() * (1.0 + 1e-12)
        if hi > lo:
            g = genes[lo:hi].astype(np.int64)
            sum_f[c] = x @ U32[g]
            if quantized:
                sum_q[c] = x @ q[g]
    terms = np.abs(mean)[:, None] * np.abs(S)[None, :] + absx[:, None] * maxabs[None, :]
    minus_mean_s = (-mean)[:, None] * S[None, :]
    out = {"n": n, "mean": mean, "absx": absx, "S": S, "maxabs": maxabs, "integer": integer, "T1": None, "bound1": None}
    if quantized:
        out["T1"] = sum_q * scale[None, :] + minus_mean_s
        bound1 = ((n + 12.0) * TWO52 * 1.000001)[:, None] * terms + 0.501 * scale[None, :] * absx[:, None] + 1e-300
        if not integer:
            bound1 = bound1 + 9.6e-7 * absx[:, None] * maxabs[None, :] + (n * 1.5e-45)[:, None] * scale[None, :]
        out["bound1"] = bound1
        out["scale"] = scale
    out["T2"] = sum_f + minus_mean_s

    def bound2(k):
        factor = (1.01 * TWO24 + (n + k) * TWO52) * 1.000001
        return factor[:, None] * terms + (absx * 1.5e-45)[:, None] + 1e-300
    out["bound2"] = bound2
    return out


def expected_listed(case, mdl=None):
    """What em2_dev_compute_signatures_listed must report at the least and may report at the most: {"words", "bits", "exact"} ->
    (certain, possible), a bit counting as certainly undecided at |T| < 0.999 bound and as possibly undecided at |T| < 1.001 bound,
    aggregated the way the kernels list: the 16-bit tier a word with one undecided bit by that bit and any other by the word; the
    word form of the float tier a word with any undecided bit, its per-bit form the word of an undecided listed bit; the sliced
    float first tier (lshCount a multiple of 32) once per 32-bit slice, the other once per word."""
    L = case["L"]
    mdl = mdl or model(case)
    cells = len(case["toc"]) - 1
    zero = (0, 0)

    def undecided(T, bound):
        return np.abs(T) < 0.999 * bound, np.abs(T) < 1.001 * bound

    def grouped(mask, width):
        padded = np.zeros((cells, (L + width - 1) // width * width), dtype=bool)
        padded[:, :L] = mask
        return padded.reshape(cells, -1, width)

    if L % 4:
        return {"words": zero, "bits": zero, "exact": zero}
    if L % 64:
        width, k = (32, 8.0) if L % 32 == 0 else (64, 2.0)
        sure, maybe = undecided(mdl["T2"], mdl["bound2"](k))
        return {"words": zero, "bits": zero,
                "exact": (int(grouped(sure, width).any(axis=2).sum()), int(grouped(maybe, width).any(axis=2).sum()))}
    sure1, maybe1 = undecided(mdl["T1"], mdl["bound1"])
    c1, p1 = grouped(sure1, 64).sum(axis=2), grouped(maybe1, 64).sum(axis=2)
    word_sure, word_maybe = c1 >= 2, p1 >= 2
    bit_sure, bit_maybe = (c1 == 1) & (p1 == 1), (p1 >= 1) & (c1 <= 1)
    sure_w, maybe_w = undecided(mdl["T2"], mdl["bound2"](2.0))
    sure_b, maybe_b = undecided(mdl["T2"], mdl["bound2"](10.0))
    exact_sure = (word_sure & grouped(sure_w, 64).any(axis=2)) | (bit_sure & grouped(sure_b & sure1, 64).any(axis=2))
    exact_maybe = (word_maybe & grouped(maybe_w, 64).any(axis=2)) | (bit_maybe & grouped(maybe_b & maybe1, 64).any(axis=2))
    return {"words": (int(word_sure.sum()), int(word_maybe.sum())), "bits": (int(bit_sure.sum()), int(bit_maybe.sum())),
            "exact": (int(exact_sure.sum()), int(exact_maybe.sum()))}


def trap_statistics(T, bound, sp, among=None):
    """Of one tier on one case: decided_wrong -- bits it would decide (|T| > bound) against the reference's sign (must be 0);
    traps -- bits whose T has the wrong sign at more than 0.9 of the bound; depth -- the largest |T| / bound among those;
    outside -- bits just outside the bound (up to 1.1 of it), right-signed.  among: the bits to look at (all)."""
    among = np.ones(T.shape, dtype=bool) if among is None else among
    wrong = ((T > 0.0) != (sp > 0.0)) & among
    ratio = np.abs(T) / bound
    traps = wrong & (ratio > 0.9)
    return {"decided_wrong": int((wrong & (ratio > 1.0)).sum()), "traps": int(traps.sum()),
            "depth": float(ratio[traps].max()) if traps.any() else 0.0,
            "outside": int((~wrong & among & (ratio > 1.0) & (ratio < 1.1)).sum()), "trap_mask": traps}


# ---------------------------------------------------------------------------------------------------------------------------------
# helpers of the generators
# ---------------------------------------------------------------------------------------------------------------------------------

def _csr(cell_genes, cell_counts):
    toc = np.zeros(len(cell_genes) + 1, dtype=np.uint64)
    toc[1:] = np.cumsum([len(g) for g in cell_genes])
    genes = np.concatenate([np.asarray(g, dtype=np.uint32) for g in cell_genes] + [np.zeros(0, dtype=np.uint32)])
    counts = np.concatenate([np.asarray(x, dtype=np.float32) for x in cell_counts] + [np.zeros(0, dtype=np.float32)])
    return toc, genes.astype(np.uint32), counts.astype(np.float32)


def _sweep(cells, L, direction, low, high, deep, uniform_share=3.0 / 8.0):
    """t[c, i], the target in units of the bound's main term.  Odd cells: a share of the columns sweep [-1.5, 1.5] uniformly (both signs
    against both directions of the rounding errors), the others lie in [low, high] on the side the direction makes a trap.  Even
    cells: every column in [deep, high] on that side -- a tier whose bound were a tenth too small would find NO undecided bit in
    such a cell's words and hand nothing to the tier behind it, which otherwise recomputes the whole word and hides the mistake."""
    period = 64
    uniform = int(round(period * uniform_share))
    pattern = np.concatenate([np.linspace(-1.5, 1.5, uniform), np.linspace(low, high, period - uniform)])
    focused = np.concatenate([np.zeros(uniform, dtype=bool), np.ones(period - uniform, dtype=bool)])
    index = (np.arange(L)[None, :] * 29 + np.arange(cells)[:, None] * 7) % period          # (29: coprime to 64)
    swept = np.where(focused[index], pattern[index] * direction, pattern[index])
    return np.where(np.arange(cells)[:, None] % 2 == 0, np.linspace(deep, high, period)[index] * direction, swept)


# ---------------------------------------------------------------------------------------------------------------------------------
# (a) quantisation traps
# ---------------------------------------------------------------------------------------------------------------------------------

QUANTISATION_VARIANTS = ("integer", "half", "unbalanced")


def quantisation_case(variant, cells=48, L=64, per_cell=12, seed=101):
    """Disjoint gene sets per cell.  For cell c and column i integers k_j with sum x_j k_j = N are chosen and the hyperplane entries
    are scale_i (k_j - 0.499 d): they quantise to k_j, every rounding error points the way d says, so T1 = N scale_i while the
    reference is about (N - 0.499 d X) scale_i.  One gene outside every cell holds the column maximum (it fixes scale_i), four more
    bring S_i to its target: about 0, or, "unbalanced", to where |mean| |S_i| is about the quantisation term.  "half": the same counts
    times 0.5 -- the float form, with every product count * q and every chunk sum still exact."""
    assert variant in QUANTISATION_VARIANTS and L % 64 == 0
    rng = np.random.default_rng(seed)
    m = per_cell
    G = cells * m + 5
    factor = 0.5 if variant == "half" else 1.0
    whole = rng.integers(1, 25, size=(cells, m))
    whole[:, 0] = 1                                                          # any integer target is reachable
    x = whole * factor
    X = x.sum(axis=1)
    maximum = rng.uniform(1.0, 2.0, size=L) * 2.0 ** rng.integers(-3, 4, size=L)
    scale = maximum / 32767.0                                                # as vectorsToQuantizedKernel computes it
    direction = np.where((np.arange(cells)[:, None] + np.arange(L)[None, :]) % 2 == 0, 1.0, -1.0)
    target_s = np.zeros(L)
    if variant == "unbalanced":
        target_s = np.where(np.arange(L) % 3 == 0, -1.0, 1.0) * rng.uniform(0.6, 1.4, size=L) * 0.5 * G * scale
    mean = X / G
    # the bound's main terms in units of scale_i: the quantisation term and, in the float form, the single-precision chunks' term
    main = (0.501 + (0.0 if variant != "half" else 9.6e-7 * 32767.0)) * X
    t = _sweep(cells, L, direction, 0.9, 1.15, 0.91)
    # T1 = factor * N * scale_i - mean * S_i  =  t * main * scale_i
    N = np.rint((t * main[:, None] + mean[:, None] * (target_s / scale)[None, :]) / factor)
    k = rng.integers(-20, 21, size=(cells, m, L)).astype(np.float64)
    k[:, 0, :] = N - np.einsum("cj,cjl->cl", whole[:, 1:].astype(np.float64), k[:, 1:, :])
    assert np.abs(k).max() < 30000
    vectors = np.zeros((G, L))
    vectors[:cells * m] = (scale[None, None, :] * (k - 0.499 * direction[:, None, :])).reshape(cells * m, L)
    vectors[cells * m] = maximum
    rest = (target_s - maximum - np.array([float(sum(Fraction(v) for v in vectors[:cells * m, i])) for i in range(L)])) / 4.0
    assert np.all(np.abs(rest) < maximum)
    vectors[cells * m + 1:] = rest[None, :]
    cell_genes = [np.arange(c * m, (c + 1) * m) for c in range(cells)]
    toc, genes, counts = _csr(cell_genes, list(x))
    return {"name": "quantisation-" + variant, "toc": toc, "genes": genes, "counts": counts, "gene_count": G, "vectors": vectors, "L": L,
            "engineered": np.ones((cells, L), dtype=bool)}


# ---------------------------------------------------------------------------------------------------------------------------------
# (b) float-copy traps
# ---------------------------------------------------------------------------------------------------------------------------------

FLOAT_COPY_LAYOUTS = (("all", 64), ("all", 1024), ("one-per-word", 1024), ("all", 96), ("all", 100))
ONE_PER_WORD_POSITIONS = (0, 7, 8, 56, 63)


def float_copy_case(layout, L, cells=48, pairs=6, seed=202):
    """Disjoint gene sets per cell, counts in pairs whose entries have opposite signs.  A trap entry is U = f (1 -+ 0.98 * 2^-24) with
    f = +-M0 (1 + m 2^-23) a float just above the power of two M0, so float(U) == f, the float copy's value is
    sum x f = tau 2^-23 M0 EXACTLY (the integers m are chosen for it) and every rounding error of the copy points the way d says: the
    reference is about (2 tau - 0.98 d X) 2^-24 M0.  One gene outside every cell brings S_i to about 0.
    "all": every column a trap.  "one-per-word": one trap column per 64-bit word, at in-word positions 0, 7, 8, 56, 63 in turn, the
    other 63 columns random hyperplanes redrawn until the 16-bit tier's model decides them with a margin of two."""
    assert layout in ("all", "one-per-word")
    rng = np.random.default_rng(seed + L)
    m = 2 + 2 * pairs
    G = cells * m + 1
    whole = np.ones((cells, m), dtype=np.int64)
    pair_counts = rng.integers(1, 25, size=(cells, pairs))
    whole[:, 2::2] = pair_counts
    whole[:, 3::2] = pair_counts
    sign = np.where(np.arange(m) % 2 == 0, 1.0, -1.0)                        # j = 0: count 1, +;  j = 1: count 1, -;  then the pairs
    X = whole.sum(axis=1).astype(np.float64)
    if layout == "all":
        trap_columns = np.arange(L)
    else:
        trap_columns = np.array([64 * w + ONE_PER_WORD_POSITIONS[w % len(ONE_PER_WORD_POSITIONS)] for w in range(L // 64)])
    T = len(trap_columns)
    M0 = 2.0 ** rng.integers(-3, 4, size=T)
    direction = np.where((np.arange(cells)[:, None] + np.arange(T)[None, :]) % 2 == 0, 1.0, -1.0)
    if layout == "all":
        t = _sweep(cells, T, direction, 0.9, 1.15, 0.945)
    else:
        t = _sweep(cells, T, direction, 0.93, 1.12, 0.93, uniform_share=1.0 / 8.0)
    tau = np.rint(t * 0.49 * X[:, None])
    mm = rng.integers(1, max(3, 1200 // pairs) + 1, size=(cells, m, T)).astype(np.float64)             # (m >= 1: below M0 itself the floats lie twice as dense)
    while True:
        rest = tau - np.einsum("cj,cjt->ct", whole[:, 2:] * sign[None, 2:], mm[:, 2:, :])
        large = np.abs(rest) > 15000.0                                           # (rare: smaller integers for that cell and column)
        if not large.any():
            break
        mm[:, 2:, :] = np.where(large[:, None, :], np.ceil(mm[:, 2:, :] / 2.0), mm[:, 2:, :])
    mm[:, 0, :] = np.maximum(rest, 0.0) + 1.0
    mm[:, 1, :] = np.maximum(-rest, 0.0) + 1.0
    assert mm.max() < 20000                                                  # f / M0 < 1.0024: 0.98 * 2^-24 f stays below half an ulp of f
    f = sign[None, :, None] * M0[None, None, :] * (1.0 + mm * 2.0 ** -23)
    entries = f * (1.0 - direction[:, None, :] * sign[None, :, None] * 0.98 * TWO24)
    assert np.array_equal(entries.astype(np.float32).astype(np.float64), f)
    vectors = np.zeros((G, L))
    if layout == "one-per-word":
        vectors[:] = rng.standard_normal((G, L))
    vectors[:cells * m, trap_columns] = entries.reshape(cells * m, T)
    vectors[cells * m, trap_columns] = [-float(sum(Fraction(v) for v in vectors[:cells * m, i])) for i in trap_columns]
    cell_genes = [np.arange(c * m, (c + 1) * m) for c in range(cells)]
    toc, genes, counts = _csr(cell_genes, list(whole.astype(np.float32)))
    engineered = np.zeros((cells, L), dtype=bool)
    engineered[:, trap_columns] = True
    case = {"name": "float-copy-%s-%d" % (layout, L), "toc": toc, "genes": genes, "counts": counts, "gene_count": G, "vectors": vectors,
            "L": L, "engineered": engineered, "trap_columns": trap_columns}
    if layout == "one-per-word":
        for _ in range(100):
            mdl = model(case)
            bad = (np.abs(mdl["T1"]) <= 2.5 * mdl["bound1"]) & ~engineered
            if not bad.any():
                break
            for c, i in np.argwhere(bad):
                vectors[c * m:(c + 1) * m, i] = rng.standard_normal(m)
        else:
            raise AssertionError("the random columns did not settle")
    return case


# ---------------------------------------------------------------------------------------------------------------------------------
# (c) flip points
# ---------------------------------------------------------------------------------------------------------------------------------

FLIP_WIDTHS = (1024, 96, 100, 63)
FLIP_CELLS = 16
FLIP_LARGE_TINY_CELLS = 6          # the cells 10..15: two counts near 2^29 and 3 * 2^28 and FLIP_TINY counts near 2^-24
FLIP_TINY = 48
FLIP_GENES = 80


def _ordered(values):
    """doubles -> integers in the order of the doubles (adjacent doubles are adjacent integers; -0.0 and 0.0 coincide)."""
    bits = np.asarray(values, dtype=np.float64).view(np.int64)
    return np.where(bits >= 0, bits, np.int64(-2 ** 63) - bits)


def _doubles(keys):
    keys = np.asarray(keys, dtype=np.int64)
    return np.where(keys >= 0, keys, np.int64(-2 ** 63) - keys).view(np.float64)


def flip_cell_values(case, c, columns, private_values):
    """The reference's sp of cell c at the given columns with U[private gene of c][columns] replaced by private_values -- S_i is
    recomputed, as it holds that entry too."""
    toc, genes, counts, G, U = (case[k] for k in ("toc", "genes", "counts", "gene_count", "vectors"))
    block = U[:, columns].copy()
    block[c] = private_values                                               # the private gene of cell c is gene c
    sums = np.zeros(len(columns))
    for g in range(G):
        sums = sums + block[g]
    lo, hi = int(toc[c]), int(toc[c + 1])
    sp = -cell_mean(counts[lo:hi], G) * sums
    for g, x in zip(genes[lo:hi], counts[lo:hi]):
        sp = sp + np.float64(x) * block[int(g)]
    return sp


def flip_case(L, seed=303):
    """Cell c owns gene c (its first entry, an ordinary fractional count) and the columns i % 16 == c.  U[c][i] of an owned column is
    bisected over the doubles to the pair of neighbours between which the reference's bit flips, and set k ulps from it, k = -3..4
    in turn.  Cells 0..9: 36 to 63 fractional counts.  Cells 10..15: the private count, two counts near 2^29 and 3 * 2^28 and 48 counts near 2^-24 --
    the sequential sum of the counts loses every tiny one, any other order keeps some."""
    rng = np.random.default_rng(seed + L)
    C, G = FLIP_CELLS, FLIP_GENES
    cell_genes, cell_counts = [], []
    for c in range(C):
        if c < C - FLIP_LARGE_TINY_CELLS:
            n = 36 + 3 * c
            x = (rng.integers(1, 40, size=n) * np.float32(0.37) + np.float32(0.123)).astype(np.float32)
        else:
            n = 3 + FLIP_TINY
            x = np.empty(n, dtype=np.float32)
            x[0] = np.float32(rng.integers(1, 40)) * np.float32(0.37) + np.float32(0.123)
            # (about 2^29 and 3 * 2^28, with full mantissas so that their products round like any other)
            x[1], x[2] = np.float32(2.0 ** 29 * rng.uniform(1.0, 1.3)), np.float32(3.0 * 2.0 ** 28 * rng.uniform(1.0, 1.3))
            x[3:] = (2.0 ** -24 * (1.0 + 0.2 * rng.uniform(size=FLIP_TINY))).astype(np.float32)
        others = np.sort(rng.choice(np.arange(C, G), size=n - 1, replace=False))
        cell_genes.append(np.concatenate([[c], others]))
        cell_counts.append(x)
    toc, genes, counts = _csr(cell_genes, cell_counts)
    vectors = rng.standard_normal((G, L)) + 0.3                            # S_i is not balanced
    case = {"name": "flip-%d" % L, "toc": toc, "genes": genes, "counts": counts, "gene_count": G, "vectors": vectors, "L": L,
            "engineered": np.zeros((C, L), dtype=bool), "large_tiny_cells": np.arange(C - FLIP_LARGE_TINY_CELLS, C)}
    offsets = np.zeros(L, dtype=np.int64)
    for c in range(C):
        columns = np.arange(c, L, C)
        if not len(columns):
            continue
        case["engineered"][c, columns] = True
        # sp is very nearly linear in the entry: the root from two evaluations, then a bracket around it
        u0 = vectors[c, columns].copy()
        s0, s1 = flip_cell_values(case, c, columns, u0), flip_cell_values(case, c, columns, u0 + 1.0)
        root = u0 - s0 / (s1 - s0)
        width = 1e-9 * (np.abs(root) + 1.0)
        for _ in range(20):
            a, b = root - width, root + width
            up = flip_cell_values(case, c, columns, b) > 0.0
            down = flip_cell_values(case, c, columns, a) > 0.0
            if np.all(up != down):
                break
            width = np.where(up != down, width, width * 10.0)
        else:
            raise AssertionError("no bracket")
        # lo: bit clear, hi: bit set
        lo, hi = _ordered(np.where(up, a, b)), _ordered(np.where(up, b, a))
        while np.any(np.abs(hi - lo) > 1):
            mid = lo + (hi - lo) // 2
            positive = flip_cell_values(case, c, columns, _doubles(mid)) > 0.0
            moving = np.abs(hi - lo) > 1
            hi = np.where(moving & positive, mid, hi)
            lo = np.where(moving & ~positive, mid, lo)
        k = (np.arange(len(columns)) + c) % 8 - 3                           # -3..4 ulps from the clear side of the flip
        step = np.where(hi > lo, 1, -1)
        vectors[c, columns] = _doubles(lo + k * step)
        offsets[columns] = k
    case["ulps"] = offsets
    return case


def flip_distance(case):
    """For every engineered bit: the smallest |d| <= 4 such that the reference's bit at d ulps of the entry differs from its bit at
    d - 1 or d + 1 ulps (towards 0) -- that is, how far the nearest sign flip is; 99 where there is none within 4 ulps."""
    C, L = case["engineered"].shape
    out = np.full((C, L), 99, dtype=np.int64)
    for c in range(C):
        columns = np.nonzero(case["engineered"][c])[0]
        if not len(columns):
            continue
        keys = _ordered(case["vectors"][c, columns])
        bits = np.array([flip_cell_values(case, c, columns, _doubles(keys + d)) > 0.0 for d in range(-4, 5)])
        for d in (4, 3, 2, 1):
            out[c, columns] = np.where(bits[4 + d] != bits[4 + d - 1], d, out[c, columns])
            out[c, columns] = np.where(bits[4 - d] != bits[4 - d + 1], d, out[c, columns])
    return out


def _round(value):
    return Fraction(float(value))                                           # (float(Fraction) rounds to nearest even)


def fused_bits(case):
    """The engineered bits under a variant of the reference that fuses every multiply-add (one rounding per entry), exactly."""
    toc, genes, counts, G, U, L = (case[k] for k in ("toc", "genes", "counts", "gene_count", "vectors", "L"))
    sums = vector_sums(U, G, L)
    out = np.zeros(case["engineered"].shape, dtype=bool)
    for c, i in np.argwhere(case["engineered"]):
        lo, hi = int(toc[c]), int(toc[c + 1])
        sp = Fraction(float(-cell_mean(counts[lo:hi], G) * sums[i]))
        for g, x in zip(genes[lo:hi], counts[lo:hi]):
            sp = _round(Fraction(float(x)) * Fraction(float(U[int(g), i])) + sp)
        out[c, i] = sp > 0
    return out


def reordered_mean_bits(case):
    """The bits under a variant that sums a cell's counts in another order (np.sum of the reversed counts), all else the reference's."""
    toc, genes, counts, G, U, L = (case[k] for k in ("toc", "genes", "counts", "gene_count", "vectors", "L"))
    sums = vector_sums(U, G, L)
    out = np.zeros(case["engineered"].shape, dtype=bool)
    for c in range(len(toc) - 1):
        lo, hi = int(toc[c]), int(toc[c + 1])
        mean = np.sum(counts[lo:hi][::-1].astype(np.float64)) / np.float64(G)
        sp = -mean * sums
        for g, x in zip(genes[lo:hi], counts[lo:hi]):
            sp = sp + np.float64(x) * U[int(g)]
        out[c] = sp > 0.0
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# (d) entry-count edges
# ---------------------------------------------------------------------------------------------------------------------------------

ENTRY_COUNT_VARIANTS = ("integer", "mantissa24")
ENTRY_COUNT_FLAT_COLUMNS = (5, 64 + 3, 64 + 40, 64 + 63)          # one in word 0, three in word 1


def entry_count_case(variant, seed=404):
    """Cell c has exactly c entries, c = 0..260, of 300 genes, 128 bits.  Random hyperplanes times 1 + 1e-6 noise, except one column
    of word 0 and three of word 1, which are a (1 + 2e-5 noise): there the 16-bit copy sees next to no difference between the genes and
    the float copy most of it -- nearly every cell sends word 0 to the per-bit form of the float tier and word 1 to its word form, and
    the cells with many entries go on to the exact tier.  "mantissa24": counts (1 + odd * 2^-23) * 2^e, no integers."""
    assert variant in ENTRY_COUNT_VARIANTS
    rng = np.random.default_rng(seed)
    cells, G, L = 261, 300, 128
    cell_genes = [np.sort(rng.choice(G, size=c, replace=False)) for c in range(cells)]
    if variant == "integer":
        cell_counts = [rng.integers(1, 60, size=c).astype(np.float32) for c in range(cells)]
    else:
        cell_counts = [((1.0 + (2 * rng.integers(0, 2 ** 22, size=c) + 1) * 2.0 ** -23) * 2.0 ** rng.integers(-2, 5, size=c)).astype(np.float32)
                       for c in range(cells)]
    vectors = rng.standard_normal((G, L)) * (1.0 + 1e-6 * (rng.uniform(size=(G, L)) - 0.5))
    for i in ENTRY_COUNT_FLAT_COLUMNS:
        vectors[:, i] = rng.uniform(0.5, 2.0) * (1.0 + 2e-5 * (rng.uniform(size=G) - 0.5))
    toc, genes, counts = _csr(cell_genes, cell_counts)
    return {"name": "entry-counts-" + variant, "toc": toc, "genes": genes, "counts": counts, "gene_count": G, "vectors": vectors, "L": L,
            "engineered": np.zeros((cells, L), dtype=bool)}


# ---------------------------------------------------------------------------------------------------------------------------------
# random draws (tools/fuzz_parity.py)
# ---------------------------------------------------------------------------------------------------------------------------------

def draw(rng):
    """A random case of (a), (b) or (c) as a small dict; build(draw) makes the case."""
    kind = str(rng.choice(["quantisation", "float-copy", "flip"]))
    seed = int(rng.integers(1 << 30))
    if kind == "quantisation":
        return {"kind": kind, "variant": str(rng.choice(QUANTISATION_VARIANTS)), "cells": int(rng.integers(1, 97)),
                "L": int(rng.choice([64, 128, 192, 1024])), "per_cell": int(rng.integers(4, 40)), "seed": seed}
    if kind == "float-copy":
        layout = str(rng.choice(["all", "all", "one-per-word"]))
        L = int(rng.choice([64, 128, 512, 1024])) if layout == "one-per-word" else int(rng.choice([4, 36, 64, 96, 100, 128, 160, 1000, 1024]))
        return {"kind": kind, "layout": layout, "L": L, "cells": int(rng.integers(1, 97)), "pairs": int(rng.integers(1, 13)), "seed": seed}
    return {"kind": kind, "L": int(rng.choice([1, 33, 63, 64, 96, 100, 128, 1000, 1024])), "seed": seed}


def build(draw):
    if draw["kind"] == "quantisation":
        return quantisation_case(draw["variant"], draw["cells"], draw["L"], draw["per_cell"], draw["seed"])
    if draw["kind"] == "float-copy":
        return float_copy_case(draw["layout"], draw["L"], draw["cells"], draw["pairs"], draw["seed"])
    return flip_case(draw["L"], draw["seed"])
