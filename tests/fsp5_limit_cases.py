"""The inputs of tests/test_gpu_fsp5_limits.py, built here so that tests/test_fsp5_limit_cases_cpu.py can prove without a GPU that
every one of them is what the GPU test means it to be (family sizes per pass of the candidate union, list lengths at the
selection tiers' edges, slice counts, filter forms, bucket sizes at the overflow rule): a GPU run then cannot pass because an
input quietly missed its target.

Signature layout as everywhere: uint64 [cells, words], bit i of a cell in word i >> 6 at position 63 - (i & 63); slice s of
length q is bits [s q, (s + 1) q), first bit most significant (src/BitSet.hpp:111-119)."""
import numpy as np

import synth


# ---- bits and slices with numpy only (nothing of the kernels' word arithmetic) ----
def bits_of(sig, L):
    """uint8 [cells, L]: bit i of every cell."""
    sig = np.ascontiguousarray(sig, dtype=np.uint64)
    n, words = sig.shape
    return np.unpackbits(sig.astype(">u8").view(np.uint8).reshape(n, words * 8), axis=1)[:, :L]


def pack_bits(bits):
    """The inverse of bits_of: uint8 [cells, L] -> uint64 [cells, words], unused bits zero."""
    n, L = bits.shape
    words = (L - 1) // 64 + 1
    padded = np.zeros((n, words * 64), dtype=np.uint8)
    padded[:, :L] = bits
    return np.packbits(padded, axis=1, bitorder="big").reshape(n, words, 8).view(">u8").reshape(n, words).astype(np.uint64)


def slice_values(sig, L, q):
    """uint64 [cells, L // q]: the value of every slice of every cell."""
    bits = bits_of(sig, L)
    weights = np.uint64(1) << np.arange(q - 1, -1, -1, dtype=np.uint64)
    slices = L // q
    out = np.zeros((bits.shape[0], slices), dtype=np.uint64)
    for s in range(slices):
        out[:, s] = bits[:, s * q:(s + 1) * q].astype(np.uint64) @ weights
    return out


def bucket_sizes(values):
    """int64 [cells, slices]: the size of the bucket every (cell, slice) falls in."""
    out = np.zeros(values.shape, dtype=np.int64)
    for s in range(values.shape[1]):
        _, inverse, counts = np.unique(values[:, s], return_inverse=True, return_counts=True)
        out[:, s] = counts[inverse]
    return out


def mismatches(sig, a, b):
    """Mismatch counts of the cell pairs (a[i], b[i])."""
    return np.bitwise_count(sig[a] ^ sig[b]).sum(axis=1).astype(np.int64)


# ---- B1: a cell count that needs three passes of unionKernel's bitmap ----
UNION_L, UNION_Q, UNION_K = 64, 16, 8
UNION_THRESHOLDS = (-2.0, 0.2)
UNION_SLICE_A, UNION_SLICE_B, UNION_SLICE_C = 0, 3, 1
UNION_VALUE_A, UNION_VALUE_B, UNION_VALUE_C = 0xA5A5, 0x3C3C, 0x5A5B
# family (c) was meant to lie in pass 2 alone, which at n = 2 P + 4099 has 4099 ids: it takes what pass 2 has left and the rest
# of its 7000 from pass 1.  Its members beyond the 6144 a block holds in registers are the highest ids: all in pass 2.
UNION_FAMILY_B = (100, 3000, 100)
UNION_FAMILY_C = (5, 3000, 3995)


def union_passes_case(ids_per_pass, seed=20251):
    """n = 2 P + 4099 random 64-bit signatures, lshCount 64, q = 16 (4 slices), with three planted buckets:
    (a) slice 0 shared by {5, P-1, P, P+1, 2P-1, 2P, n-1}; (b) slice 3 shared by 100 / 3000 / 100 cells of pass 0 / 1 / 2;
    (c) slice 1 shared by 5 / 3000 / 3995 cells.  No other cell has a family's value in the family's slice."""
    P = int(ids_per_pass)
    n = 2 * P + 4099
    rng = np.random.default_rng(seed)
    sig = rng.integers(0, 1 << 64, size=(n, 1), dtype=np.uint64, endpoint=False)
    family_a = np.array([5, P - 1, P, P + 1, 2 * P - 1, 2 * P, n - 1], dtype=np.int64)
    free = np.ones(n, dtype=bool)
    free[family_a] = False
    bounds = ((0, P), (P, 2 * P), (2 * P, n))

    def draw(counts):
        parts = []
        for (lo, hi), count in zip(bounds, counts):
            ids = lo + np.nonzero(free[lo:hi])[0]
            chosen = np.sort(rng.choice(ids, size=count, replace=False))
            free[chosen] = False
            parts.append(chosen)
        return np.concatenate(parts)

    family_b = draw(UNION_FAMILY_B)
    family_c = draw(UNION_FAMILY_C)
    for slice_, value, family in ((UNION_SLICE_A, UNION_VALUE_A, family_a), (UNION_SLICE_B, UNION_VALUE_B, family_b),
                                  (UNION_SLICE_C, UNION_VALUE_C, family_c)):
        shift = np.uint64(48 - 16 * slice_)
        field = np.uint64(0xffff) << shift
        current = (sig[:, 0] & field) >> shift
        sig[current == np.uint64(value), 0] ^= np.uint64(1) << shift                 # nobody else in this bucket
        sig[family, 0] = (sig[family, 0] & ~field) | (np.uint64(value) << shift)
    edges = np.concatenate([np.arange(0, 16), np.arange(P - 24, P + 24), np.arange(2 * P - 24, 2 * P + 24), np.arange(n - 16, n)])
    some = []
    for family, counts in ((family_b, UNION_FAMILY_B), (family_c, UNION_FAMILY_C)):
        begin = 0
        for count in counts:
            some += [family[begin:begin + 3], family[begin + count - 3:begin + count]]
            begin += count
    cells = np.unique(np.concatenate([family_a, edges] + some)).astype(np.uint32)
    return dict(sig=sig, n=n, P=P, L=UNION_L, q=UNION_Q, k=UNION_K, family_a=family_a, family_b=family_b, family_c=family_c,
                cells=cells, rows=(P + 4321, 2 * P + 2000))


# ---- B2: signature widths by filter form ----
FILTER_N, FILTER_Q, FILTER_K = 600, 8, 10
FILTER_THRESHOLDS = (0.2, 0.0)
# width in bits -> (the filter the host chooses for a 16-byte aligned array, 16-byte units of a row, lanes per candidate)
FILTER_WIDTHS = {
    384: ("wide<1,0,false>", 3, 4),
    640: ("wide<1,8,false>", 5, 8),
    1152: ("wide<1,16,false>", 9, 16),
    1280: ("wide<1,16,false>", 10, 16),
    1920: ("wide<1,16,false>", 15, 16),
    1100: ("wide<1,16,false>", 9, 16),          # 18 words, the last one partly used
    2176: ("wide<2,16,false>", 17, 16),
    3072: ("wide<2,16,false>", 24, 16),
    3968: ("wide<2,16,false>", 31, 16),
    8192: ("cooperative", 64, 16),              # 128 words: the eight registers of the cooperative form all in use
    8256: ("lane", 0, 0),                       # 129 words: one lane per candidate
}
FILTER_UNALIGNED_WIDTHS = (1024, 1280, 3072)    # even word counts: cooperative only because the array is 8 mod 16


def filter_form(L, aligned=True):
    """The candidate filter runFsp5 chooses for lshCount L (csrc/em2_fsp5.hip), as capi names it."""
    words = (L - 1) // 64 + 1
    if words > 128:
        return "lane"
    if words % 2 or words > 64 or not aligned:
        return "cooperative"
    units = words // 2
    per_lane = 1 if words <= 32 else 2
    lanes = 1
    while lanes < 16 and lanes * per_lane < units:
        lanes *= 2
    if per_lane == 1:
        if units == 16:
            return "wide<4,4,true>"
        return "wide<1,16,false>" if lanes == 16 else "wide<1,8,false>" if lanes == 8 else "wide<1,0,false>"
    if units == 32:
        return "wide<2,16,true>"
    return "wide<2,16,false>" if lanes == 16 else "wide<2,0,false>"


def filter_case(L):
    return synth.clustered_signatures(FILTER_N, L, cluster_count=4, flip=0.1, seed=L)


# ---- B3: candidate lists of exactly the lengths at which another selection launch takes over ----
TIER_Q, TIER_THRESHOLD = 16, 0.2
TIER_PACKED_K = 7
TIER_PACKED_ENTRIES = (4096, 4097, 5120, 5121, 6144, 6145, 8192, 8193, 16384, 16385)
TIER_WHOLE_K = 2049
TIER_WHOLE_ENTRIES = (4096, 4097, 5120, 5121, 6656, 6657, 12288, 12289)
TIER_K_EDGES = (1024, 1025, 2048, 2049)
TIER_K_EDGE_ENTRIES = 4500
TIER_FLIPS = 12


def tier_case(entries, L, flips):
    """entries + 1 cells that all share slice 0 (bucketOverflow 0: every list has `entries` candidates).  flips = 0: identical
    cells, every comparison of the selection a tie; else up to `flips` flipped bits per cell outside slice 0."""
    m = entries + 1
    sig = np.tile(synth.random_signatures(1, L, seed=entries), (m, 1))
    if flips:
        rng = np.random.default_rng(entries)
        counts = rng.integers(0, flips + 1, size=m)
        bits = rng.integers(TIER_Q, L, size=(m, flips))
        for j in range(flips):
            rows = np.nonzero(j < counts)[0]
            bit = bits[rows, j]
            sig[rows, bit // 64] ^= np.uint64(1) << (63 - bit % 64).astype(np.uint64)
    return sig


def tier_rows(entries):
    return (0, 20), (entries + 1 - 20, entries + 1)


# ---- B4: slice counts around the lane = slice loops (64) and the union's descriptor count (256) ----
SLICES_N, SLICES_Q, SLICES_K, SLICES_THRESHOLD = 800, 4, 9, 0.2
SLICES_WIDTHS = {256: 64, 260: 65, 1020: 255, 1024: 256, 1028: 257}         # lshCount -> slices
SLICES_OVERFLOW_WIDTHS = (1020, 1024)


def slices_case(L):
    return synth.clustered_signatures(SLICES_N, L, cluster_count=5, flip=0.2, seed=L)


def slices_overflow(sig, L):
    """A bucketOverflow that drops some but not all of the buckets of most cells: the median bucket size over (cell, slice)."""
    return int(np.median(bucket_sizes(slice_values(sig, L, SLICES_Q))))


# ---- B5: slices of 30, 31 and 32 bits ----
WIDE_N, WIDE_L, WIDE_K = 300, 256, 300
WIDE_ORIGINALS = 100
WIDE_THRESHOLDS = (-2.0, 0.15)


def wide_slice_case(q, seed=5):
    """Cells 0 .. 99 are random; cell c >= 100 is random too, except that it copies the bits of one slice (slice (c + c // 100) mod
    sliceCount) from cell c mod 100 and has the complement of that cell's bit right before the slice (odd c; after it where the
    slice starts the signature) or right after it (even c; before it where the slice ends the signature).  A slice value with
    one bit too many or too few at either end separates the two."""
    L = WIDE_L
    slices = L // q
    bits = bits_of(synth.random_signatures(WIDE_N, L, seed=seed + q), L).copy()
    copied = []
    for c in range(WIDE_ORIGINALS, WIDE_N):
        partner = c % WIDE_ORIGINALS
        s = (c + c // WIDE_ORIGINALS) % slices
        begin, end = s * q, (s + 1) * q
        bits[c, begin:end] = bits[partner, begin:end]
        before = c % 2 == 1
        if begin == 0:
            before = False
        if end >= L:
            before = True
        outside = begin - 1 if before else end
        bits[c, outside] = 1 - bits[partner, outside]
        copied.append((c, partner, s, outside))
    return pack_bits(bits), copied


def wide_slice_model(sig, L, q, thr, similarity_table):
    """findSimilarPairs5 for k >= cells (keepBest never cuts) with numpy and Python integers: slice values from the unpacked
    bits, buckets by equality, the ascending union, mismatches by popcount, similarity from the reference's table (double,
    compared with the threshold as a double, stored as float), similarity descending then cell ascending.
    Returns the lists [(cell, float32 similarity), ...] per cell."""
    bits = bits_of(sig, L)
    n = len(sig)
    slices = L // q
    value = [[int("".join("01"[b] for b in bits[c, s * q:(s + 1) * q]), 2) for s in range(slices)] for c in range(n)]
    lists = []
    for c in range(n):
        union = sorted({o for s in range(slices) for o in range(n) if value[o][s] == value[c][s]})
        found = []
        for o in union:
            if o == c:
                continue
            m = int(np.bitwise_count(sig[c] ^ sig[o]).sum())
            if similarity_table[m] > thr:
                found.append((o, np.float32(similarity_table[m])))
        found.sort(key=lambda e: (-float(e[1]), e[0]))
        lists.append(found)
    return lists


def lists_to_arrays(lists, k):
    n = len(lists)
    cell = np.zeros((n, k), dtype=np.uint32)
    sim = np.zeros((n, k), dtype=np.float32)
    used = np.zeros(n, dtype=np.uint32)
    for c, found in enumerate(lists):
        used[c] = len(found)
        for i, (o, s) in enumerate(found):
            cell[c, i] = o
            sim[c, i] = s
    return cell, sim, used


# ---- B6: small edges ----
OVERFLOW_B, OVERFLOW_L, OVERFLOW_Q, OVERFLOW_N = 37, 64, 16, 300
OVERFLOW_GROUP_AT = (10, 100)         # b identical cells from 10 on, b + 1 identical cells from 100 on


def overflow_groups_case(seed=41):
    sig = synth.random_signatures(OVERFLOW_N, OVERFLOW_L, seed=seed)
    first, second = OVERFLOW_GROUP_AT
    sig[first:first + OVERFLOW_B] = sig[first]
    sig[second:second + OVERFLOW_B + 1] = sig[second]
    return sig


EDGE_N, EDGE_L, EDGE_Q = 500, 256, 8


def edge_case():
    """Clustered cells with the first 30 cells made identical (similarity exactly 1 among them)."""
    sig = synth.clustered_signatures(EDGE_N, EDGE_L, cluster_count=4, flip=0.1, seed=606)
    sig[:30] = sig[0]
    return sig


BATCH_N, BATCH_L, BATCH_Q, BATCH_K, BATCH_THRESHOLD = 6000, 256, 8, 12, 0.1
BATCH_ROWS = (1234, 5432)
BATCH_LOG2 = 20


def batch_case():
    return synth.clustered_signatures(BATCH_N, BATCH_L, cluster_count=7, flip=0.2, seed=6003)


def plan_batches(gathered, begin, end, budget_log2):
    """The batches runFsp5 cuts [begin, end) into (csrc/em2_fsp5.hip): consecutive cells while the bucket members they gather
    fit the budget, at most 2^20 cells.  Returns the [begin, end) of every batch."""
    budget = 1 << budget_log2
    out = []
    at = begin
    while at < end:
        total = 0
        stop = at
        while stop < end and stop - at < (1 << 20):
            g = int(gathered[stop])
            if total + g > budget and stop > at:
                break
            total += g
            stop += 1
            if total > budget:
                break
        out.append((at, stop))
        at = stop
    return out
