"""A second, independent restatement of findSimilarPairs6 (src/ExpressionMatrixLsh.cpp:842-1145, the Charikar permutation
search) in plain Python, sharing no code with tests/native/em2_fsp6_restatement.cpp.  Only the bit permutations come from
the C++ restatement: they are std::shuffle's output, and which draws libstdc++'s shuffle makes is the contract, not something
to restate.  The priority queue is an explicit emulation of libstdc++'s std::push_heap / std::pop_heap (bits/stl_heap.h:
__push_heap, __adjust_heap) with the pointer's operator< on prefixLength alone (src/charikar.hpp), so the order in which
pointers with equal prefixes pop -- which decides the cells visited -- is checked on tie-heavy inputs: 1-bit prefixes,
identical cells, two-word prefixes."""
import math

import numpy as np
import pytest

import fsp6_binding
import synth


@pytest.fixture(scope="module")
def restatement():
    return fsp6_binding.load()


def push_heap(heap, value):
    """std::priority_queue::push: push_back + std::push_heap (__push_heap with topIndex 0)."""
    heap.append(value)
    hole = len(heap) - 1
    parent = (hole - 1) // 2
    while hole > 0 and heap[parent][0] < value[0]:
        heap[hole] = heap[parent]
        hole = parent
        parent = (hole - 1) // 2
    heap[hole] = value


def pop_heap(heap):
    """std::priority_queue::pop: std::pop_heap (__pop_heap + __adjust_heap) + pop_back."""
    length = len(heap)
    if length > 1:
        length -= 1
        value = heap[length]
        heap[length] = heap[0]
        hole = 0
        child = 0
        while child < (length - 1) // 2:
            child = 2 * (child + 1)
            if heap[child][0] < heap[child - 1][0]:
                child -= 1
            heap[hole] = heap[child]
            hole = child
        if length % 2 == 0 and child == (length - 2) // 2:
            child = 2 * (child + 1)
            heap[hole] = heap[child - 1]
            hole = child - 1
        parent = (hole - 1) // 2
        while hole > 0 and heap[parent][0] < value[0]:
            heap[hole] = heap[parent]
            hole = parent
            parent = (hole - 1) // 2
        heap[hole] = value
    heap.pop()


def find_similar_pairs6(sig, lsh_count, k, threshold, permutations, search_count, rows=None):
    """-> (cell [r, k], similarity [r, k] float32, usedCount [r]) for every cell, or for `rows` only."""
    n = sig.shape[0]
    rows = list(range(n)) if rows is None else [int(r) for r in rows]
    table = [math.cos(float(m) * math.pi / float(lsh_count)) for m in range(lsh_count + 1)]    # src/Lsh.cpp:229-249
    bits = np.unpackbits(sig.astype(">u8").view(np.uint8).reshape(n, -1), axis=1)
    words = [[int(x) for x in row] for row in sig]
    permuted_bits = permutations.shape[1]
    # permuted prefix of each cell as one Python integer of 64 * wordCount bits, first bit most significant
    width = ((permuted_bits - 1) // 64 + 1) * 64
    sorted_cells, position, prefixes = [], [], []
    for perm in permutations:
        prefix = [0] * n
        for cell in range(n):
            value = 0
            for source in perm:
                value = (value << 1) | int(bits[cell, source])
            prefix[cell] = value << (width - permuted_bits)
        order = sorted(range(n), key=lambda c: (prefix[c], c))
        sorted_cells.append(order)
        pos = [0] * n
        for i, c in enumerate(order):
            pos[c] = i
        position.append(pos)
        prefixes.append(prefix)

    def common_prefix(p, cell, index):
        x = prefixes[p][cell] ^ prefixes[p][sorted_cells[p][index]]
        return width if x == 0 else width - x.bit_length()

    cells = np.zeros((len(rows), k), dtype=np.uint32)
    sims = np.zeros((len(rows), k), dtype=np.float32)
    used = np.zeros(len(rows), dtype=np.uint32)
    for r, cell in enumerate(rows):
        heap = []
        for p in range(len(permutations)):
            i = position[p][cell]
            if i < n - 1:
                push_heap(heap, (common_prefix(p, cell, i + 1), p, i + 1, True))
            if i > 1:
                push_heap(heap, (common_prefix(p, cell, i - 1), p, i - 1, False))
        neighbours = []
        for _ in range(search_count):
            if not heap:
                break
            _, p, index, forward = heap[0]
            pop_heap(heap)
            other = sorted_cells[p][index]
            mismatch = sum(bin(a ^ b).count("1") for a, b in zip(words[cell], words[other]))
            if table[mismatch] > threshold:
                neighbours.append((other, np.float32(table[mismatch])))
            if forward and index < n - 1:
                push_heap(heap, (common_prefix(p, cell, index + 1), p, index + 1, True))
            elif not forward and index > 0:
                push_heap(heap, (common_prefix(p, cell, index - 1), p, index - 1, False))
        best = sorted(set(neighbours), key=lambda x: (-x[1], x[0]))[:k]
        used[r] = len(best)
        for j, (other, s) in enumerate(best):
            cells[r, j] = other
            sims[r, j] = s
    return cells, sims, used


@pytest.mark.parametrize("n,L,k,thr,P,S,pbits,seed,kind", [
    (40, 64, 5, 0.2, 4, 30, 1, 231, "clustered"),           # 1-bit prefixes: every length is 0 or 64, ties everywhere
    (40, 64, 50, -1.0, 3, 10**6, 1, 7, "clustered"),         # the queues empty; k above the neighbours
    (30, 128, 6, 0.0, 5, 40, 128, 5, "clustered"),           # two-word prefixes
    (50, 100, 4, 0.1, 6, 64, 70, -3, "clustered"),           # two words, the second with 6 live bits; L not a multiple of 64
    (25, 64, 8, 0.2, 4, 50, 64, 231, "identical"),           # all prefixes equal: every length 64
    (33, 192, 7, 0.2, 3, 25, 65, 11, "identical_pairs"),     # duplicated cells next to each other in every sorted list
    (3, 64, 3, 0.2, 2, 10, 8, 231, "clustered"),             # three cells: the backward-pointer quirk at position 1
    (60, 256, 10, 0.5, 8, 100, 16, 99, "clustered"),
])
def test_python_restatement_matches_cpp(restatement, n, L, k, thr, P, S, pbits, seed, kind):
    if kind == "identical":
        sig = np.tile(synth.random_signatures(1, L, seed=4), (n, 1))
    elif kind == "identical_pairs":
        base = synth.clustered_signatures((n + 1) // 2, L, cluster_count=2, flip=0.1, seed=n)
        sig = np.repeat(base, 2, axis=0)[:n]
    else:
        sig = synth.clustered_signatures(n, L, cluster_count=3, flip=0.1, seed=n + L)
    permutations = restatement.permutations(L, P, pbits, seed)
    expect = find_similar_pairs6(sig, L, k, thr, permutations, S)
    got = restatement.find_similar_pairs6(sig, L, k, thr, P, S, pbits, seed)
    assert np.array_equal(got[2], expect[2])
    assert np.array_equal(got[0], expect[0])
    assert np.array_equal(got[1].view(np.uint32), expect[1].view(np.uint32))
    if thr < 1.0 and n > 3:
        assert expect[2].sum() > 0


@pytest.mark.parametrize("n,L,k,thr,P,S,pbits,seed,kind", [
    (129, 128, 200, -0.5, 64, 8192, 64, 231, "clustered"),   # 64 x 128 pointers: the queues hold exactly 8192 pops
    (129, 64, 150, 0.2, 64, 10**6, 1, 3, "identical"),       # the same, reached by the clamp; every prefix length equal
    (300, 100, 20, -0.5, 64, 8192, 100, -9, "clustered"),    # searchCount 8192 stops the walk before the queues empty
    (257, 192, 30, 0.0, 64, 4097, 129, 17, "clustered"),     # just past a power of two; a third word with one live bit
])
def test_python_restatement_matches_cpp_at_the_search_limit(restatement, n, L, k, thr, P, S, pbits, seed, kind):
    """The GPU kernels' limits (64 permutations, 8192 candidates per cell) on a few rows of each shape: both restatements
    agree there too, so the C++ one can stand in for the reference at the sizes the GPU limit tests use."""
    if kind == "identical":
        sig = np.tile(synth.random_signatures(1, L, seed=5), (n, 1))
    else:
        sig = synth.clustered_signatures(n, L, cluster_count=2, flip=0.02, seed=n + L)
    rows = np.array([0, 1, 2, 63, 64, n // 2, n - 2, n - 1], dtype=np.uint32)
    permutations = restatement.permutations(L, P, pbits, seed)
    expect = find_similar_pairs6(sig, L, k, thr, permutations, S, rows=rows)
    got = restatement.find_similar_pairs6(sig, L, k, thr, P, S, pbits, seed, rows=rows)
    assert np.array_equal(got[2], expect[2])
    assert np.array_equal(got[0], expect[0])
    assert np.array_equal(got[1].view(np.uint32), expect[1].view(np.uint32))
    assert expect[2].min() > 0
