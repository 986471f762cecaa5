"""ctypes binding of tests/native/em2_gene_graph_restatement.cpp (the GeneGraph constructor and GeneGraph::getConnectivity
restated with a std::map vertex table, std::set out-edges and a std::list of edges) and the inputs the gene graph tests share.
Compiled with g++ at first use.  Test infrastructure only."""
import ctypes
import functools
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE_DIR = os.path.join(ROOT, "tests", "native")
SOURCE = os.path.join(NATIVE_DIR, "em2_gene_graph_restatement.cpp")
PAIR_DTYPE = np.dtype([("cell", "<u4"), ("similarity", "<f4")])
GRAPH_KEYS = ("vertices", "edgeGene0", "edgeGene1", "edgeSimilarity", "connectivityOffsets", "connectivityGenes",
              "connectivitySimilarities")
NO_LIMIT = 2 ** 64 - 1                                      # what size_t makes of the Python int -1

c = ctypes
P = c.c_void_p


def _ptr(a):
    return a.ctypes.data_as(c.c_void_p)


class GeneGraphRestatement:
    def __init__(self, lib):
        self.lib = lib
        lib.em2r_gene_graph_create.argtypes = [P, P, c.c_uint32, c.c_uint32, P, P, c.c_uint32, c.c_double, c.c_uint64, P]
        lib.em2r_gene_graph_create.restype = P
        lib.em2r_gene_graph_sizes.argtypes = [P, P, P, P]
        lib.em2r_gene_graph_sizes.restype = None
        lib.em2r_gene_graph_get.argtypes = [P] * 8
        lib.em2r_gene_graph_get.restype = None
        lib.em2r_gene_graph_free.argtypes = [P]
        lib.em2r_gene_graph_free.restype = None

    def gene_graph(self, pairs, used_count, pairs_gene_set, graph_gene_set, similarity_threshold, max_connectivity):
        """-> the dict of capi.gene_graph_take, and "seconds" (the constructor on one thread)."""
        pairs = np.ascontiguousarray(pairs, dtype=PAIR_DTYPE)
        used_count = np.ascontiguousarray(used_count, dtype=np.uint32)
        pairs_genes = np.ascontiguousarray(pairs_gene_set, dtype=np.uint32)
        graph_genes = np.ascontiguousarray(graph_gene_set, dtype=np.uint32)
        assert pairs.ndim == 2 and pairs.shape[0] == len(pairs_genes) == len(used_count)
        seconds = c.c_double(0.)
        handle = self.lib.em2r_gene_graph_create(_ptr(pairs), _ptr(used_count), len(pairs_genes), pairs.shape[1], _ptr(pairs_genes),
                                                 _ptr(graph_genes), len(graph_genes), similarity_threshold,
                                                 int(max_connectivity) % 2 ** 64, c.byref(seconds))
        try:
            sizes = [c.c_uint64(0) for _ in range(3)]
            self.lib.em2r_gene_graph_sizes(handle, *[c.byref(s) for s in sizes])
            vertices, edges, removed = (s.value for s in sizes)
            out = {
                "vertices": np.zeros(vertices, dtype=np.uint32),
                "edgeGene0": np.zeros(edges, dtype=np.uint32),
                "edgeGene1": np.zeros(edges, dtype=np.uint32),
                "edgeSimilarity": np.zeros(edges, dtype=np.float32),
                "connectivityOffsets": np.zeros(len(graph_genes) + 1, dtype=np.uint64),
                "connectivityGenes": np.zeros(2 * edges, dtype=np.uint32),
                "connectivitySimilarities": np.zeros(2 * edges, dtype=np.float32),
            }
            self.lib.em2r_gene_graph_get(handle, *[_ptr(out[key]) for key in GRAPH_KEYS])
            out["removedCount"] = removed
            out["seconds"] = seconds.value
        finally:
            self.lib.em2r_gene_graph_free(handle)
        return out


@functools.lru_cache(maxsize=None)
def load():
    build = os.path.join(NATIVE_DIR, "build")
    os.makedirs(build, exist_ok=True)
    path = os.path.join(build, "libem2genegraphrestatement.so")
    if not os.path.exists(path) or os.path.getmtime(path) < os.path.getmtime(SOURCE):
        tmp = path + ".%d.tmp" % os.getpid()
        cmd = ["g++", "-std=c++17", "-O2", "-fPIC", "-shared", "-o", tmp, SOURCE]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError("gene graph restatement build failed: " + r.stderr)
        os.replace(tmp, path)
    return GeneGraphRestatement(ctypes.CDLL(path))


def bits(a):
    """A float32 array as uint32: NaN compares equal to itself, -0.0 differs from 0.0."""
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def assert_same_graph(mine, theirs, what):
    assert mine["removedCount"] == theirs["removedCount"], "%s: removedCount %d != %d" % (what, mine["removedCount"], theirs["removedCount"])
    for key in GRAPH_KEYS:
        a, b = mine[key], theirs[key]
        assert a.dtype == b.dtype and a.shape == b.shape, "%s: %s has another size" % (what, key)
        if a.dtype == np.float32:
            a, b = bits(a), bits(b)
        assert np.array_equal(a, b), "%s: %s differs" % (what, key)


# ---- inputs ----
# A case is a dict: pairs [|P|, k] PAIR_DTYPE, used [|P|], P and S (ascending global gene ids), threshold (a Python float,
# i.e. a double) and limit (maxConnectivity as the Python int the caller passes: 0 and negative values mean no limit).

def lists_to_case(lists, k, p_ids, s_ids, threshold, limit):
    """lists[g] = [(partner local id in P, similarity), ...] as stored (the caller orders them)."""
    pairs = np.zeros((len(p_ids), k), dtype=PAIR_DTYPE)
    used = np.zeros(len(p_ids), dtype=np.uint32)
    for g, entries in enumerate(lists):
        assert len(entries) <= k
        used[g] = len(entries)
        for j, (partner, similarity) in enumerate(entries):
            pairs[g, j] = (partner, similarity)
    return {"pairs": pairs, "used": used, "P": np.asarray(p_ids, dtype=np.uint32), "S": np.asarray(s_ids, dtype=np.uint32),
            "threshold": float(threshold), "limit": int(limit)}


# the similarities of the random cases: few distinct float32 values, so that ties and thresholds equal to a stored value occur
GRID = np.linspace(0.05, 0.95, 19).astype(np.float32)

SET_KINDS = ("equal", "subset", "superset", "interleaved", "disjoint")


def random_case(seed, p_count, k, set_kind="equal", gaps=False, limit=3, threshold=None, duplicates=False):
    """Random stored lists over P: gene 0 stores nothing, gene 1 (if there are enough genes) k pairs, the others 0..k; the
    partners are mostly near the gene, so that both ends often select an edge; similarities from GRID, descending."""
    rng = np.random.default_rng(seed)
    universe = np.sort(rng.choice(4 * p_count + 8, 2 * p_count + 4, replace=False)).astype(np.uint32) if gaps else np.arange(
        100, 100 + 2 * p_count + 4, dtype=np.uint32)
    # P and S as positions in the universe.  Without gaps both stay ranges of consecutive ids (the look-up without a search)
    # wherever the kind allows; with gaps neither is.
    if set_kind == "equal":
        p_at = s_at = np.arange(p_count)
    elif set_kind == "subset":                               # S a strict subset of P (p_count 1: S = P)
        p_at = np.arange(p_count)
        size = max(1, (2 * p_count) // 3)
        s_at = np.sort(rng.choice(p_count, size, replace=False)) if gaps else np.arange(p_count // 4, p_count // 4 + size)
    elif set_kind == "superset":                             # S a strict superset of P
        s_at = np.arange(p_count + 3)
        p_at = np.sort(rng.choice(p_count + 3, p_count, replace=False)) if gaps else np.arange(1, p_count + 1)
    elif set_kind == "interleaved":                          # each holds genes the other lacks
        if gaps:
            p_at = np.arange(0, 2 * p_count, 2)
            s_at = np.sort(np.concatenate([p_at[::2], np.arange(1, 2 * p_count, 4)]))
        else:
            p_at = np.arange(p_count)
            s_at = np.arange((p_count + 1) // 2, (p_count + 1) // 2 + p_count)
    elif set_kind == "disjoint":
        p_at = np.arange(p_count)
        s_at = np.arange(p_count, 2 * p_count)
    else:
        raise ValueError(set_kind)
    p_ids, s_ids = universe[p_at], universe[s_at]
    lists = []
    for g in range(p_count):
        others = p_count - 1
        most = min(k, others) if not duplicates else (k if others else 0)
        count = 0 if g == 0 else (most if g == 1 else int(rng.integers(0, most + 1)))
        if count:
            near = (g + rng.integers(1, min(others, 6) + 1, size=4 * k)) % p_count
            far = rng.integers(0, p_count, size=4 * k)
            candidates = np.where(rng.random(4 * k) < 0.7, near, far)
            candidates = candidates[candidates != g]
            if not duplicates:
                _, first = np.unique(candidates, return_index=True)
                candidates = candidates[np.sort(first)]
                if len(candidates) < count:
                    rest = np.setdiff1d(np.arange(p_count), np.concatenate([candidates, [g]]))
                    candidates = np.concatenate([candidates, rng.permutation(rest)])
            partners = candidates[:count]
            count = len(partners)
            similarities = np.sort(rng.choice(GRID, count))[::-1]
            lists.append(list(zip(partners.tolist(), similarities.tolist())))
        else:
            lists.append([])
    if threshold is None:
        threshold = float(GRID[int(rng.integers(0, len(GRID)))]) if rng.random() < 0.5 else float(rng.uniform(0., 1.))
    return lists_to_case(lists, k, p_ids, s_ids, threshold, limit)


def _edge_kinds():
    # 0 <-> 1 selected by both ends, (2, 3) by the lower end only, (4, 5) by the higher end only
    lists = [[(1, 0.9)], [(0, 0.9)], [(3, 0.8)], [], [], [(4, 0.7)]]
    return lists_to_case(lists, 2, np.arange(6), np.arange(6), 0.5, 0)


def _asymmetric():
    """The two ends store different similarities: the lower vertex's value wins where it selected the edge (0-1: 0.9, not
    0.8), otherwise the higher vertex's (2-3: 3 alone stores it; 4-5: 4's 0.3 is below the threshold, 5's 0.6 is not)."""
    lists = [[(1, 0.9)], [(0, 0.8)], [], [(2, 0.7)], [(5, 0.3)], [(4, 0.6)]]
    return lists_to_case(lists, 2, np.arange(6), np.arange(6), 0.5, 0)


def _limit_on_the_last_pair():
    # gene 0 stores exactly three pairs, all in S: the count reaches 3 on the last one; gene 4 stores k = 4
    lists = [[(1, 0.9), (2, 0.8), (3, 0.7)], [], [], [], [(0, 0.9), (1, 0.8), (2, 0.7), (3, 0.6)]]
    return lists_to_case(lists, 4, np.arange(5), np.arange(5), 0.1, 3)


def _limit_reached_by_a_duplicate():
    """Limit 2.  Gene 1 stores 0, 2, 3: add_edge(1, 0) finds the edge gene 0 made and still counts, (1, 2) is the second,
    (1, 3) is never added.  Gene 4 stores gene 5 twice (no file of findSimilarGenePairs0 does): the second is a no-op that
    counts too, so (4, 3) is not added either."""
    lists = [[(1, 0.9)], [(0, 0.9), (2, 0.8), (3, 0.7)], [], [], [(5, 0.9), (5, 0.8), (3, 0.7)], []]
    return lists_to_case(lists, 3, np.arange(6), np.arange(6), 0.1, 2)


STORED = np.float32(0.6)                                    # 0.60000002384...


def _threshold(kind):
    below = np.nextafter(np.float32(0.2), np.float32(0))
    lists = [[(1, 0.9), (2, float(STORED)), (3, 0.5)], [], [], [],
             [(5, 0.9), (6, float(np.float32(0.2))), (7, float(below))], [], [], []]
    threshold = {"equal": float(STORED), "ulp-above": float(np.nextafter(np.float64(STORED), np.inf)), "0.2": 0.2}[kind]
    return lists_to_case(lists, 3, np.arange(8), np.arange(8), threshold, 0)


def _nan():
    # a NaN in the middle of a list: NaN < threshold is false, the pair is kept and the walk goes on to 0.7 and stops at 0.1
    lists = [[(1, 0.9), (2, float("nan")), (3, 0.7), (4, 0.1)], [], [], [], [], [(0, float("nan"))]]
    return lists_to_case(lists, 4, np.arange(6), np.arange(6), 0.5, 0)


def _incoming_only():
    # genes 1..4 store nothing and survive because gene 0 selected them; 5 is isolated
    lists = [[(1, 0.9), (2, 0.8), (3, 0.7), (4, 0.6)], [], [], [], [], []]
    return lists_to_case(lists, 4, np.arange(6), np.arange(6), 0.5, 0)


def _ring(n=70):
    lists = [[((g + 1) % n, 0.9)] for g in range(n)]
    return lists_to_case(lists, 1, np.arange(10, 10 + n), np.arange(10, 10 + n), 0.5, 1)


def _hub(n=600, k=4):
    """Every gene selects gene 0 (limit 1): its degree n - 1 exceeds k and a block of 256."""
    lists = [[(1, 0.9), (2, 0.8), (3, 0.7), (4, 0.6)]] + [[(0, 0.9)] + [((g + d) % (n - 1) + 1, 0.8 - 0.1 * d) for d in (1, 2, 3)] for g in range(1, n)]
    for g in range(1, n):
        assert all(partner != g for partner, _ in lists[g])
    return lists_to_case(lists, k, np.arange(n), np.arange(n), 0.1, 1)


def _with(case_, **changes):
    out = dict(case_)
    out.update(changes)
    return out


@functools.lru_cache(maxsize=None)
def case(name):
    """A named input; built once, never modified (the arrays are read-only)."""
    if name.startswith("genes-"):                            # genes-<n>: S = P, n genes, k = 8, limit 3
        n = int(name.split("-")[1])
        out = random_case(1000 + n, n, 8, limit=3, threshold=0.3)
    elif name.startswith("sets-"):                           # sets-<kind>-<consecutive|gaps>
        _, kind, spacing = name.split("-")
        out = random_case(2000 + SET_KINDS.index(kind) * 2 + (spacing == "gaps"), 90, 6, set_kind=kind, gaps=spacing == "gaps", limit=4, threshold=0.3)
    else:
        out = {
            "limit-1": lambda: random_case(31, 200, 8, limit=1, threshold=0.2),
            "limit-0": lambda: random_case(32, 200, 8, limit=0, threshold=0.2),
            "limit-negative": lambda: random_case(32, 200, 8, limit=-1, threshold=0.2),
            "limit-on-the-last-pair": _limit_on_the_last_pair,
            "limit-reached-by-a-duplicate": _limit_reached_by_a_duplicate,
            "threshold-equal": lambda: _threshold("equal"),
            "threshold-ulp-above": lambda: _threshold("ulp-above"),
            "threshold-0.2": lambda: _threshold("0.2"),
            "nan": _nan,
            "edge-kinds": _edge_kinds,
            "asymmetric": _asymmetric,
            "incoming-only": _incoming_only,
            "nothing-isolated": _ring,
            "everything-isolated": lambda: _with(random_case(41, 300, 8, threshold=0.3), threshold=2.0),
            "hub": _hub,
            "duplicates": lambda: random_case(51, 150, 8, limit=5, threshold=0.25, duplicates=True),
            "k-16": lambda: random_case(52, 1000, 16, set_kind="subset", gaps=True, limit=0, threshold=0.4),
        }[name]()
    for key in ("pairs", "used", "P", "S"):
        out[key].setflags(write=False)
    return out


GRAPH_CASES = ["genes-%d" % n for n in (1, 63, 64, 65, 257, 1000)] + [
    "sets-%s-%s" % (kind, spacing) for kind in SET_KINDS for spacing in ("consecutive", "gaps")] + [
    "limit-1", "limit-0", "limit-negative", "limit-on-the-last-pair", "limit-reached-by-a-duplicate", "threshold-equal",
    "threshold-ulp-above", "threshold-0.2", "nan", "edge-kinds", "asymmetric", "incoming-only", "nothing-isolated",
    "everything-isolated", "hub", "duplicates", "k-16"]


def fuzz_case(i):
    """Case i of the fuzz: every shape of the named cases, at random.  Not cached (about 200 of them)."""
    rng = np.random.default_rng(7000 + i)
    p_count = int(rng.choice([1, 2, 3, 7, 63, 64, 65, 130, 257]))
    k = int(rng.choice([1, 2, 5, 16]))
    kind = SET_KINDS[int(rng.integers(0, len(SET_KINDS)))]
    limit = int(rng.choice([0, -1, 1, 2, 3, k, k + 1]))
    return random_case(8000 + i, p_count, k, set_kind=kind, gaps=bool(rng.integers(0, 2)), limit=limit,
                       duplicates=bool(rng.random() < 0.25))


FUZZ_COUNT = 200


def arguments(case_):
    return (case_["pairs"], case_["used"], case_["P"], case_["S"], case_["threshold"], case_["limit"])


@functools.lru_cache(maxsize=None)
def reference(name):
    """The restatement's graph of a named case; computed once and shared (the arrays are read-only)."""
    out = load().gene_graph(*arguments(case(name)))
    for key in GRAPH_KEYS:
        out[key].setflags(write=False)
    return out
