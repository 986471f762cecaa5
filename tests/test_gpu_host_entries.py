"""The host-buffer searches em2_find_similar_pairs4/5/6/7 through the raw C ABI: what they share is the wrapper around the
device-level call -- signatures up, the call, pairs (when k > 0) and used counts down.  65 cells x 128 bits: more than one
wave's worth of rows, the last wave partial.  k = 3: pairs and used counts bit-identical to the oracle (findSimilarPairs6:
to the C++ restatement).  k = 0 with pairs = NULL: OK and every used count zero (keepBest(v, 0) empties every list), with
the used counts set to a sentinel before the call so that a call that does not write them is seen."""
import numpy as np
import pytest

import fsp6_binding
import synth
from expressionmatrix2_amd import capi

pytestmark = pytest.mark.gpu

N, L, K, THR = 65, 128, 3, 0.2
SLICES = np.array([10, 8], dtype=np.int32)
# entry point -> (arguments between similarityThreshold and pairs, the oracle's answer)
ENTRIES = {
    "em2_find_similar_pairs4": ((), lambda o, r, sig, k: o.find_similar_pairs4(sig, L, k, THR)),
    "em2_find_similar_pairs5": ((8, 1000), lambda o, r, sig, k: o.find_similar_pairs5(sig, L, k, THR, 8, 1000)),
    "em2_find_similar_pairs6": ((4, 50, 64, 231), lambda o, r, sig, k: r.find_similar_pairs6(sig, L, k, THR, 4, 50, 64, 231)),
    "em2_find_similar_pairs7": ((SLICES.ctypes.data, 2, 100, 12),
                                lambda o, r, sig, k: o.find_similar_pairs7(sig, L, k, THR, [10, 8], 100, 12)),
}


@pytest.fixture(scope="module")
def signatures():
    return np.ascontiguousarray(synth.clustered_signatures(N, L, cluster_count=4, flip=0.12, seed=65), dtype=np.uint64)


@pytest.mark.parametrize("name", sorted(ENTRIES))
def test_host_entry_matches_oracle(oracle, signatures, name):
    extra, expected = ENTRIES[name]
    lib = capi.load()
    pairs = np.zeros((N, K), dtype=capi.PAIR_DTYPE)
    used = np.full(N, 0xdeadbeef, dtype=np.uint32)
    rc = getattr(lib, name)(signatures.ctypes.data, N, L, K, THR, *extra, pairs.ctypes.data, used.ctypes.data)
    assert rc == capi.EM2_OK, lib.em2_last_error().decode()
    cell, sim, oused = expected(oracle, fsp6_binding.load(), signatures, K)
    assert oused.sum() > 0
    assert np.array_equal(used, oused)
    assert np.array_equal(pairs["cell"], cell)
    assert np.array_equal(pairs["similarity"].view(np.uint32), sim.view(np.uint32))


@pytest.mark.parametrize("name", sorted(ENTRIES))
def test_host_entry_k0_without_pairs(signatures, name):
    extra, _ = ENTRIES[name]
    lib = capi.load()
    used = np.full(N, 0xdeadbeef, dtype=np.uint32)
    rc = getattr(lib, name)(signatures.ctypes.data, N, L, 0, THR, *extra, None, used.ctypes.data)
    assert rc == capi.EM2_OK, lib.em2_last_error().decode()
    assert np.array_equal(used, np.zeros(N, dtype=np.uint32))
