"""ctypes binding of tests/native/em2_fsp6_restatement.cpp, the literal C++ restatement of findSimilarPairs6
(src/ExpressionMatrixLsh.cpp:842-1145).  Compiled with g++ at first use, like oracle_binding.load_host_checks, so that
its std::shuffle and std::priority_queue are the libstdc++ of the box the tests run on.  Test infrastructure only."""
import ctypes
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE_DIR = os.path.join(ROOT, "tests", "native")
SOURCE = os.path.join(NATIVE_DIR, "em2_fsp6_restatement.cpp")

c = ctypes
P = c.c_void_p


def _ptr(a):
    return a.ctypes.data_as(c.c_void_p)


class Fsp6Restatement:
    def __init__(self, lib):
        self.lib = lib
        lib.em2r_fsp6_permutations.argtypes = [c.c_uint32, c.c_uint32, c.c_uint32, c.c_int32, P]
        lib.em2r_fsp6_permutations.restype = None
        lib.em2r_find_similar_pairs6.argtypes = [P, c.c_uint32, c.c_uint32, c.c_uint32, c.c_double, c.c_uint32, c.c_uint32,
                                                 c.c_uint32, c.c_int32, P, c.c_uint32, P, P, P]
        lib.em2r_find_similar_pairs6.restype = c.c_int

    def permutations(self, lsh_count, permutation_count, permuted_bit_count, seed):
        """[permutation_count, permuted_bit_count] source bit of each permuted bit."""
        out = np.zeros((permutation_count, permuted_bit_count), dtype=np.uint32)
        self.lib.em2r_fsp6_permutations(lsh_count, permutation_count, permuted_bit_count, seed, _ptr(out))
        return out

    def find_similar_pairs6(self, sig, lsh_count, k, thr, permutation_count, search_count, permuted_bit_count=64, seed=231,
                            rows=None):
        """-> (cell [r, k], similarity [r, k] float32, usedCount [r]) for every cell, or for `rows` only."""
        sig = np.ascontiguousarray(sig, dtype=np.uint64)
        n = sig.shape[0]
        row_array = None if rows is None else np.ascontiguousarray(rows, dtype=np.uint32)
        r = n if row_array is None else len(row_array)
        cell = np.zeros((r, k), dtype=np.uint32)
        sim = np.zeros((r, k), dtype=np.float32)
        used = np.zeros(r, dtype=np.uint32)
        rc = self.lib.em2r_find_similar_pairs6(_ptr(sig), n, lsh_count, k, thr, permutation_count, search_count,
                                               permuted_bit_count, seed, None if row_array is None else _ptr(row_array),
                                               r, _ptr(cell), _ptr(sim), _ptr(used))
        if rc != 0:
            raise ValueError("the fsp6 restatement rejected the arguments (%d)" % rc)
        return cell, sim, used


def load():
    build = os.path.join(NATIVE_DIR, "build")
    os.makedirs(build, exist_ok=True)
    path = os.path.join(build, "libem2fsp6restatement.so")
    if not os.path.exists(path) or os.path.getmtime(path) < os.path.getmtime(SOURCE):
        tmp = path + ".%d.tmp" % os.getpid()
        cmd = ["g++", "-std=c++17", "-O2", "-msse4.2", "-ffp-contract=off", "-fPIC", "-shared", "-o", tmp, SOURCE]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError("fsp6 restatement build failed: " + r.stderr)
        os.replace(tmp, path)
    return Fsp6Restatement(ctypes.CDLL(path))
