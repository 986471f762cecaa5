"""Times findSimilarPairs6 (em2_dev_find_similar_pairs6) on one GPU and the C++ restatement
(tests/native/em2_fsp6_restatement.cpp, one CPU thread) on sampled rows, the latter extrapolated to all rows and labelled so.
Prints one JSON line.  Under `rocprofv3 --kernel-trace --stats -- python tools/fsp6_time.py ...` the stats give the phase
breakdown (permuteKernel / the rocPRIM sort passes / scatterKernel / walkKernel / selectKernel).

    python tools/fsp6_time.py [--cells 1000000] [--lsh-count 1024] [--permutations 16] [--search 400] [--k 100]
                              [--threshold 0.2] [--sample-rows 256] [--repeats 3]

Signatures: 64 random cluster centres, every bit flipped with probability 1/8 (cheap to make at 1M cells; the tests use
tests/synth.clustered_signatures)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from expressionmatrix2_amd import capi          # noqa: E402
import synth                                    # noqa: E402


def signatures(n, lsh_count, clusters=64, seed=6):
    words = (lsh_count - 1) // 64 + 1
    centres = synth.random_signatures(clusters, lsh_count, seed=seed)
    cluster = synth.hash_u64(seed, 1, np.arange(n, dtype=np.uint64)) % np.uint64(clusters)
    noise = (synth.random_signatures(n, lsh_count, seed=seed + 1) & synth.random_signatures(n, lsh_count, seed=seed + 2)
             & synth.random_signatures(n, lsh_count, seed=seed + 3))
    sig = centres[cluster.astype(np.int64)] ^ noise
    pad = words * 64 - lsh_count
    if pad:
        sig[:, -1] &= ~np.uint64((1 << pad) - 1)
    return np.ascontiguousarray(sig)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, default=1000000)
    ap.add_argument("--lsh-count", type=int, default=1024)
    ap.add_argument("--permutations", type=int, default=16)
    ap.add_argument("--search", type=int, default=400)
    ap.add_argument("--permuted-bits", type=int, default=64)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--threshold", type=float, default=0.2)
    ap.add_argument("--seed", type=int, default=231)
    ap.add_argument("--sample-rows", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=3)
    a = ap.parse_args()
    import torch

    n, L, k = a.cells, a.lsh_count, a.k
    sig = signatures(n, L)
    d_sig = torch.from_numpy(sig.view(np.int64)).cuda()
    d_pairs = torch.zeros((n, k, 2), dtype=torch.int32, device="cuda")
    d_used = torch.zeros(n, dtype=torch.int32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    times = []
    for _ in range(a.repeats + 1):                   # the first call also loads the library's code objects
        torch.cuda.synchronize()
        t = time.perf_counter()
        capi.dev_find_similar_pairs6(d_sig.data_ptr(), n, 0, n, L, k, a.threshold, a.permutations, a.search, a.permuted_bits,
                                     a.seed, d_pairs.data_ptr(), d_used.data_ptr(), stream)
        times.append(time.perf_counter() - t)
    used = d_used.cpu().numpy().view(np.uint32)
    pairs = d_pairs.cpu().numpy().view(np.uint32)
    out = {"what": "findSimilarPairs6 on one GPU (em2_dev_find_similar_pairs6, device-resident signatures)",
           "cells": n, "lsh_count": L, "k": k, "threshold": a.threshold, "permutation_count": a.permutations,
           "search_count": a.search, "permuted_bit_count": a.permuted_bits, "seed": a.seed,
           "gpu_seconds_first_call": round(times[0], 4), "gpu_seconds": [round(x, 4) for x in times[1:]],
           "gpu_seconds_median": round(float(np.median(times[1:])), 4), "stored_pairs": int(used.sum())}

    if a.sample_rows > 0:
        import fsp6_binding
        restatement = fsp6_binding.load()
        rows = np.unique(synth.hash_u64(3, np.arange(a.sample_rows * 2, dtype=np.uint64)) % np.uint64(n)).astype(np.uint32)
        rows = rows[:a.sample_rows]
        t = time.perf_counter()
        restatement.find_similar_pairs6(sig, L, k, a.threshold, a.permutations, a.search, a.permuted_bits, a.seed,
                                        rows=rows[:0])
        phase1 = time.perf_counter() - t
        t = time.perf_counter()
        cell, sim, rused = restatement.find_similar_pairs6(sig, L, k, a.threshold, a.permutations, a.search,
                                                           a.permuted_bits, a.seed, rows=rows)
        both = time.perf_counter() - t
        per_row = max(0.0, both - phase1) / len(rows)
        same = (np.array_equal(rused, used[rows]) and np.array_equal(cell, pairs[rows, :, 0])
                and np.array_equal(sim.view(np.uint32), pairs[rows, :, 1]))
        out.update({"restatement_rows_sampled": int(len(rows)), "restatement_phase1_seconds": round(phase1, 3),
                    "restatement_seconds_per_row": per_row,
                    "restatement_seconds_all_rows_EXTRAPOLATED": round(phase1 + per_row * n, 1),
                    "sampled_rows_bit_exact": bool(same)})
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
