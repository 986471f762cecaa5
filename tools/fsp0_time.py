"""Times findSimilarPairs0 (em2_dev_find_similar_pairs0) on one GPU and the C++ restatement's pair loop
(tests/native/em2_fsp0_restatement.cpp, one CPU thread) on a range of rows of the same data on the same box, the latter
extrapolated to all pairs by pair count and labelled so.  Prints one JSON line per size and writes it to
profiles/fsp0_time_<cells>.json.  Under `rocprofv3 --kernel-trace --stats -- python tools/fsp0_time.py ...` the stats give
the kernel time of fsp0RowsKernel.

    python tools/fsp0_time.py [--cells 20000 50000] [--genes 20000] [--density 0.01] [--k 100] [--threshold 0.2]
                              [--restatement-rows 200] [--repeats 2] [--output-directory profiles]

Also printed: sum over rows i of sum over columns j != i of nnz(j), the count of 8-byte loads and LDS gathers the kernel
issues."""
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
import fsp0_binding                             # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, nargs="+", default=[20000, 50000])
    ap.add_argument("--genes", type=int, default=20000)
    ap.add_argument("--density", type=float, default=0.01)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--threshold", type=float, default=0.2)
    ap.add_argument("--restatement-rows", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--output-directory", default=os.path.join(ROOT, "profiles"))
    a = ap.parse_args()
    import torch

    restatement = fsp0_binding.load()
    for n in a.cells:
        toc, data = fsp0_binding.clustered(n, a.genes, a.density, cluster_count=64)
        nnz = int(toc[-1])
        d = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).copy()).cuda()
        d_toc, d_data = d(toc), d(data)
        ws_bytes = capi.dev_find_similar_pairs0_workspace(n, n, a.genes, a.k)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device="cuda")
        d_pairs = torch.zeros((n, a.k, 2), dtype=torch.int32, device="cuda")
        d_used, d_index, d_low = (torch.zeros(n, dtype=torch.int32, device="cuda") for _ in range(3))
        stream = torch.cuda.current_stream().cuda_stream
        times = []
        for _ in range(a.repeats + 1):               # the first call also loads the library's code objects
            torch.cuda.synchronize()
            t = time.perf_counter()
            capi.dev_find_similar_pairs0(d_toc.data_ptr(), d_data.data_ptr(), n, a.genes, 0, n, a.k, a.threshold, d_pairs.data_ptr(),
                                         d_used.data_ptr(), d_index.data_ptr(), d_low.data_ptr(), ws.data_ptr(), ws_bytes, stream)
            times.append(time.perf_counter() - t)
        used = d_used.cpu().numpy().view(np.uint32)
        pairs = n * (n - 1) // 2
        gpu = float(np.median(times[1:])) if a.repeats else times[0]
        out = {"what": "findSimilarPairs0 on one GPU (em2_dev_find_similar_pairs0, device-resident CSR)", "cells": n,
               "genes": a.genes, "density": a.density, "nnz": nnz, "k": a.k, "threshold": a.threshold,
               "gpu_seconds_first_call": round(times[0], 4), "gpu_seconds": [round(x, 4) for x in times[1:]],
               "gpu_seconds_median": round(gpu, 4), "stored_pairs": int(used.sum()), "unordered_pairs": pairs,
               "gpu_ns_per_unordered_pair": gpu / pairs * 1e9,
               "loads_and_gathers_issued": n * nnz - nnz,       # sum_i sum_{j != i} nnz(j) = (n - 1) * nnz
               "reference_published_seconds_at_20us_per_pair": pairs * 20e-6}
        rows = min(a.restatement_rows, n - 1)
        if rows > 0:
            t = time.perf_counter()
            found = restatement.count_similar_pairs_of_rows(toc, data, a.genes, 0, rows, a.threshold)
            seconds = time.perf_counter() - t
            row_pairs = sum(n - 1 - r for r in range(rows))
            out.update({"restatement_rows": rows, "restatement_pairs": row_pairs, "restatement_seconds": round(seconds, 3),
                        "restatement_pairs_above_threshold": found, "restatement_ns_per_pair": seconds / row_pairs * 1e9,
                        "restatement_seconds_all_pairs_EXTRAPOLATED": round(seconds / row_pairs * pairs, 1),
                        "speedup_against_restatement_EXTRAPOLATED": round(seconds / row_pairs * pairs / gpu, 1),
                        "speedup_against_reference_published_20us_per_pair": round(pairs * 20e-6 / gpu, 1)})
        line = json.dumps(out)
        print(line, flush=True)
        os.makedirs(a.output_directory, exist_ok=True)
        with open(os.path.join(a.output_directory, "fsp0_time_%d.json" % n), "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
