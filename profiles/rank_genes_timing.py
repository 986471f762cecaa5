"""Timing of the rank-sum marker genes (csrc/em2_rank_genes.hip) on the bench's synthetic matrix
(expressionmatrix2_amd/synthetic.py), L2 normalisation, through the device-pointer entry:

    python profiles/rank_genes_timing.py [--cells N] [--genes G] [--repeats R] [--output profiles/rank_genes_timing_<cells>.json]

Workload: N cells x G genes of the bench generator, its chain up to the clusters (findSimilarPairs4 with k = 100 at threshold
0.2, the cell graph at k = 20, label propagation), and as groups the clusters of at least 100 cells -- what createClusterGraph
keeps; the cells of smaller clusters belong to no group.  One process: a warm-up call, R whole calls with the stage timing off,
R calls with EM2_TIMING=1, whose stages synchronise, for the stage split, and the same once more with the accumulate pass's
counters forced to global memory (em2_set_rank_genes_test_limits).  Next to the stage times stand the bytes a stage has to move
once and the time they take at the 6.29 TB/s this project measures as its streaming rate.  The C++ restatement
(tests/native/em2_rank_genes_restatement.cpp) runs on one thread of the same box on the first genes only; its time for all genes
is EXTRAPOLATED from them and labelled so, and the device's integers for those genes are compared with it.  The GPU step runs in
a child process under a time limit of its own; where it fails nothing more is started."""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

LSH, K, THRESHOLD, GRAPH_K, MIN_CLUSTER = 1024, 100, 0.2, 20, 100
STREAMING = 6.29e12
NO_GROUP = 0xffffffff


def child(args):
    import torch
    from expressionmatrix2_amd import capi, sharded, synthetic
    import rank_genes_binding as rgb
    lib = capi.load()
    device = torch.device("cuda")
    C, G = args.cells, args.genes
    toc, data = synthetic.expression_shard(0, C, G, density=args.density, device=device)
    entries = int(data.numel())
    pipe = sharded.DevicePipeline(C, G, LSH, K, THRESHOLD, world_size=1, rank=0, dist=None, device=device)
    pipe.set_inputs(toc, data, torch.from_numpy(capi.lsh_generate_vectors(G, LSH, 231)).to(device))
    pipe.step()
    pipe.check()
    torch.cuda.synchronize()
    cells = np.arange(C, dtype=np.uint32)
    v0 = torch.empty(C * GRAPH_K, dtype=torch.int32, device=device)
    v1 = torch.empty(C * GRAPH_K, dtype=torch.int32, device=device)
    sim = torch.empty(C * GRAPH_K, dtype=torch.float32, device=device)
    edges = capi.dev_cell_graph_edges_to_device(pipe.pairs.data_ptr(), pipe.used.data_ptr(), C, K, cells, cells, THRESHOLD, GRAPH_K,
                                                v0.data_ptr(), v1.data_ptr(), sim.data_ptr())
    clusters, _ = capi.dev_cell_graph_label_propagation(cells, v0.data_ptr(), v1.data_ptr(), sim.data_ptr(), edges)
    del pipe, v0, v1, sim
    capi.dev_release_scratch()
    sizes = np.bincount(clusters)
    kept = int((sizes >= MIN_CLUSTER).sum())                  # (clusters are numbered by decreasing size)
    group = np.where(clusters < kept, clusters, NO_GROUP).astype(np.uint32)
    d_group = torch.from_numpy(group.view(np.int32).copy()).to(device)

    counts = (data >> 32).to(torch.int32).view(torch.float32)
    rows = torch.repeat_interleave(torch.arange(C, device=device), toc[1:] - toc[:-1])
    sum2 = torch.zeros(C, dtype=torch.float64, device=device).index_add_(0, rows, (counts * counts).to(torch.float64))
    norm = 1. / torch.sqrt(sum2)          # (the sum's order is torch's: this script times, the tests check the norms)
    del rows, counts, sum2

    d_size = torch.zeros(kept, dtype=torch.int32, device=device)
    d_count = torch.zeros(G * kept, dtype=torch.int32, device=device)
    d_sum = torch.zeros(G * kept, dtype=torch.int64, device=device)
    d_tie = torch.zeros(G, dtype=torch.int64, device=device)

    def calls(label):
        workspace_bytes = lib.em2_dev_rank_genes_workspace(C, G, entries, kept)
        workspace = torch.empty(workspace_bytes, dtype=torch.uint8, device=device)

        def call():
            capi.check(lib.em2_dev_rank_genes(toc.data_ptr(), data.data_ptr(), C, G, entries, norm.data_ptr(), d_group.data_ptr(), kept,
                                              d_size.data_ptr(), d_count.data_ptr(), d_sum.data_ptr(), d_tie.data_ptr(),
                                              workspace.data_ptr(), workspace_bytes, None))
        os.environ["EM2_TIMING"] = "0"                        # (the library reads EM2_TIMING at every call)
        call()
        for _ in range(args.repeats):
            torch.cuda.synchronize()
            begin = time.perf_counter()
            call()
            print("[whole call, %s] %.3f ms" % (label, 1000. * (time.perf_counter() - begin)), file=sys.stderr, flush=True)
        os.environ["EM2_TIMING"] = "1"
        print("[stages, %s]" % label, file=sys.stderr, flush=True)
        for _ in range(args.repeats):
            call()
        os.environ["EM2_TIMING"] = "0"
        return workspace_bytes

    workspace_bytes = calls("LDS counters")
    lib.em2_set_rank_genes_test_limits(0, 0, 1)
    calls("global counters")
    lib.em2_set_rank_genes_test_limits(0, 0, 0)

    n = min(args.restatement_genes, G)
    mine = {"groupSize": d_size.cpu().numpy().view(np.uint32), "nonZeroCount": d_count.cpu().numpy().view(np.uint32).reshape(G, kept)[:n],
            "rankSum2": d_sum.cpu().numpy().view(np.uint64).reshape(G, kept)[:n], "tieSum": d_tie.cpu().numpy().view(np.uint64)[:n]}
    host_toc, genes, values = synthetic.csr_to_host(toc, data)
    host = np.zeros(len(genes), dtype=capi.COUNT_DTYPE)
    host["gene"], host["count"] = genes, values
    theirs = rgb.load().rank_genes(host_toc, host, G, group, kept, norm.cpu().numpy(), 0, n)
    equal = all(np.array_equal(mine[name], theirs[name]) for name in rgb.INTEGERS)
    json.dump({"entries": entries, "groups": kept, "cells_in_a_group": int((group != NO_GROUP).sum()), "workspace_bytes": int(workspace_bytes),
               "restatement_genes": n, "restatement_seconds": theirs["seconds"], "equal": bool(equal)}, open(args.child_output, "w"))


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--cells", type=int, default=100000)
    parser.add_argument("--genes", type=int, default=30000)
    parser.add_argument("--density", type=float, default=0.01)
    parser.add_argument("--repeats", type=int, default=5)
    parser.add_argument("--restatement-genes", type=int, default=20)
    parser.add_argument("--limit", type=int, default=500, help="time limit of the GPU step in seconds")
    parser.add_argument("--output", default=None)
    parser.add_argument("--child-output", default=None)
    args = parser.parse_args()
    if args.child_output:
        return child(args)

    output = os.path.join(tempfile.mkdtemp(prefix="rank_genes_timing_"), "result.json")
    command = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--child-output", output] + \
              ["--%s=%s" % (name.replace("_", "-"), getattr(args, name)) for name in ("cells", "genes", "density", "repeats", "restatement_genes")]
    done = subprocess.run(command, capture_output=True, text=True)
    if done.returncode != 0:
        sys.stderr.write(done.stderr[-4000:])
        raise SystemExit("the GPU step ended with status %d: nothing more is started" % done.returncode)
    device = json.load(open(output))
    result = {"cells": args.cells, "genes": args.genes, "density": args.density, "normalization": "L2", "repeats": args.repeats,
              "stored_entries": device["entries"], "groups": device["groups"], "cells_in_a_group": device["cells_in_a_group"],
              "workspace_bytes": device["workspace_bytes"], "runs": "one run of this script: R calls in one process on one GPU"}
    E, G, Kg = device["entries"], args.genes, device["groups"]
    passes = int(np.ceil((32 + max(1, int(np.ceil(np.log2(G))))) / 8.))
    least = {"entries": 20. * E,                                          # the CSR once (8 B an entry), a key and a group out (12 B)
             "sort": 24. * E * passes,                                    # 12 B in and 12 B out per digit pass; ASSUMES 8 key bits per pass
             "searches, runs and chunk table": 28. * E,                   # head flags 8 + 4, the scan 4 + 4, the run starts 8
             "accumulate": 12. * E,                                       # group, flag and run number of every entry; the run starts are gathers
             "finish": 28. * G * Kg}
    for label, key in (("LDS counters", "lds"), ("global counters", "global")):
        section = done.stderr.split("[stages, %s]" % label)[1].split("[whole call")[0]
        stages = {}
        for name, value in re.findall(r"rankGenes: ([^\n]*?) ([0-9.]+) ms", section):
            stages.setdefault(re.sub(r"accumulate \(.*\)", "accumulate", name), []).append(float(value) / 1000.)
        whole = [float(v) / 1000. for v in re.findall(r"\[whole call, %s\] ([0-9.]+) ms" % label, done.stderr)]
        result[key] = {"whole_device_call_seconds": {"each": whole, "median": float(np.median(whole)), "best": min(whole)},
                       "stage_seconds_median_of_%d" % args.repeats: {name: float(np.median(v)) for name, v in stages.items()},
                       "stage_seconds_best": {name: min(v) for name, v in stages.items()}}
    best = result["lds"]["stage_seconds_best"]
    result["least_bytes"] = least
    result["sort_bytes_assume_8_key_bits_per_radix_pass"] = {"digit_passes": passes}
    result["seconds_at_6.29e12_bytes_per_second"] = {name: value / STREAMING for name, value in least.items()}
    result["achieved_share_of_6.29e12_lds_best"] = {name: least[name] / STREAMING / best[name] for name in least if best.get(name)}
    n = device["restatement_genes"]
    result["restatement_seconds_per_gene_first_%d_genes" % n] = device["restatement_seconds"] / n
    result["restatement_seconds_all_genes_EXTRAPOLATED"] = device["restatement_seconds"] / n * G
    result["first_genes_equal_the_restatement"] = device["equal"]
    line = json.dumps(result)
    print(line)
    if args.output:
        with open(args.output, "w") as out:
            out.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
