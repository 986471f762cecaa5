"""Timing of the gene graph (csrc/em2_gene_graph.hip) on synthetic stored lists (by default 30 000 genes x k = 100, the graph's
gene set equal to the pairs'), through the host entry and the device-pointer entry:

    python profiles/gene_graph_timing.py [--genes N] [--k K] [--limit-per-gene 20] [--threshold 0.3] [--repeats R]

Prints one JSON line: em2_gene_graph_create and em2_dev_gene_graph_create (the whole call, R times each, with the stage timing
off; then R more device-entry calls with EM2_TIMING=1, whose stages synchronise, for the stage split) and the C++ restatement
(tests/native/em2_gene_graph_restatement.cpp: std::map, std::set, std::list) on one thread of the same box, with the ratios, and
whether the two graphs are equal.  The GPU step runs in a child process under a time limit of its own; where it fails nothing
more is started."""
import argparse
import ctypes
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

PAIR_DTYPE = np.dtype([("cell", "<u4"), ("similarity", "<f4")])


def stored_lists(genes, k, seed=1):
    """k distinct partners per gene within the 20 k genes behind it (so that the two ends of a pair often store each other),
    in random order; similarities uniform in (0, 1), descending; one gene in 50 stores fewer than k."""
    rng = np.random.default_rng(seed)
    assert genes > 20 * k
    offsets = np.cumsum(rng.integers(1, 20, (genes, k)), axis=1)
    sign = rng.integers(0, 2, (genes, 1)) * 2 - 1
    partners = (np.arange(genes)[:, None] + sign * rng.permuted(offsets, axis=1)) % genes
    pairs = np.zeros((genes, k), dtype=PAIR_DTYPE)
    pairs["cell"] = partners
    pairs["similarity"] = -np.sort(-rng.random((genes, k), dtype=np.float32), axis=1)
    used = np.full(genes, k, dtype=np.uint32)
    short = rng.random(genes) < 0.02
    used[short] = rng.integers(0, k, short.sum())
    return pairs, used


def child(args):
    """The GPU step: R calls of each entry (stage lines on stderr), the graph to a file."""
    import torch
    from expressionmatrix2_amd import capi
    lib = capi.load()
    pairs, used = stored_lists(args.genes, args.k)
    ids = np.arange(args.genes, dtype=np.uint32)
    d_pairs = torch.from_numpy(pairs.view(np.int64).reshape(-1).copy()).to("cuda")
    d_used = torch.from_numpy(used.view(np.int32).copy()).to("cuda")
    torch.cuda.synchronize()
    graph = None
    for label, entry, p, u in (("host entry", lib.em2_gene_graph_create, capi._ptr(pairs), capi._ptr(used)),
                               ("device entry", lib.em2_dev_gene_graph_create, d_pairs.data_ptr(), d_used.data_ptr()),
                               ("stages", lib.em2_dev_gene_graph_create, d_pairs.data_ptr(), d_used.data_ptr())):
        os.environ["EM2_TIMING"] = "1" if label == "stages" else "0"          # (the library reads EM2_TIMING at every call)
        for _ in range(args.repeats):
            handle = ctypes.c_void_p(None)
            begin = time.perf_counter()
            capi.check(entry(p, u, args.genes, args.k, capi._ptr(ids), capi._ptr(ids), args.genes, args.threshold, args.limit_per_gene,
                             ctypes.byref(handle)))
            if label != "stages":
                print("[%s] %.3f ms" % (label, 1000. * (time.perf_counter() - begin)), file=sys.stderr, flush=True)
            graph = capi.gene_graph_take(handle)
    np.savez(args.child_output, removed=graph["removedCount"], **{key: graph[key] for key in capi.GENE_GRAPH_KEYS})


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--genes", type=int, default=30000)
    parser.add_argument("--k", type=int, default=100)
    parser.add_argument("--limit-per-gene", type=int, default=20, help="maxConnectivity")
    parser.add_argument("--threshold", type=float, default=0.3)
    parser.add_argument("--repeats", type=int, default=5)
    parser.add_argument("--limit", type=int, default=300, help="time limit of the GPU step in seconds")
    parser.add_argument("--child-output", default=None)
    args = parser.parse_args()
    if args.child_output:
        return child(args)

    output = os.path.join(tempfile.mkdtemp(prefix="gene_graph_timing_"), "result.npz")
    command = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--child-output", output] + \
              ["--%s=%s" % (name.replace("_", "-"), getattr(args, name)) for name in ("genes", "k", "limit_per_gene", "threshold", "repeats")]
    done = subprocess.run(command, capture_output=True, text=True)
    if done.returncode != 0:
        sys.stderr.write(done.stderr[-4000:])
        raise SystemExit("the GPU step ended with status %d: nothing more is started" % done.returncode)
    stages = {}
    for name, value in re.findall(r"geneGraph: ([^\n]*?) ([0-9.]+) ms", done.stderr):
        stages.setdefault(name, []).append(float(value) / 1000.)
    host = [float(v) / 1000. for v in re.findall(r"\[host entry\] ([0-9.]+) ms", done.stderr)]
    device_entry = [float(v) / 1000. for v in re.findall(r"\[device entry\] ([0-9.]+) ms", done.stderr)]
    device = np.load(output)

    import gene_graph_binding as ggb
    pairs, used = stored_lists(args.genes, args.k)
    ids = np.arange(args.genes, dtype=np.uint32)
    theirs = ggb.load().gene_graph(pairs, used, ids, ids, args.threshold, args.limit_per_gene)
    mine = {key: device[key] for key in ggb.GRAPH_KEYS}
    equal = bool(int(device["removed"]) == theirs["removedCount"] and all(
        mine[key].shape == theirs[key].shape and np.array_equal(mine[key].view(np.uint32) if mine[key].dtype == np.float32 else mine[key],
                                                                theirs[key].view(np.uint32) if theirs[key].dtype == np.float32 else theirs[key])
        for key in ggb.GRAPH_KEYS))
    print(json.dumps({
        "genes": args.genes, "k": args.k, "max_connectivity": args.limit_per_gene, "threshold": args.threshold,
        "vertices": int(len(mine["vertices"])), "edges": int(len(mine["edgeGene0"])), "removed": int(device["removed"]),
        "host_entry_seconds_best_of_%d" % args.repeats: min(host), "host_entry_seconds_all_in_call_order": host,
        "device_entry_seconds_best_of_%d" % args.repeats: min(device_entry), "device_entry_seconds_all_in_call_order": device_entry,
        "device_stage_seconds_best_of_%d_later_calls_synchronised" % args.repeats: {name: min(values) for name, values in stages.items()},
        "restatement_seconds_one_thread": theirs["seconds"],
        "restatement_over_host_entry": theirs["seconds"] / min(host), "restatement_over_device_entry": theirs["seconds"] / min(device_entry),
        "device_equals_the_restatement": equal}))


if __name__ == "__main__":
    main()
