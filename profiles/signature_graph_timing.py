"""Timing of the signature graph (csrc/em2_signature_graph.hip) on the signatures of the bench's synthetic matrix
(expressionmatrix2_amd/synthetic.py: by default 1M cells x 30k genes, 24-bit signatures), through the device-pointer entries:

    python profiles/signature_graph_timing.py [--cells N] [--genes G] [--lsh-count 24] [--min-cell-count 1] [--repeats R]

Prints one JSON line: em2_dev_signature_graph_create (the whole call, R times, with the stage timing off; then R more calls
with EM2_TIMING=1, whose stages synchronise, for the stage split), em2_dev_lsh_signature_statistics, and the C++ restatement
(tests/native/em2_signature_graph_restatement.cpp: std::map, map::find per zero bit) on one thread of the same box, with the
ratios, and whether the two graphs are equal.  The GPU step runs in a child process under a time limit of its own; where it
fails nothing more is started."""
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


def child(args):
    """The GPU step: the signatures in HBM, R calls of each entry (stage lines on stderr), signatures and graph to a file."""
    import torch
    from expressionmatrix2_amd import capi, sharded, synthetic
    lib = capi.load()
    pipe = sharded.DevicePipeline(args.cells, args.genes, args.lsh_count, 1, 0.2, world_size=1, rank=0, dist=None, device="cuda")
    toc, data = synthetic.expression_shard(0, args.cells, args.genes, density=args.density)
    pipe.set_inputs(toc, data, torch.from_numpy(capi.lsh_generate_vectors(args.genes, args.lsh_count, 231)).to("cuda"))
    pipe.project()
    torch.cuda.synchronize()
    signatures = pipe.full_sig[:args.cells].contiguous()
    graph = None
    for timing in ("0", "1"):                             # (the library reads EM2_TIMING at every call)
        os.environ["EM2_TIMING"] = timing
        for _ in range(args.repeats):
            handle = ctypes.c_void_p(None)
            begin = time.perf_counter()
            capi.check(lib.em2_dev_signature_graph_create(signatures.data_ptr(), args.cells, args.lsh_count, args.min_cell_count,
                                                          ctypes.byref(handle)))
            if timing == "0":
                print("[whole call] %.3f ms" % (1000. * (time.perf_counter() - begin)), file=sys.stderr, flush=True)
            graph = capi.signature_graph_take(handle)
    os.environ["EM2_TIMING"] = "0"
    counts = np.zeros(args.lsh_count, dtype=np.uint64)
    for _ in range(args.repeats):
        begin = time.perf_counter()
        capi.check(lib.em2_dev_lsh_signature_statistics(signatures.data_ptr(), args.cells, args.lsh_count, capi._ptr(counts)))
        print("[statistics] %.3f ms" % (1000. * (time.perf_counter() - begin)), file=sys.stderr, flush=True)
    np.savez(args.child_output, signatures=signatures.cpu().numpy().view(np.uint64), counts=counts,
             distinct=graph["distinctCount"], **{key: graph[key] for key in ("vertexSignatures", "cellOffsets", "cells", "edgeVertex0", "edgeVertex1")})


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--cells", type=int, default=1000000)
    parser.add_argument("--genes", type=int, default=30000)
    parser.add_argument("--density", type=float, default=0.01)
    parser.add_argument("--lsh-count", type=int, default=24)
    parser.add_argument("--min-cell-count", type=int, default=1)
    parser.add_argument("--repeats", type=int, default=5)
    parser.add_argument("--limit", type=int, default=400, help="time limit of the GPU step in seconds")
    parser.add_argument("--child-output", default=None)
    args = parser.parse_args()
    if args.child_output:
        return child(args)

    output = os.path.join(tempfile.mkdtemp(prefix="signature_graph_timing_"), "result.npz")
    command = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--child-output", output] + \
              ["--%s=%s" % (name.replace("_", "-"), getattr(args, name)) for name in ("cells", "genes", "density", "lsh_count", "min_cell_count", "repeats")]
    done = subprocess.run(command, capture_output=True, text=True)
    if done.returncode != 0:
        sys.stderr.write(done.stderr[-4000:])
        raise SystemExit("the GPU step ended with status %d: nothing more is started" % done.returncode)
    stages = {}
    for name, value in re.findall(r"signatureGraph: ([^\n]*?) ([0-9.]+) ms", done.stderr):
        stages.setdefault(name, []).append(float(value) / 1000.)
    whole = [float(v) / 1000. for v in re.findall(r"\[whole call\] ([0-9.]+) ms", done.stderr)]
    statistics = [float(v) / 1000. for v in re.findall(r"\[statistics\] ([0-9.]+) ms", done.stderr)]
    device = np.load(output)

    import signature_graph_binding as sgb
    restatement = sgb.load()
    theirs = restatement.signature_graph(device["signatures"], args.lsh_count, args.min_cell_count)
    their_counts, their_statistics_seconds = restatement.signature_statistics(device["signatures"], args.lsh_count)
    equal = bool(theirs["distinctCount"] == int(device["distinct"]) and all(np.array_equal(theirs[key], device[key]) for key in sgb.GRAPH_KEYS)
                 and np.array_equal(their_counts, device["counts"]))
    print(json.dumps({
        "cells": args.cells, "genes": args.genes, "lsh_count": args.lsh_count, "min_cell_count": args.min_cell_count,
        "distinct_signatures": int(device["distinct"]), "vertices": int(len(device["cellOffsets"]) - 1), "edges": int(len(device["edgeVertex0"])),
        "device_graph_seconds_best_of_%d_stage_timing_off" % args.repeats: min(whole), "device_graph_seconds_all_in_call_order": whole,
        "device_stage_seconds_best_of_%d_later_calls_synchronised" % args.repeats: {name: min(values) for name, values in stages.items()},
        "device_statistics_seconds_best_of_%d" % args.repeats: min(statistics), "device_statistics_seconds_all": statistics,
        "restatement_graph_seconds_one_thread": theirs["seconds"], "restatement_statistics_seconds_one_thread": their_statistics_seconds,
        "graph_restatement_over_device": theirs["seconds"] / min(whole), "statistics_restatement_over_device": their_statistics_seconds / min(statistics),
        "device_equals_the_restatement": equal}))


if __name__ == "__main__":
    main()
