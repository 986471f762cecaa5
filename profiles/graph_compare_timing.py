"""Timing of compareCellGraphs and of the group colouring (csrc/em2_graph_compare.hip) at the size the chain runs:

    python profiles/graph_compare_timing.py [--cells N] [--repeats R] [--output profiles/graph_compare_timing_<cells>.json]

Workload: N cells of bench.py's scan-only generator (synthetic_signatures: 64 cluster centres, every bit flipped with
probability 0.15), findSimilarPairs4 with k = 100 at threshold 0.2 on the device, and from those pairs two cell graphs of the
same cells with the edges left in device memory: graph 0 at threshold 0.2 and k = 20 (the chain's), graph 1 at threshold 0.6
and k = 15, so that a share of the edges is common and the common ones carry identical similarities.  The group colouring takes
the label-propagation clusters of graph 0 as groups.

One process, after one warm-up call of each: the host entry and the em2_dev_ entry alternated R times (whole calls, stage timing
off), then R more device-entry calls with EM2_TIMING=1, whose stages synchronise, for the stage split.  The C++ restatement
(tests/native/em2_graph_compare_restatement.cpp: two std::map, a std::map<float, size_t>, std::set_intersection; std::set
adjacency) runs on one thread of the same box on the same arrays, and every result is compared with it.  Next to the stage times
stand the bytes a stage has to move and the time they take at the 6.29 TB/s this project measures as its streaming rate
(DESIGN.md 3.15).  The GPU step runs in a child process under a time limit of its own; where it fails nothing more is started."""
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

LSH, K, THRESHOLD = 1024, 100, 0.2
GRAPHS = ((0.2, 20), (0.6, 15))
STREAMING = 6.29e12


def child(args):
    import torch
    import bench
    from expressionmatrix2_amd import capi
    device = torch.device("cuda")
    C = args.cells
    cells = np.arange(C, dtype=np.uint32)
    stream = torch.cuda.current_stream().cuda_stream
    sig = bench.synthetic_signatures(torch, C, LSH, device)
    pairs = torch.zeros((C, K, 2), dtype=torch.int32, device=device)
    used = torch.zeros(C, dtype=torch.int32, device=device)
    ws_bytes = capi.dev_find_similar_pairs4_workspace(C, C, LSH, K)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=device)
    capi.dev_find_similar_pairs4(sig.data_ptr(), C, 0, C, LSH, K, THRESHOLD, pairs.data_ptr(), used.data_ptr(), ws.data_ptr(), ws_bytes, stream)
    capi.dev_find_similar_pairs4_status(ws.data_ptr(), C, K, stream)
    del ws, sig
    graphs = []
    for threshold, k in GRAPHS:
        v0 = torch.empty(C * k, dtype=torch.int32, device=device)
        v1 = torch.empty(C * k, dtype=torch.int32, device=device)
        sim = torch.empty(C * k, dtype=torch.float32, device=device)
        edges = capi.dev_cell_graph_edges_to_device(pairs.data_ptr(), used.data_ptr(), C, K, cells, cells, threshold, k,
                                                    v0.data_ptr(), v1.data_ptr(), sim.data_ptr())
        graphs.append((v0, v1, sim, edges))
    clusters, _ = capi.dev_cell_graph_label_propagation(cells, graphs[0][0].data_ptr(), graphs[0][1].data_ptr(), graphs[0][2].data_ptr(),
                                                        graphs[0][3])
    host = [(cells, g[0][:g[3]].cpu().numpy().view(np.uint32), g[1][:g[3]].cpu().numpy().view(np.uint32), g[2][:g[3]].cpu().numpy())
            for g in graphs]
    device_arguments = [x for g in graphs for x in (cells, g[0].data_ptr(), g[1].data_ptr(), g[2].data_ptr(), g[3])]

    def timed(label, call):
        torch.cuda.synchronize()
        begin = time.perf_counter()
        result = call()
        print("[%s] %.3f ms" % (label, 1000. * (time.perf_counter() - begin)), file=sys.stderr, flush=True)
        return result

    os.environ["EM2_TIMING"] = "0"                                    # (the library reads EM2_TIMING at every call)
    capi.cell_graph_compare(host[0], host[1])
    capi.dev_cell_graph_compare(*device_arguments)
    capi.graph_group_colors(clusters, host[0][1], host[0][2])
    for _ in range(args.repeats):
        timed("compare host entry", lambda: capi.cell_graph_compare(host[0], host[1]))
        comparison = timed("compare device entry", lambda: capi.dev_cell_graph_compare(*device_arguments))
        timed("colors host entry", lambda: capi.graph_group_colors(clusters, host[0][1], host[0][2]))
        colors = timed("colors device entry", lambda: capi.dev_graph_group_colors(clusters, graphs[0][0].data_ptr(), graphs[0][1].data_ptr(),
                                                                                 graphs[0][3]))
    listed = timed("compare device entry, list path", lambda: capi.dev_cell_graph_compare(*device_arguments, capi.GRAPH_COMPARE_LIST))
    os.environ["EM2_TIMING"] = "1"
    for _ in range(args.repeats):
        capi.dev_cell_graph_compare(*device_arguments)
    os.environ["EM2_TIMING"] = "0"
    np.savez(args.child_output, clusters=clusters, listBinDelta=listed["binDelta"], listBinCount=listed["binCount"],
             **{"g%d_%s" % (which, name): array for which, g in enumerate(host) for name, array in zip(("v0", "v1", "sim"), g[1:])},
             **{"compare_" + key: value for key, value in comparison.items()}, **{"colors_" + key: value for key, value in colors.items()})


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--cells", type=int, default=100000)
    parser.add_argument("--repeats", type=int, default=5)
    parser.add_argument("--limit", type=int, default=400, help="time limit of the GPU step in seconds")
    parser.add_argument("--output", default=None)
    parser.add_argument("--child-output", default=None)
    args = parser.parse_args()
    if args.child_output:
        return child(args)

    output = os.path.join(tempfile.mkdtemp(prefix="graph_compare_timing_"), "result.npz")
    command = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--child-output", output,
               "--cells=%d" % args.cells, "--repeats=%d" % args.repeats]
    done = subprocess.run(command, capture_output=True, text=True)
    if done.returncode != 0:
        sys.stderr.write(done.stderr[-4000:])
        raise SystemExit("the GPU step ended with status %d: nothing more is started" % done.returncode)
    stages = {}
    for name, value in re.findall(r"compareCellGraphs: ([^\n]*?) ([0-9.]+) ms", done.stderr):
        stages.setdefault(name, []).append(float(value) / 1000.)
    calls = {}
    for name, value in re.findall(r"\[([a-z, ]+)\] ([0-9.]+) ms", done.stderr):
        calls.setdefault(name, []).append(float(value) / 1000.)
    device = np.load(output)

    import graph_compare_binding as gb
    cells = np.arange(args.cells, dtype=np.uint32)
    host = [(cells, device["g%d_v0" % which], device["g%d_v1" % which], device["g%d_sim" % which]) for which in range(2)]
    restatement = gb.load()
    begin = time.perf_counter()
    status, reference = restatement.compare(host[0], host[1])
    compare_seconds = time.perf_counter() - begin
    begin = time.perf_counter()
    color_status, reference_colors = restatement.group_colors(device["clusters"], host[0][1], host[0][2])
    color_seconds = time.perf_counter() - begin
    assert status == gb.OK and color_status == gb.OK
    mine = {key: (device["compare_" + key] if key.startswith("bin") else int(device["compare_" + key])) for key in gb.COUNT_KEYS + ("binDelta", "binCount")}
    equal = all(mine[key] == reference[key] for key in gb.COUNT_KEYS) and \
        all(np.array_equal(gb.bits(a), gb.bits(reference["binDelta"])) and np.array_equal(b, reference["binCount"])
            for a, b in ((mine["binDelta"], mine["binCount"]), (device["listBinDelta"], device["listBinCount"])))
    colors_equal = int(device["colors_groupCount"]) == reference_colors["groupCount"] and all(
        np.array_equal(device["colors_" + key], reference_colors[key]) for key in ("pairGroup0", "pairGroup1", "pairEdgeCount", "colorTable"))

    edges = [len(g[1]) for g in host]
    distinct = [mine["edgeCount0"], mine["edgeCount1"]]
    # what a stage has to move once: the keys kernel reads 12 bytes per edge, gathers two cell ids and writes 12; a sort reads and
    # writes its 12-byte records once at the least (a radix sort does so once per digit pass); the join reads both lists of
    # distinct (key, similarity) records once
    must_move = {"keys": 32 * sum(edges), "sort": 24 * sum(edges), "join and histogram": 12 * sum(distinct)}
    best = {name: min(values) for name, values in stages.items()}
    summed = {}                                                     # "keys", "sort", "distinct keys" occur once per graph and call
    for name, values in stages.items():
        per_call = len(values) // args.repeats
        summed[name] = min(sum(values[at * per_call:(at + 1) * per_call]) for at in range(args.repeats))
    result = {
        "cells": args.cells, "lsh_count": LSH, "similar_pairs_k": K, "similar_pairs_threshold": THRESHOLD,
        "graphs_threshold_and_k": GRAPHS, "input_edges": edges, "distinct_edges": distinct,
        "common_edges": mine["commonEdgeCount"], "common_identical_edges": mine["commonIdenticalEdgeCount"],
        "common_vertices": mine["commonVertexCount"], "bins": int(len(mine["binCount"])),
        "groups": int(device["colors_groupCount"]), "group_pairs": int(len(device["colors_pairGroup0"])),
        "colors_used": int(device["colors_colorTable"].max()) + 1 if len(device["colors_colorTable"]) else 0,
        "seconds_all_in_call_order": calls, "seconds_best_of_%d" % args.repeats: {name: min(values) for name, values in calls.items()},
        "device_entry_stage_seconds_per_call_best_of_%d_later_calls_synchronised" % args.repeats: summed,
        "single_stage_seconds_best": best,
        "bytes_a_stage_must_move": must_move,
        "seconds_for_those_bytes_at_6.29_TB_per_s": {name: value / STREAMING for name, value in must_move.items()},
        "stage_over_streaming_time": {name: summed[name] / (value / STREAMING) for name, value in must_move.items() if name in summed},
        "restatement_seconds_one_thread": {"compare": compare_seconds, "colors": color_seconds},
        "restatement_over_device_entry": {"compare": compare_seconds / min(calls["compare device entry"]),
                                          "colors": color_seconds / min(calls["colors device entry"])},
        "restatement_over_host_entry": {"compare": compare_seconds / min(calls["compare host entry"]),
                                        "colors": color_seconds / min(calls["colors host entry"])},
        "device_equals_the_restatement": {"compare_both_paths": bool(equal), "colors": bool(colors_equal)},
    }
    text = json.dumps(result)
    print(text)
    if args.output:
        with open(args.output, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
