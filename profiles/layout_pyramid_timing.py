"""Timing of the layout with the pyramid's far field (csrc/em2_layout.hip) next to the exact one, on the cell
graphs of profiles/layout_timing.py (the bench's generator, threshold 0.2, at most 20 edges per vertex) at 10^5 and 10^6 cells:

    python profiles/layout_pyramid_timing.py [--vertices 100000 1000000] [--genes 30000] [--rounds 3] [--limit 900] [--no-whole-exact]

Prints one JSON line.  Per size, in ONE process, the exact and the pyramid entry alternate --rounds times; one iteration = (a
call of 6 iterations - a call of 1) / 5, the best of the rounds each, and the ratio of every round on its own.  Then the same
for the forced depths around the automatic one -- which is how the leaf targets 4, 8, 16 and 32 differ: each is a depth at a
given vertex count --, the stages of an evaluation from the library's StageTimer (EM2_TIMING=1: a synchronisation after every
stage, so their sum is above the iteration measured without it), and whole runs with the default parameters.
One process uses the GPU at a time: each size is a child process under a time limit of its own; where one fails nothing more is
started."""
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
sys.path.insert(0, os.path.join(ROOT, "profiles"))

LEAF_TARGETS = (4, 8, 16, 32)
MAX_DEPTH = 10
STAGES = ("box", "keys and sort", "pyramid", "walk", "force")


def depth_of(leaf_target, vertices):
    for depth in range(MAX_DEPTH):
        if leaf_target * 4 ** depth >= vertices:
            return depth
    return MAX_DEPTH


def timed(vertices, d_v0, d_v1, edges, d_x, d_y, depth, **changes):
    """One call of em2_dev_graph_layout (depth None) or em2_dev_graph_layout_pyramid -> (seconds, iterations, step, energy)."""
    from expressionmatrix2_amd import capi
    parameters = capi.LayoutParameters(**changes)
    result = capi.LayoutResult()
    lib = capi.load()
    head = (vertices, d_v0.data_ptr(), d_v1.data_ptr(), edges, ctypes.byref(parameters))
    tail = (d_x.data_ptr(), d_y.data_ptr(), ctypes.byref(result))
    begin = time.perf_counter()
    capi.check(lib.em2_dev_graph_layout(*head, *tail) if depth is None else lib.em2_dev_graph_layout_pyramid(*head, depth, *tail))
    return time.perf_counter() - begin, result.iterationCount, result.step, result.energy


def stage_milliseconds(call):
    """The library's stage lines of one call (they go to the C stderr) -> {stage: the sum of its milliseconds}."""
    sys.stderr.flush()
    saved = os.dup(2)
    totals = {}
    with tempfile.TemporaryFile() as log:
        os.dup2(log.fileno(), 2)
        os.environ["EM2_TIMING"] = "1"
        try:
            call()
        finally:
            del os.environ["EM2_TIMING"]
            os.dup2(saved, 2)
            os.close(saved)
        log.seek(0)
        for line in log.read().decode().splitlines():
            match = re.match(r"\[em2 timing\] graphLayout: (.+) ([0-9.]+) ms$", line)
            if match:
                totals[match.group(1)] = totals.get(match.group(1), 0.) + float(match.group(2))
    return totals


def child(args):
    import torch
    from layout_timing import cell_graph
    from expressionmatrix2_amd import capi
    n = args.child
    d_v0, d_v1, edges = cell_graph(n, args.genes)
    d_x = torch.zeros(n, dtype=torch.float32, device="cuda")
    d_y = torch.zeros(n, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    auto = depth_of(capi.LAYOUT_LEAF_TARGET, n)

    def seconds(depth, iterations):
        return timed(n, d_v0, d_v1, edges, d_x, d_y, depth, maxIterationCount=iterations)[0]

    for depth in (None, capi.LAYOUT_DEPTH_AUTO):                                       # warm-up: code objects, the scratch cache
        seconds(depth, 2)
    rounds = []
    for _ in range(args.rounds):                                                       # exact, pyramid, exact, pyramid, ...
        entry = {}
        for name, depth in (("exact", None), ("pyramid", capi.LAYOUT_DEPTH_AUTO)):
            entry[name] = {"call_of_1": seconds(depth, 1), "call_of_6": seconds(depth, 6)}
            entry[name]["iteration_seconds"] = (entry[name]["call_of_6"] - entry[name]["call_of_1"]) / 5.
        entry["exact_over_pyramid"] = entry["exact"]["iteration_seconds"] / entry["pyramid"]["iteration_seconds"]
        rounds.append(entry)
    best = {name: (min(r[name]["call_of_6"] for r in rounds) - min(r[name]["call_of_1"] for r in rounds)) / 5. for name in ("exact", "pyramid")}

    depths = {}
    for depth in sorted({depth_of(target, n) for target in LEAF_TARGETS} | {max(auto - 1, 0), min(auto + 1, MAX_DEPTH)}):
        seconds(depth, 2)
        ones = [seconds(depth, 1) for _ in range(args.rounds)]
        sixes = [seconds(depth, 6) for _ in range(args.rounds)]
        depths[depth] = {"iteration_seconds": (min(sixes) - min(ones)) / 5., "call_of_1_all": ones, "call_of_6_all": sixes}
    targets = {target: {"depth": depth_of(target, n), "iteration_seconds": depths[depth_of(target, n)]["iteration_seconds"]}
               for target in LEAF_TARGETS}

    stages = stage_milliseconds(lambda: seconds(capi.LAYOUT_DEPTH_AUTO, 6))
    per_evaluation = {name: stages.get(name, 0.) / 6. for name in STAGES}

    whole = {}
    for name, depth in (("pyramid", capi.LAYOUT_DEPTH_AUTO),) + ((("exact", None),) if args.whole_exact else ()):
        s, iterations, step, energy = timed(n, d_v0, d_v1, edges, d_x, d_y, depth)
        whole[name] = {"seconds": s, "iterations": iterations, "final_step": step, "final_energy": energy,
                       "positions_finite": bool(np.all(np.isfinite(d_x.cpu().numpy())))}
    print(json.dumps({"vertices": n, "edges": edges, "automatic_depth": auto, "leaf_target": capi.LAYOUT_LEAF_TARGET, "rounds": rounds,
                      "iteration_seconds_best": best, "exact_over_pyramid_best": best["exact"] / best["pyramid"],
                      "forced_depths": depths, "leaf_targets": targets,
                      "stage_milliseconds_per_evaluation_with_a_synchronisation_each": per_evaluation,
                      "whole_run_default_parameters": whole}))


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--vertices", type=int, nargs="+", default=[100000, 1000000])
    parser.add_argument("--genes", type=int, default=30000)
    parser.add_argument("--rounds", type=int, default=3)
    parser.add_argument("--limit", type=int, default=900, help="time limit of the GPU step of one size in seconds")
    parser.add_argument("--no-whole-exact", dest="whole_exact", action="store_false",
                        help="leave out the whole default run of the exact entry (two minutes at 10^6 vertices)")
    parser.add_argument("--child", type=int, default=None)
    args = parser.parse_args()
    if args.child:
        return child(args)
    sizes = []
    for n in args.vertices:
        command = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--child", str(n), "--genes",
                   str(args.genes), "--rounds", str(args.rounds)] + ([] if args.whole_exact else ["--no-whole-exact"])
        done = subprocess.run(command, capture_output=True, text=True)
        if done.returncode != 0:
            sys.stderr.write(done.stderr[-4000:])
            raise SystemExit("the GPU step of %d vertices ended with status %d: nothing more is started" % (n, done.returncode))
        sizes.append(json.loads(done.stdout.strip().splitlines()[-1]))
    print(json.dumps({"sizes": sizes}))


if __name__ == "__main__":
    main()
