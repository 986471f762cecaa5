"""Timing of the multilevel layout (csrc/em2_layout.hip) next to the single-level pyramid run, on the cell graphs
of profiles/layout_timing.py (the bench's generator, threshold 0.2, at most 20 edges per vertex) at 10^5 and 10^6 cells:

    python profiles/layout_multilevel_timing.py [--vertices 100000 1000000] [--genes 30000] [--rounds 3] [--limit 900] [--output DIR]

Writes the record of every size to DIR/layout_multilevel_timing_<vertices>.json (DIR: this directory, next to the other
layout timings) and prints one JSON line with all of them.  Per size, in ONE process, whole runs with the default parameters of em2_dev_graph_layout_pyramid and of
em2_dev_graph_layout_multilevel at EM2_LAYOUT_DEPTH_AUTO alternate --rounds times: the seconds of every call, the best of each
and the ratio of every round on its own.  Then one multilevel run under the library's StageTimer (EM2_TIMING=1: a
synchronisation after the levels are built and after every level's iteration) for the milliseconds of the coarsening and of
each level, next to the level's vertex count, merged edges, matching rounds and iterations from em2_layout_levels.
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


def timed(vertices, d_v0, d_v1, edges, d_x, d_y, multilevel):
    """One call with the default parameters -> (seconds, iterations, step, energy, levels or None)."""
    from expressionmatrix2_amd import capi
    parameters = capi.LayoutParameters()
    result, levels = capi.LayoutResult(), capi.LayoutLevels()
    lib = capi.load()
    head = (vertices, d_v0.data_ptr(), d_v1.data_ptr(), edges, ctypes.byref(parameters), capi.LAYOUT_DEPTH_AUTO, d_x.data_ptr(),
            d_y.data_ptr(), ctypes.byref(result))
    begin = time.perf_counter()
    capi.check(lib.em2_dev_graph_layout_multilevel(*head, ctypes.byref(levels)) if multilevel else lib.em2_dev_graph_layout_pyramid(*head))
    seconds = time.perf_counter() - begin
    return seconds, result.iterationCount, result.step, result.energy, levels.as_list() if multilevel else None


def stage_milliseconds(call):
    """The library's stage lines of one call (they go to the C stderr) -> ({stage: milliseconds}, what the call returned)."""
    sys.stderr.flush()
    saved = os.dup(2)
    stages = {}
    with tempfile.TemporaryFile() as log:
        os.dup2(log.fileno(), 2)
        os.environ["EM2_TIMING"] = "1"
        try:
            returned = call()
        finally:
            del os.environ["EM2_TIMING"]
            os.dup2(saved, 2)
            os.close(saved)
        log.seek(0)
        for line in log.read().decode().splitlines():
            match = re.match(r"\[em2 timing\] graphLayoutMultilevel: (.+) ([0-9.]+) ms$", line)
            if match:
                stages[match.group(1)] = stages.get(match.group(1), 0.) + float(match.group(2))
    return stages, returned


def child(args):
    import torch
    from layout_timing import cell_graph
    n = args.child
    d_v0, d_v1, edges = cell_graph(n, args.genes)
    d_x = torch.zeros(n, dtype=torch.float32, device="cuda")
    d_y = torch.zeros(n, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()

    def run(multilevel):
        seconds, iterations, step, energy, levels = timed(n, d_v0, d_v1, edges, d_x, d_y, multilevel)
        return {"seconds": seconds, "iterations": iterations, "final_step": step, "final_energy": energy,
                "positions_finite": bool(np.all(np.isfinite(d_x.cpu().numpy())))}, levels

    for multilevel in (False, True):                                                   # warm-up: code objects, the scratch cache
        run(multilevel)
    rounds = []
    for _ in range(args.rounds):                                                       # pyramid, multilevel, pyramid, multilevel, ...
        entry = {"pyramid": run(False)[0], "multilevel": run(True)[0]}
        entry["multilevel_over_pyramid"] = entry["multilevel"]["seconds"] / entry["pyramid"]["seconds"]
        rounds.append(entry)
    best = {name: min(r[name]["seconds"] for r in rounds) for name in ("pyramid", "multilevel")}

    stages, (_, levels) = stage_milliseconds(lambda: run(True))
    per_level = [{"level": l, "vertices": v, "merged_edges": e, "matching_rounds": r, "iterations": i,
                  "milliseconds": stages.get("level %d" % l)} for l, (v, e, r, i) in enumerate(levels)]
    print(json.dumps({"vertices": n, "edges": edges, "rounds": rounds, "seconds_best": best,
                      "multilevel_over_pyramid_best": best["multilevel"] / best["pyramid"],
                      "coarsening_milliseconds": stages.get("levels"), "levels": per_level}))


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--vertices", type=int, nargs="+", default=[100000, 1000000])
    parser.add_argument("--genes", type=int, default=30000)
    parser.add_argument("--rounds", type=int, default=3)
    parser.add_argument("--limit", type=int, default=900, help="time limit of the GPU step of one size in seconds")
    parser.add_argument("--output", default=os.path.join(ROOT, "profiles"), help="the directory of the JSON files")
    parser.add_argument("--child", type=int, default=None)
    args = parser.parse_args()
    if args.child:
        return child(args)
    sizes = []
    for n in args.vertices:
        command = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--child", str(n), "--genes",
                   str(args.genes), "--rounds", str(args.rounds)]
        done = subprocess.run(command, capture_output=True, text=True)
        if done.returncode != 0:
            sys.stderr.write(done.stderr[-4000:])
            raise SystemExit("the GPU step of %d vertices ended with status %d: nothing more is started" % (n, done.returncode))
        sizes.append(json.loads(done.stdout.strip().splitlines()[-1]))
        with open(os.path.join(args.output, "layout_multilevel_timing_%d.json" % n), "w") as out:
            json.dump(sizes[-1], out, indent=1)
            out.write("\n")
    print(json.dumps({"sizes": sizes}))


if __name__ == "__main__":
    main()
