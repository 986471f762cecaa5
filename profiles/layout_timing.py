"""Timing of the graph layout (csrc/em2_layout.hip) on the cell graph of the bench's generator: synthetic
expression counts -> findSimilarPairs4 (k = 100) -> createCellGraph (threshold 0.2, at most 20 edges per vertex), as bench.py
--workload chain builds it, at 10^5 and at 10^6 cells:

    python profiles/layout_timing.py [--vertices 100000 1000000] [--genes 30000] [--repeats 3] [--limit 900]

Prints one JSON line.  Per size: one iteration (the difference of a run of 6 and a run of 1 iteration over 5, best of R each, so
that the check of the edges, the adjacency and the copies are not in it), the pairs per second that makes (N^2 pair evaluations
per iteration), its share of the hand-derived issue bound of the repulsion loop, and a whole run with the
default parameters.  Then the restatement (tests/native/em2_layout_restatement.cpp) on one thread of the same box: its time per
pair measured at --restatement-vertices and EXTRAPOLATED to the sizes above as pairs x that time (labelled so).
One process uses the GPU at a time: each size is a child process under a time limit of its own, one after the other; where one
fails nothing more is started."""
import argparse
import ctypes
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

# The issue bound of the repulsion loop, from the listing of the full-tile loop (8 pairs per trip): per pair 16 vector
# instructions -- v_pk_add_f32 (both differences), v_mul_f32 + v_fmac_f32 (d^2), v_max_f32, the correctly rounded divide
# (2 v_div_scale_f32, v_rcp_f32, 6 v_fma / v_fmac / v_mul_f32, v_div_fmas_f32, v_div_fixup_f32 = 11), v_pk_fma_f32 (both
# accumulations).  At one issue slot of 4 cycles each, and two for v_rcp_f32, that is 17 slots for 64 pairs on each of the
# 1024 SIMDs at 2.4 GHz.  (The measured rate is ABOVE this bound: see DESIGN.md 3.19 for what that says about the count.)
VECTOR_INSTRUCTIONS_PER_PAIR = 16
ISSUE_SLOTS_PER_PAIR = 17
SIMDS, LANES, CYCLES_PER_SLOT, CLOCK_HZ = 1024, 64, 4, 2.4e9
BOUND_PAIRS_PER_SECOND = SIMDS * LANES * CLOCK_HZ / (ISSUE_SLOTS_PER_PAIR * CYCLES_PER_SLOT)


def cell_graph(vertices, genes, graph_k=20, lsh_count=1024, k=100, threshold=0.2, seed=231):
    """The edges of bench.py's chain workload, in device memory -> (d_v0, d_v1, edge count)."""
    import torch
    from expressionmatrix2_amd import capi, sharded, synthetic
    device = torch.device("cuda")
    pipe = sharded.DevicePipeline(vertices, genes, lsh_count, k, threshold, world_size=1, rank=0, dist=None, device=device)
    toc, data = synthetic.expression_shard(0, vertices, genes, density=0.01, device=device)
    pipe.set_inputs(toc, data, torch.from_numpy(capi.lsh_generate_vectors(genes, lsh_count, seed)).to(device))
    pipe.step()
    pipe.check()
    torch.cuda.synchronize()
    cells = np.arange(vertices, dtype=np.uint32)
    d_v0 = torch.empty(vertices * graph_k, dtype=torch.int32, device=device)
    d_v1 = torch.empty(vertices * graph_k, dtype=torch.int32, device=device)
    d_similarity = torch.empty(vertices * graph_k, dtype=torch.float32, device=device)
    edges = capi.dev_cell_graph_edges_to_device(pipe.pairs.data_ptr(), pipe.used.data_ptr(), vertices, k, cells, cells, threshold, graph_k,
                                                d_v0.data_ptr(), d_v1.data_ptr(), d_similarity.data_ptr())
    return d_v0, d_v1, edges


def timed_layout(vertices, d_v0, d_v1, edges, d_x, d_y, **changes):
    """One em2_dev_graph_layout call (it returns when the positions are written) -> (seconds, iterations, step, energy)."""
    from expressionmatrix2_amd import capi
    parameters = capi.LayoutParameters(**changes)
    result = capi.LayoutResult()
    begin = time.perf_counter()
    capi.check(capi.load().em2_dev_graph_layout(vertices, d_v0.data_ptr(), d_v1.data_ptr(), edges, ctypes.byref(parameters),
                                                d_x.data_ptr(), d_y.data_ptr(), ctypes.byref(result)))
    return time.perf_counter() - begin, result.iterationCount, result.step, result.energy


def child(args):
    """The GPU step of one size; a JSON line on stdout."""
    import torch
    n = args.child
    d_v0, d_v1, edges = cell_graph(n, args.genes)
    d_x = torch.zeros(n, dtype=torch.float32, device="cuda")
    d_y = torch.zeros(n, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    timed_layout(n, d_v0, d_v1, edges, d_x, d_y, maxIterationCount=2)               # warm-up: code objects, the scratch cache
    one = [timed_layout(n, d_v0, d_v1, edges, d_x, d_y, maxIterationCount=1)[0] for _ in range(args.repeats)]
    six = [timed_layout(n, d_v0, d_v1, edges, d_x, d_y, maxIterationCount=6)[0] for _ in range(args.repeats)]
    seconds, iterations, step, energy = timed_layout(n, d_v0, d_v1, edges, d_x, d_y)
    x = d_x.cpu().numpy()
    iteration = (min(six) - min(one)) / 5.
    print(json.dumps({
        "vertices": n, "edges": edges, "pairs_per_iteration": n * n,
        "call_of_1_iteration_seconds_all": one, "call_of_6_iterations_seconds_all": six,
        "iteration_seconds": iteration, "pairs_per_second": n * n / iteration,
        "issue_bound_pairs_per_second": BOUND_PAIRS_PER_SECOND, "share_of_issue_bound": n * n / iteration / BOUND_PAIRS_PER_SECOND,
        "issue_slots_per_pair_counted": ISSUE_SLOTS_PER_PAIR,
        "issue_slots_per_pair_the_rate_amounts_to": SIMDS * LANES * CLOCK_HZ / CYCLES_PER_SLOT / (n * n / iteration),
        "whole_run_default_parameters": {"seconds": seconds, "iterations": iterations, "final_step": step, "final_energy": energy,
                                         "positions_finite": bool(np.all(np.isfinite(x)))}}))


def restatement_seconds_per_pair(vertices):
    import layout_binding as lb
    n, edges = lb.random_graph(vertices, 20, 1)
    restatement = lb.load()
    x, y = restatement.initial(n, 231)
    best = None
    for _ in range(3):
        begin = time.perf_counter()
        restatement.forces(n, edges, 0.02, x, y)
        seconds = time.perf_counter() - begin
        best = seconds if best is None else min(best, seconds)
    return best / (n * n)


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--vertices", type=int, nargs="+", default=[100000, 1000000])
    parser.add_argument("--genes", type=int, default=30000)
    parser.add_argument("--repeats", type=int, default=3)
    parser.add_argument("--limit", type=int, default=900, help="time limit of the GPU step of one size in seconds")
    parser.add_argument("--restatement-vertices", type=int, default=8192)
    parser.add_argument("--child", type=int, default=None)
    args = parser.parse_args()
    if args.child:
        return child(args)

    sizes = []
    for n in args.vertices:
        command = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--child", str(n),
                   "--genes", str(args.genes), "--repeats", str(args.repeats)]
        done = subprocess.run(command, capture_output=True, text=True)
        if done.returncode != 0:
            sys.stderr.write(done.stderr[-4000:])
            raise SystemExit("the GPU step of %d vertices ended with status %d: nothing more is started" % (n, done.returncode))
        sizes.append(json.loads(done.stdout.strip().splitlines()[-1]))
    per_pair = restatement_seconds_per_pair(args.restatement_vertices)
    for size in sizes:
        size["restatement_iteration_seconds_one_thread_EXTRAPOLATED_from_%d_vertices" % args.restatement_vertices] = \
            per_pair * size["pairs_per_iteration"]
        size["restatement_EXTRAPOLATED_over_device_iteration"] = per_pair * size["pairs_per_iteration"] / size["iteration_seconds"]
    print(json.dumps({"sizes": sizes, "restatement_seconds_per_pair_one_thread_measured_at_%d_vertices" % args.restatement_vertices: per_pair}))


if __name__ == "__main__":
    main()
