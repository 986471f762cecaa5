"""Timing of the dense read-out (csrc/em2_dense.hip) on the bench's synthetic matrix (expressionmatrix2_amd/synthetic.py), by
default 10^6 cells x 2 000 genes, L2 normalisation, both element types, through the device-pointer entry:

    python profiles/dense_expression_timing.py [--cells N] [--genes G] [--density D] [--repeats 5] [--restatement-rows 10000]

Prints one JSON line: the stage times of EM2_TIMING=1 (best and all of R calls), the fill against the roofline of a streaming
write (bytes written / 6.29 TB/s, the float4 copy rate of the MI355X), the time torch takes to zero the same buffer (the floor of
the alternative "memset, then scatter"), and the C++ restatement on one thread for the first rows, which the device's rows are
compared with.  The GPU step runs in a child process under a time limit of its own; where it fails nothing more is started."""
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

ROOFLINE_BYTES_PER_SECOND = 6.29e12


def child(args):
    """The GPU step: the matrix in HBM, R calls per element type (stage lines on stderr), the first rows to a file."""
    import torch
    from expressionmatrix2_amd import capi, synthetic
    capi.load()
    toc, data = synthetic.expression_shard(0, args.cells, args.genes, density=args.density)
    kept = {}
    for name, dtype in (("float64", torch.float64), ("float32", torch.float32)):
        out = torch.empty(args.cells * args.genes, dtype=dtype, device="cuda")
        workspace = torch.empty(capi.load().em2_dev_dense_expression_workspace(args.cells), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        for _ in range(args.repeats):
            print("[element type] %s" % name, file=sys.stderr, flush=True)
            begin = time.time()
            capi.dev_dense_expression(toc, data, args.cells, args.genes, 2, out, d_workspace=workspace)
            print("[whole call] %s %.3f ms" % (name, 1000. * (time.time() - begin)), file=sys.stderr, flush=True)
        kept[name] = out[:args.restatement_rows * args.genes].cpu().numpy()
        for _ in range(args.repeats):
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            out.zero_()
            stop.record()
            torch.cuda.synchronize()
            print("[zero] %s %.3f ms" % (name, start.elapsed_time(stop)), file=sys.stderr, flush=True)
        del out
    rows = args.restatement_rows
    host_toc, genes, values = synthetic.csr_to_host(toc[:rows + 1], data[:int(toc[rows].item())])
    host = np.zeros(len(genes), dtype=capi.COUNT_DTYPE)
    host["gene"], host["count"] = genes, values
    np.savez(args.child_output, toc=host_toc, data=host, entries=int(data.numel()), **kept)


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--cells", type=int, default=1000000)
    parser.add_argument("--genes", type=int, default=2000)
    parser.add_argument("--density", type=float, default=0.01)
    parser.add_argument("--repeats", type=int, default=5)
    parser.add_argument("--restatement-rows", type=int, default=10000)
    parser.add_argument("--limit", type=int, default=300, help="time limit of the GPU step in seconds")
    parser.add_argument("--child-output", default=None)
    args = parser.parse_args()
    args.restatement_rows = min(args.restatement_rows, args.cells)
    if args.child_output:
        return child(args)

    output = os.path.join(tempfile.mkdtemp(prefix="dense_expression_timing_"), "result.npz")
    command = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--child-output", output] + \
              ["--%s=%s" % (name.replace("_", "-"), getattr(args, name)) for name in ("cells", "genes", "density", "repeats", "restatement_rows")]
    done = subprocess.run(command, env=dict(os.environ, EM2_TIMING="1"), capture_output=True, text=True)
    if done.returncode != 0:
        sys.stderr.write(done.stderr[-4000:])
        raise SystemExit("the GPU step ended with status %d: nothing more is started" % done.returncode)
    device = np.load(output)
    import dense_binding as db
    restatement = db.load()
    expected, seconds = restatement.dense_expression(device["toc"], device["data"], args.genes, 2, with_seconds=True)
    result = {"cells": args.cells, "genes": args.genes, "density": args.density, "stored_entries": int(device["entries"]),
              "normalization": "L2", "calls": args.repeats, "roofline_bytes_per_second": ROOFLINE_BYTES_PER_SECOND,
              "restatement_rows": args.restatement_rows, "restatement_seconds_one_thread": seconds,
              "restatement_seconds_all_rows_EXTRAPOLATED": seconds / args.restatement_rows * args.cells}
    # the stderr in order: an "[element type]" line, then that call's stage lines
    for name, item in (("float64", 8), ("float32", 4)):
        part = done.stderr.split("[element type] %s\n" % name)[1:]
        part = [p.split("[element type]")[0] for p in part]
        factors = [float(re.search(r"denseExpression: factors ([0-9.]+) ms", p).group(1)) / 1000. for p in part]
        fill = [float(re.search(r"denseExpression: fill ([0-9.]+) ms", p).group(1)) / 1000. for p in part]
        whole = [float(v) / 1000. for v in re.findall(r"\[whole call\] %s ([0-9.]+) ms" % name, done.stderr)]
        zero = [float(v) / 1000. for v in re.findall(r"\[zero\] %s ([0-9.]+) ms" % name, done.stderr)]
        written = float(args.cells) * args.genes * item
        got = device[name].reshape(args.restatement_rows, args.genes)
        result[name] = {
            "bytes_written": written, "roofline_seconds": written / ROOFLINE_BYTES_PER_SECOND,
            "factors_seconds": factors, "fill_seconds": fill, "whole_call_seconds": whole, "torch_zero_seconds": zero,
            "fill_best_bytes_per_second": written / min(fill), "fill_best_share_of_roofline": written / min(fill) / ROOFLINE_BYTES_PER_SECOND,
            "first_rows_agree_with_the_restatement": db.dense_difference(name, got, expected) is None}
    print(json.dumps(result))


if __name__ == "__main__":
    main()
