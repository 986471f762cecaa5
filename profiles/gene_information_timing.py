"""Timing of the gene information content (csrc/em2_gene_information.hip) on the bench's synthetic matrix
(expressionmatrix2_amd/synthetic.py: by default 1M cells x 30k genes), L2 normalisation, through the device-pointer entry:

    python profiles/gene_information_timing.py [--cells N] [--genes G] [--density D] [--repeats R] [--restatement-genes 20]

Prints one JSON line: the stage times of EM2_TIMING=1 (best of R calls), the achieved bytes per second of the sort and of each
reduction pass against the HBM figure DESIGN.md uses (8 TB/s), and the C++ restatement's seconds per gene on its first genes with
the whole gene set EXTRAPOLATED from them (labelled so).  The GPU step runs in a child process under a time limit of its own;
where it fails nothing more is started."""
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

HBM_BYTES_PER_SECOND = 8e12


def child(args):
    """The GPU step: the matrix in HBM, R calls (stage lines on stderr), the first genes' host CSR and results to a file."""
    import torch
    from expressionmatrix2_amd import capi, synthetic
    lib = capi.load()
    toc, data = synthetic.expression_shard(0, args.cells, args.genes, density=args.density)
    entries = int(data.numel())
    counts = (data >> 32).to(torch.int32).view(torch.float32)
    rows = torch.repeat_interleave(torch.arange(args.cells, device="cuda"), toc[1:] - toc[:-1])
    sum2 = torch.zeros(args.cells, dtype=torch.float64, device="cuda").index_add_(0, rows, (counts * counts).to(torch.float64))
    norm = 1. / torch.sqrt(sum2)          # (the sum's order is torch's: this script times, the tests check the norms)
    del rows
    single = torch.zeros(args.genes, dtype=torch.float32, device="cuda")
    double = torch.zeros(args.genes, dtype=torch.float64, device="cuda")
    expressing = torch.zeros(args.genes, dtype=torch.int32, device="cuda")
    workspace_bytes = lib.em2_dev_gene_information_content_workspace(args.cells, args.genes, entries)
    workspace = torch.empty(workspace_bytes, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    for _ in range(args.repeats):
        begin = time.time()
        capi.check(lib.em2_dev_gene_information_content(toc.data_ptr(), data.data_ptr(), args.cells, args.genes, entries,
                                                        norm.data_ptr(), single.data_ptr(), double.data_ptr(),
                                                        expressing.data_ptr(), workspace.data_ptr(), workspace_bytes, None))
        print("[whole call] %.3f ms" % (1000. * (time.time() - begin)), file=sys.stderr, flush=True)
    host_toc, genes, values = synthetic.csr_to_host(toc, data)
    host = np.zeros(len(genes), dtype=capi.COUNT_DTYPE)
    host["gene"], host["count"] = genes, values
    np.savez(args.child_output, toc=host_toc, data=host, norm=norm.cpu().numpy(), single=single.cpu().numpy(),
             double=double.cpu().numpy(), expressing=expressing.cpu().numpy(), entries=entries)


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--cells", type=int, default=1000000)
    parser.add_argument("--genes", type=int, default=30000)
    parser.add_argument("--density", type=float, default=0.01)
    parser.add_argument("--repeats", type=int, default=3)
    parser.add_argument("--restatement-genes", type=int, default=20)
    parser.add_argument("--limit", type=int, default=400, help="time limit of the GPU step in seconds")
    parser.add_argument("--child-output", default=None)
    args = parser.parse_args()
    if args.child_output:
        return child(args)

    output = os.path.join(tempfile.mkdtemp(prefix="gene_information_timing_"), "result.npz")
    command = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--child-output", output] + \
              ["--%s=%s" % (name, getattr(args, name)) for name in ("cells", "genes", "density", "repeats")]
    done = subprocess.run(command, env=dict(os.environ, EM2_TIMING="1"), capture_output=True, text=True)
    if done.returncode != 0:
        sys.stderr.write(done.stderr[-4000:])
        raise SystemExit("the GPU step ended with status %d: nothing more is started" % done.returncode)
    stages = {}
    for name, value in re.findall(r"geneInformationContent: ([^\n]*?) ([0-9.]+) ms", done.stderr):
        stages.setdefault(name, []).append(float(value) / 1000.)
    best = {name: min(values) for name, values in stages.items()}
    whole = [float(v) / 1000. for v in re.findall(r"\[whole call\] ([0-9.]+) ms", done.stderr)]
    device = np.load(output)
    entries = int(device["entries"])
    gene_bits = max(1, int(np.ceil(np.log2(args.genes))))
    sort_bytes = entries * (16. * np.ceil(gene_bits / 8.) + 4.)          # 8 + 8 per radix pass, the keys once; ASSUMES 8 key bits per pass of rocPRIM's sort
    rates = {"sort": sort_bytes / best["sort"], "pass 1 (sums)": 4. * entries / best["pass 1 (sums)"],
             "pass 2 (terms) and finish": 4. * entries / best["pass 2 (terms) and finish"]}

    import gene_information_binding as gib
    restatement = gib.load()
    n = min(args.restatement_genes, args.genes)
    theirs = restatement.gene_information_content(device["toc"], device["data"], args.genes, device["norm"], 0, n)
    none = theirs["positive"] == 0
    parity = bool(np.array_equal(theirs["expressing"], device["expressing"][:n].view(np.uint32)) and
                  np.array_equal(theirs["single"][none].view(np.uint32), device["single"][:n][none].view(np.uint32)) and
                  np.allclose(theirs["double"], device["double"][:n], rtol=0, atol=1e-9, equal_nan=True))
    print(json.dumps({
        "cells": args.cells, "genes": args.genes, "density": args.density, "stored_entries": entries, "normalization": "L2",
        "stage_seconds_best_of_%d" % args.repeats: best, "whole_device_call_seconds": min(whole) if whole else None,
        "achieved_bytes_per_second": rates, "sort_bytes_assume_8_key_bits_per_radix_pass": True, "share_of_hbm_8e12": {k: v / HBM_BYTES_PER_SECOND for k, v in rates.items()},
        "restatement_seconds_per_gene_first_%d_genes" % n: theirs["seconds"] / n,
        "restatement_seconds_all_genes_EXTRAPOLATED": theirs["seconds"] / n * args.genes,
        "first_genes_agree_with_the_restatement": parity}))


if __name__ == "__main__":
    main()
