"""Timing of findSimilarGenePairs0 (csrc/em2_gene_pairs.hip) at one configuration: by default 8192 genes x 65536 cells of
synth data, L2, k = 100, threshold 0.2.  A stand-alone script, not a test and not bench.py:

    python profiles/gene_pairs_timing.py [--genes G] [--cells N] [--density D] [--band B] [--repeats R]

The GPU step runs in a child process of its own under a time limit (--limit seconds); the parent reads the stage lines the
library prints with EM2_TIMING=1.  Reported, as one JSON line:
  * seconds of each stage (dense vectors, pair kernel, sort, selection) and of the whole call, best of R repeats;
  * multiply-adds per second of the pair kernel: G (G - 1) / 2 * N pairs-times-cells over its time (the kernel also walks the
    diagonal tiles' lower halves and the padding, which are not counted);
  * that rate as a fraction of the kernel's own roofline.  The roofline used: HALF THE FP32 VECTOR PEAK.  Without FMA a
    multiply-add is two vector operations (one multiplication, one addition, each rounded), the peak of 157.3 TFLOP/s counts an
    FMA as two operations, so the bound is 157.3e12 / 4 = 39.3e12 multiply-adds per second.  The packed instructions the
    kernel uses (v_pk_mul_f32, v_pk_add_f32) do two lanes' worth per instruction but are assumed to run at the same
    operations-per-clock peak, not above it;
  * the restatement's time per multiply-add on a band of B genes on this host (one thread), and the whole problem
    EXTRAPOLATED from it (labelled as such: nobody ran the restatement on the whole problem);
  * parity: the band is the LAST B genes of the problem.  The last gene has every partner below it, so the band holds its
    whole row: the restatement's keepBest and std::sort (the real std::nth_element and std::sort) run on that row, and the
    device's stored list of that gene -- usedCount, which partners, their order, the float bits -- must equal the result.
    For the other genes of the band the stored partners below the gene must carry exactly the restatement's r, and where the
    list was not cut to k they must be exactly the restatement's survivors.  (allSimilarities is limited to 8192 genes and
    not used here.)
"""
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

VECTOR_PEAK_FLOPS = 157.3e12            # MI355X, FP32 vector, an FMA counted as two operations
ROOFLINE_MULTIPLY_ADDS = VECTOR_PEAK_FLOPS / 4.


def make_input(genes, cells, density, seed):
    import fsp0_binding
    return fsp0_binding.clustered(cells, genes, density, seed=seed, cluster_count=16)


def child(args):
    """The GPU step: R calls; the stage lines go to stderr, the result of the last call to a file."""
    from expressionmatrix2_amd import capi
    toc, data = make_input(args.genes, args.cells, args.density, args.seed)
    for _ in range(args.repeats):
        begin = time.time()
        pairs, used = capi.find_similar_gene_pairs0(toc, data, args.genes, 2, args.k, args.threshold)
        print("[whole call] %.3f ms" % (1000. * (time.time() - begin)), file=sys.stderr, flush=True)
    np.savez(args.child_output, cell=pairs["cell"], similarity=pairs["similarity"], used=used)


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--genes", type=int, default=8192)
    parser.add_argument("--cells", type=int, default=65536)
    parser.add_argument("--density", type=float, default=0.02)
    parser.add_argument("--seed", type=int, default=1)
    parser.add_argument("--k", type=int, default=100)
    parser.add_argument("--threshold", type=float, default=0.2)
    parser.add_argument("--band", type=int, default=2, help="genes of the restatement's band (the last genes of the problem)")
    parser.add_argument("--repeats", type=int, default=3)
    parser.add_argument("--limit", type=int, default=300, help="time limit of the GPU step in seconds")
    parser.add_argument("--child-output", default=None)
    args = parser.parse_args()
    if args.child_output:
        return child(args)

    output = os.path.join(tempfile.mkdtemp(prefix="gene_pairs_timing_"), "result.npz")
    environment = dict(os.environ, EM2_TIMING="1")
    command = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--child-output", output] + \
              ["--%s=%s" % (name, getattr(args, name)) for name in ("genes", "cells", "density", "seed", "k", "threshold", "repeats")]
    done = subprocess.run(command, env=environment, capture_output=True, text=True)
    if done.returncode != 0:
        sys.stderr.write(done.stderr[-4000:])
        raise SystemExit("the GPU step ended with status %d: nothing more is started" % done.returncode)
    stages = {}
    for name, value in re.findall(r"findSimilarGenePairs0: ([^\n]*?) ([0-9.]+) ms", done.stderr):
        stages.setdefault(name, []).append(float(value) / 1000.)
    whole = [float(v) / 1000. for v in re.findall(r"\[whole call\] ([0-9.]+) ms", done.stderr)]
    best = {name: min(values) for name, values in stages.items()}
    multiply_adds = args.genes * (args.genes - 1) / 2. * args.cells
    rate = multiply_adds / best["pair kernel"]

    # the restatement on a band: the last `band` genes against all genes below them
    import gene_pairs_binding
    restatement = gene_pairs_binding.load()
    toc, data = make_input(args.genes, args.cells, args.density, args.seed)
    begin_gene = args.genes - args.band
    band, seconds = restatement.gene_pair_band(toc, data, args.genes, 2, begin_gene, args.genes)
    band_multiply_adds = sum(range(begin_gene, args.genes)) * float(args.cells)
    device = np.load(output)
    parity = True
    for i, gene in enumerate(range(begin_gene, args.genes)):
        # the band's view of gene `gene`: its partners BELOW it; the device stored its k best among all partners
        used = int(device["used"][gene])
        below = device["cell"][gene, :used] < gene
        partners, similarities = device["cell"][gene, :used][below], device["similarity"][gene, :used][below]
        parity = parity and bool(np.array_equal(band[i, partners].view(np.uint32), similarities.view(np.uint32)))
        if used < args.k:                       # the list was not cut: every survivor below the gene must be stored
            survivors = np.nonzero(band[i, :gene].astype(np.float64) > args.threshold)[0]
            parity = parity and bool(np.array_equal(np.sort(partners), survivors))
    # the last gene: its whole row is in the band, so its stored list is checked in full
    last = args.genes - 1
    gene, similarity, used = restatement.keep_best_and_sort(band[-1, :last], args.k, args.threshold)
    parity = parity and used == int(device["used"][last]) and bool(np.array_equal(device["cell"][last], gene)) and \
        bool(np.array_equal(device["similarity"][last].view(np.uint32), similarity.view(np.uint32)))
    result = {
        "genes": args.genes, "cells": args.cells, "density": args.density, "k": args.k, "threshold": args.threshold,
        "stage_seconds_best_of_%d" % args.repeats: best, "whole_call_seconds": min(whole) if whole else None,
        "stored_pairs": int(device["used"].sum()),
        "pair_kernel_multiply_adds_per_second": rate,
        "roofline_multiply_adds_per_second": ROOFLINE_MULTIPLY_ADDS,
        "roofline_used": "half the FP32 vector peak (157.3 TFLOP/s / 4 multiply-adds per second: no FMA)",
        "fraction_of_roofline": rate / ROOFLINE_MULTIPLY_ADDS,
        "restatement_band_genes": args.band, "restatement_band_seconds": seconds,
        "restatement_seconds_per_multiply_add": seconds / band_multiply_adds,
        "restatement_whole_problem_seconds_EXTRAPOLATED": seconds / band_multiply_adds * multiply_adds,
        "band_parity": parity, "last_gene_candidates": int((band[-1, :last].astype(np.float64) > args.threshold).sum()),
    }
    print(json.dumps(result))
    if not parity:
        raise SystemExit("the device's stored pairs of the band differ from the restatement")


if __name__ == "__main__":
    main()
