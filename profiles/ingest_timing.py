"""Timing of the device pass of the bulk add (csrc/em2_ingest.hip: em2_dev_ingest_count plus em2_dev_ingest_fill) at one
configuration: by default 10^6 cells x 30 000 genes x ~300 entries per cell of the bench's generator
(expressionmatrix2_amd/synthetic.py), the columns shuffled within every row.  A stand-alone script, not a test and not bench.py:

    python profiles/ingest_timing.py [--cells N] [--genes G] [--density D] [--repeats R] [--sample S]

The GPU step runs in a child process of its own under a time limit (--limit seconds).  Reported, as one JSON line:
  * seconds of each pass, best of R repeats (wall time around the call: both entries leave the stream synchronised);
  * the bytes the two passes must move -- count: indptr, indices, values in, 12 bytes per cell and the toc out; fill: the same
    in, 8 bytes per kept entry and 56 per cell out; the gather from the gene map is not counted -- and that over the streaming
    roofline used by profiles/dense_expression_timing.py, 6.29 TB/s (the float4 copy rate of the MI355X);
  * the C++ restatement (tests/native/em2_ingest_restatement.cpp) on the first S cells on one thread of this host, its seconds
    per entry, and the whole problem EXTRAPOLATED from it (labelled as such);
  * parity: the device's kept counts, entries and Cell records of those S cells equal the restatement's bytes.
"""
import argparse
import json
import os
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
    import torch
    from expressionmatrix2_amd import capi, synthetic
    lib = capi.load()
    toc, data = synthetic.expression_shard(0, args.cells, args.genes, density=args.density, device="cuda")
    entries = int(toc[-1].item())
    rows = torch.repeat_interleave(torch.arange(args.cells, device="cuda"), toc[1:] - toc[:-1])
    generator = torch.Generator(device="cuda")
    generator.manual_seed(7)
    order = torch.argsort(rows * (1 << 31) + torch.randint(0, 1 << 31, (entries,), generator=generator, device="cuda"))
    del rows
    data = data[order]                                       # columns shuffled within every row
    del order
    indices = (data & 0xFFFFFFFF).to(torch.int32).contiguous()
    values = (data >> 32).to(torch.int32).view(torch.float32).contiguous()
    del data
    gene_map = torch.arange(args.genes, dtype=torch.int32, device="cuda")
    kept = torch.zeros(args.cells, dtype=torch.int32, device="cuda")
    status, duplicate = torch.zeros_like(kept), torch.zeros_like(kept)
    out_toc = torch.zeros(args.cells + 1, dtype=torch.int64, device="cuda")
    out_data = torch.zeros(entries, dtype=torch.int64, device="cuda")
    out_cells = torch.zeros(7 * args.cells, dtype=torch.float64, device="cuda")
    seconds = {"count": [], "fill": []}
    for _ in range(args.repeats):
        torch.cuda.synchronize()
        begin = time.time()
        capi.check(lib.em2_dev_ingest_count(toc.data_ptr(), indices.data_ptr(), values.data_ptr(), None, args.cells, gene_map.data_ptr(),
                                            args.genes, kept.data_ptr(), status.data_ptr(), duplicate.data_ptr(), out_toc.data_ptr(), None))
        seconds["count"].append(time.time() - begin)
        begin = time.time()
        capi.check(lib.em2_dev_ingest_fill(toc.data_ptr(), indices.data_ptr(), values.data_ptr(), None, args.cells, gene_map.data_ptr(),
                                           args.genes, out_toc.data_ptr(), out_data.data_ptr(), out_cells.data_ptr(), None))
        seconds["fill"].append(time.time() - begin)
    sample = min(args.sample, args.cells)
    sample_entries = int(toc[sample].item())
    np.savez(args.child_output, count_seconds=seconds["count"], fill_seconds=seconds["fill"], entries=entries,
             kept_entries=int(out_toc[-1].item()), failed=int((status != 0).sum().item()),
             indptr=toc[:sample + 1].cpu().numpy().astype(np.uint64), indices=indices[:sample_entries].cpu().numpy().view(np.uint32),
             values=values[:sample_entries].cpu().numpy(), kept=kept[:sample].cpu().numpy().view(np.uint32),
             out_toc=out_toc[:sample + 1].cpu().numpy().astype(np.uint64),
             out_data=out_data[:int(out_toc[sample].item())].cpu().numpy().view(np.uint8),
             out_cells=out_cells[:7 * sample].cpu().numpy().view(np.uint8))


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--cells", type=int, default=1000000)
    parser.add_argument("--genes", type=int, default=30000)
    parser.add_argument("--density", type=float, default=0.01)
    parser.add_argument("--repeats", type=int, default=3)
    parser.add_argument("--sample", type=int, default=20000, help="cells of the restatement's run (the first cells)")
    parser.add_argument("--limit", type=int, default=300, help="time limit of the GPU step in seconds")
    parser.add_argument("--child-output", default=None)
    args = parser.parse_args()
    if args.child_output:
        return child(args)

    output = os.path.join(tempfile.mkdtemp(prefix="ingest_timing_"), "result.npz")
    command = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--child-output", output] + \
              ["--%s=%s" % (name, getattr(args, name)) for name in ("cells", "genes", "density", "repeats", "sample")]
    done = subprocess.run(command, capture_output=True, text=True)
    if done.returncode != 0:
        sys.stderr.write(done.stderr[-4000:])
        raise SystemExit("the GPU step ended with status %d: nothing more is started" % done.returncode)
    device = np.load(output)
    entries, kept_entries = int(device["entries"]), int(device["kept_entries"])
    count_seconds, fill_seconds = float(device["count_seconds"].min()), float(device["fill_seconds"].min())
    count_bytes = 8 * (args.cells + 1) + 8 * entries + 12 * args.cells + 8 * (args.cells + 1)
    fill_bytes = 8 * (args.cells + 1) + 8 * entries + 8 * (args.cells + 1) + 8 * kept_entries + 56 * args.cells

    import ingest_binding as ib
    sample = len(device["kept"])
    csr = ib.Csr([])
    csr.indptr, csr.indices, csr.values, csr.cells = device["indptr"], device["indices"], device["values"], sample
    begin = time.time()
    expected = ib.restate(csr, np.arange(args.genes, dtype=np.uint32))
    restatement_seconds = time.time() - begin
    sample_entries = int(device["indptr"][-1])
    parity = bool(np.array_equal(expected["kept"], device["kept"]) and np.array_equal(expected["toc"], device["out_toc"]) and
                  np.array_equal(expected["data"], device["out_data"]) and np.array_equal(expected["cells"], device["out_cells"]))
    result = {
        "cells": args.cells, "genes": args.genes, "entries": entries, "kept_entries": kept_entries, "rows_with_an_error": int(device["failed"]),
        "count_seconds_best_of_%d" % args.repeats: count_seconds, "fill_seconds_best_of_%d" % args.repeats: fill_seconds,
        "both_passes_seconds": count_seconds + fill_seconds,
        "count_bytes": count_bytes, "fill_bytes": fill_bytes, "roofline_bytes_per_second": ROOFLINE_BYTES_PER_SECOND,
        "roofline_seconds_both_passes": (count_bytes + fill_bytes) / ROOFLINE_BYTES_PER_SECOND,
        "share_of_roofline": (count_bytes + fill_bytes) / ROOFLINE_BYTES_PER_SECOND / (count_seconds + fill_seconds),
        "restatement_cells": sample, "restatement_seconds_one_thread": restatement_seconds,
        "restatement_seconds_per_entry": restatement_seconds / max(sample_entries, 1),
        "restatement_whole_problem_seconds_EXTRAPOLATED": restatement_seconds / max(sample_entries, 1) * entries,
        "sample_parity": parity,
    }
    print(json.dumps(result))
    if not parity:
        raise SystemExit("the device's entries or Cell records of the sample differ from the restatement")


if __name__ == "__main__":
    main()
