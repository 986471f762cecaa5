"""Times ExpressionMatrix.addCells on a generated expression counts file (not run by the tests).

    python profiles/csv_ingest_timing.py [--genes 20000] [--cells 10000] [--out DIR] [--restatement-lines N]

The file is in the style of bench.py's generator: integers, about 90 % "0".  Its gene lines are drawn from a pool of 256
random lines (each gene has its own name), which leaves the statistics of the text -- and so the work of every path -- as
they are and lets a 420 MB file be written in seconds.  Every timing runs in a process of its own, started fresh by this
script, and sets its first call aside (a small file through the same path: code objects, the HIP runtime, the allocator):

    device       the whole addCells call on the GPU path, into a new store
    passes       em2_dev_csv_parse alone, the text resident on the device, chunk by chunk as addCells cuts it; the median
                 of three runs; reported as a share of the streaming roofline for the bytes the passes must move
    host         the whole addCells call on the host path
    restatement  tests/native/em2_csv_restatement.cpp (the reference's loops: getline, a character-by-character tokenizer,
                 strings per token, strtof per field) on one thread; over the whole file, or -- with --restatement-lines N --
                 over the first N gene lines and extrapolated by lines (the output says which)

One JSON line per timing, and a last one with the ratios."""
import argparse
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

HBM_BYTES_PER_SECOND = 6.29e12          # float4 copy, measured (MI355X_MICROARCH.md); the spec is 8.0e12


def generate(directory, genes, cells, seed=1, name="big"):
    rng = np.random.default_rng(seed)
    pool = []
    for _ in range(min(256, genes)):
        values = rng.integers(1, 200, cells)
        values[rng.random(cells) < .9] = 0
        pool.append(",".join(map(str, values.tolist())))
    expression = os.path.join(directory, name + "_expression.csv")
    with open(expression, "w") as f:
        f.write("," + ",".join("cell%d" % i for i in range(cells)) + "\n")
        for g, p in enumerate(rng.integers(0, len(pool), genes).tolist()):
            f.write("gene%d,%s\n" % (g, pool[p]))
    meta = os.path.join(directory, name + "_meta.csv")
    with open(meta, "w") as f:
        f.write("cell,tissue\n")
        for i in range(cells):
            f.write("cell%d,t%d\n" % (i, i % 7))
    return expression, meta


def add_cells(directory, expression, meta, use_device):
    from expressionmatrix2_amd import ExpressionMatrix
    import expressionmatrix2_amd.expression_matrix as facade
    facade.CSV_USE_DEVICE = use_device
    shutil.rmtree(directory, ignore_errors=True)
    e = ExpressionMatrix.create(directory)
    t0 = time.perf_counter()
    e.addCells(expressionCountsFileName=expression, cellMetaDataFileName=meta)
    seconds = time.perf_counter() - t0                      # (the call ends with every result back on the host)
    result = {"seconds": seconds, "cells": e.cellCount(), "genes": e.geneCount(), "deferred_fields": e.lastCsvDeferredFieldCount,
              "chunk_bytes": facade.CSV_CHUNK_BYTES}
    e.close()
    shutil.rmtree(directory, ignore_errors=True)
    return result


def passes(expression, cells):
    import torch
    import csv_binding as cb
    from expressionmatrix2_amd import capi
    import expressionmatrix2_amd.expression_matrix as facade
    lib = capi.load()
    text = open(expression, "rb").read()
    body = text[text.index(b"\n") + 1:]
    kept = torch.from_numpy(np.concatenate([[cb.NONE], np.arange(cells)]).astype(np.uint32).view(np.uint8)).cuda()
    chunks, at = [], 0
    while at < len(body):
        end = len(body) if len(body) - at <= facade.CSV_CHUNK_BYTES else body.rindex(b"\n", at, at + facade.CSV_CHUNK_BYTES) + 1
        chunks.append((at, end))
        at = end
    runs, moved, counts_all = [], 0, None
    for run in range(4):                                    # the first is set aside
        seconds, moved, totals = 0., 0, [0, 0, 0]
        for begin, end in chunks:
            n = end - begin
            d_text = torch.from_numpy(np.frombuffer(body, np.uint8, n, begin).copy()).cuda()
            lines, triples, deferred = n // (cells + 1) + 2, n // 8 + 1024, n // 64 + 1024
            out = [torch.empty(size, dtype=torch.uint8, device="cuda") for size in (24 * lines, 8 * triples, 4 * triples, 16 * deferred)]
            counts = (cb.c.c_uint64 * 3)()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            capi.check(lib.em2_dev_csv_parse(d_text.data_ptr(), n, b",", 1, cells + 1, kept.data_ptr(), 0, lines, out[0].data_ptr(), triples,
                                             out[1].data_ptr(), out[2].data_ptr(), deferred, out[3].data_ptr(), counts, None))
            seconds += time.perf_counter() - t0             # (the entry leaves the stream synchronised)
            assert counts[0] <= lines and counts[1] <= triples and counts[2] <= deferred
            # what the passes must move: the text once (the three kernels read it three times), the line table, the counts
            moved += n + 24 * counts[0] + 12 * counts[1] + 16 * counts[2]
            totals = [a + int(b) for a, b in zip(totals, counts)]
        if run:
            runs.append(seconds)
        counts_all = totals
    seconds = float(np.median(runs))
    return {"seconds": seconds, "runs": runs, "chunks": len(chunks), "bytes_that_must_move": moved, "lines": counts_all[0],
            "counts": counts_all[1], "deferred_fields": counts_all[2], "roofline_seconds": moved / HBM_BYTES_PER_SECOND,
            "share_of_streaming_roofline": moved / HBM_BYTES_PER_SECOND / seconds}


def restatement(expression, meta, lines):
    import csv_binding as cb
    total = sum(1 for _ in open(expression, "rb")) - 1
    path, what = expression, "the whole file"
    if lines and lines < total:
        path, what = expression + ".head", "the first %d of %d gene lines, extrapolated by lines" % (lines, total)
        with open(expression, "rb") as f, open(path, "wb") as g:
            for _ in range(lines + 1):
                g.write(f.readline())
    warm = generate(os.path.dirname(expression), 20, 30, name="warm")
    cb.restated_add_cells(warm[0], ",", warm[1], ",")       # set aside
    n = cb.c.c_uint64(0)
    t0 = time.perf_counter()
    cb.load().em2r_csv_add_cells(path.encode(), b",", meta.encode(), b",", b"", 0, cb.ctypes.byref(n))
    seconds = time.perf_counter() - t0
    scale = total / lines if lines and lines < total else 1.
    return {"seconds": seconds * scale, "measured_seconds": seconds, "over": what}


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--genes", type=int, default=20000)
    parser.add_argument("--cells", type=int, default=10000)
    parser.add_argument("--out", default=None)
    parser.add_argument("--restatement-lines", type=int, default=0)
    parser.add_argument("--mode", default=None)
    parser.add_argument("--files", default=None)
    args = parser.parse_args()
    if args.mode is None:                                   # the parent: the files, then a fresh process per timing
        work = tempfile.mkdtemp(prefix="csv_ingest_timing_")
        try:
            expression, meta = generate(work, args.genes, args.cells)
            results = {"file_bytes": os.path.getsize(expression), "genes": args.genes, "cells": args.cells}
            for mode in ("device", "passes", "host", "restatement"):
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--mode", mode, "--files", work, "--genes", str(args.genes),
                                    "--cells", str(args.cells), "--restatement-lines", str(args.restatement_lines)],
                                   capture_output=True, text=True)
                if r.returncode != 0:
                    raise RuntimeError("%s failed:\n%s" % (mode, r.stderr[-3000:]))
                results[mode] = json.loads(r.stdout.strip().splitlines()[-1])
                print(json.dumps({mode: results[mode]}), flush=True)
            results["restatement_over_device"] = results["restatement"]["seconds"] / results["device"]["seconds"]
            results["host_over_device"] = results["host"]["seconds"] / results["device"]["seconds"]
            print(json.dumps(results), flush=True)
            if args.out:
                os.makedirs(args.out, exist_ok=True)
                with open(os.path.join(args.out, "csv_ingest_timing.json"), "w") as f:
                    json.dump(results, f, indent=1)
        finally:
            shutil.rmtree(work, ignore_errors=True)
        return
    expression, meta = os.path.join(args.files, "big_expression.csv"), os.path.join(args.files, "big_meta.csv")
    if args.mode in ("device", "host"):
        small = generate(args.files, 50, 40, name="small_" + args.mode)
        add_cells(os.path.join(args.files, "store_small_" + args.mode), small[0], small[1], args.mode == "device")       # set aside
        result = add_cells(os.path.join(args.files, "store_" + args.mode), expression, meta, args.mode == "device")
    elif args.mode == "passes":
        result = passes(expression, args.cells)
    else:
        result = restatement(expression, meta, args.restatement_lines)
    print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()
