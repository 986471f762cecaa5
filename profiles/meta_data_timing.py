"""Timing of the contingency table of two labelings (csrc/em2_contingency.hip) at n cells (by default 10^6) with the ids
already on the device:

    python profiles/meta_data_timing.py [--cells N] [--repeats R]

Two inputs: (a) 64 x 64 values, (b) one field with about 10^5 values, many of them singletons, against 64 values (what
createMetaDataFromClusterGraph leaves when many cells are unclustered).  Prints one JSON line: the LDS path and the sort path on
(a), the sort path on (b) (em2_dev_contingency, the whole call with the results copied to the host, R calls each, all listed in
call order), the host entry including its upload on both inputs, and the C++ restatement
(tests/native/em2_meta_data_restatement.cpp: a std::map of pairs) on one thread of the same box, with whether every table equals
the restatement's.  Each GPU step runs in a child process under a time limit of its own; where one fails nothing more is
started."""
import argparse
import json
import os
import re
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

STEPS = ("a-lds", "a-sort", "b-sort", "a-host", "b-host")


def ids_of(which, n, seed=1):
    rng = np.random.default_rng(seed)
    if which == "a":
        id0 = rng.integers(0, 64, n).astype(np.uint32)
        id1 = ((id0 + (rng.random(n) ** 3 * 64).astype(np.uint32)) % 64).astype(np.uint32)      # correlated with id0
        return id0, id1, 64, 64
    values = max(2, n // 10)                                    # about 10^5 at a million cells
    heavy = rng.integers(0, 40, n).astype(np.uint32)            # forty clusters hold 70 % of the cells ...
    own = (40 + rng.integers(0, values - 40, n)).astype(np.uint32)      # ... the others mostly a value of their own
    id0 = np.where(rng.random(n) < 0.7, heavy, own).astype(np.uint32)
    id1 = rng.integers(0, 64, n).astype(np.uint32)
    return id0, id1, values, 64


def child(args):
    """One GPU step: R calls, their wall times on stderr, the last table to a file."""
    import torch
    from expressionmatrix2_amd import capi
    which, how = args.step.split("-")
    id0, id1, n0, n1 = ids_of(which, args.cells)
    path = {"lds": capi.CONTINGENCY_LDS, "sort": capi.CONTINGENCY_SORT, "host": capi.CONTINGENCY_AUTOMATIC}[how]
    if how != "host":
        d0 = torch.from_numpy(id0.view(np.int32)).to("cuda")
        d1 = torch.from_numpy(id1.view(np.int32)).to("cuda")
        torch.cuda.synchronize()
    table = None
    for _ in range(args.repeats):
        begin = time.perf_counter()
        if how == "host":
            table = capi.contingency(id0, id1, n0, n1, path)
        else:
            table = capi.dev_contingency(d0.data_ptr(), d1.data_ptr(), args.cells, n0, n1, path)
        print("[call] %.3f ms" % (1000. * (time.perf_counter() - begin)), file=sys.stderr, flush=True)
    np.savez(args.child_output, sums=np.array([table["sumCells"], table["sumRows"], table["sumColumns"]], dtype=np.uint64),
             path=table["path"], **{key: table[key] for key in ("rowTotals", "columnTotals", "i0", "i1", "count")})


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--cells", type=int, default=1000000)
    parser.add_argument("--repeats", type=int, default=5)
    parser.add_argument("--limit", type=int, default=120, help="time limit of each GPU step in seconds")
    parser.add_argument("--step", default=None)
    parser.add_argument("--child-output", default=None)
    args = parser.parse_args()
    if args.child_output:
        return child(args)

    import tempfile
    import meta_data_binding as mb
    directory = tempfile.mkdtemp(prefix="meta_data_timing_")
    result = {"cells": args.cells, "repeats": args.repeats}
    expected = {}
    for which in ("a", "b"):
        id0, id1, n0, n1 = ids_of(which, args.cells)
        begin = time.perf_counter()
        expected[which] = mb.load().contingency(id0, id1, n0, n1)
        result["%s_restatement_seconds_one_thread" % which] = time.perf_counter() - begin
        result["%s_values" % which] = [n0, n1]
        result["%s_table_cells_not_zero" % which] = int(len(expected[which]["count"]))
    for step in STEPS:
        output = os.path.join(directory, step + ".npz")
        command = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--child-output", output,
                   "--step", step, "--cells", str(args.cells), "--repeats", str(args.repeats)]
        done = subprocess.run(command, capture_output=True, text=True)
        if done.returncode != 0:
            sys.stderr.write(done.stderr[-4000:])
            print(json.dumps(result))
            raise SystemExit("the GPU step %s ended with status %d: nothing more is started" % (step, done.returncode))
        seconds = [float(v) / 1000. for v in re.findall(r"\[call\] ([0-9.]+) ms", done.stderr)]
        table = np.load(output)
        theirs = expected[step[0]]
        equal = bool(all(np.array_equal(table[key], theirs[key]) for key in mb.CONTINGENCY_KEYS) and
                     [int(x) for x in table["sums"]] == [theirs["sumCells"], theirs["sumRows"], theirs["sumColumns"]])
        key = step.replace("-", "_")
        result[key + "_seconds_all_in_call_order"] = seconds
        result[key + "_seconds_slowest_after_the_first"] = max(seconds[1:]) if len(seconds) > 1 else None
        result[key + "_seconds_fastest"] = min(seconds)
        result[key + "_path"] = int(table["path"])
        result[key + "_equals_the_restatement"] = equal
    print(json.dumps(result))


if __name__ == "__main__":
    main()
