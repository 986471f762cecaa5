#!/usr/bin/env python3
"""Randomised parity sweep on a GPU box (not part of pytest): random shapes, thresholds, k and scan-form knobs, every
result compared bit for bit with the CPU oracle.  SECONDS=300 python3 tools/fuzz_parity.py [seed]
FUZZ_ONLY=fsp4 restricts the sweep to one path, FUZZ_WIDTHS=1100,1500,2048 to those signature widths, FUZZ_MODE=triangle
to one scan form with the matrix cores on.  The fsp6 leg compares with the C++ restatement (tests/fsp6_binding.py); shapes past
its kernels' limits must answer EM2_ERROR_UNSUPPORTED and are counted apart (fsp6_unsupported), as are runs at the 8192
clamp and runs over several row chunks.  Half the fsp7 draws go through the device entry on a random row range (fsp7_ranged);
fsp7 draws the oracle would be slow for are skipped and counted (fsp7_skipped, see fsp7_oracle_is_slow).  The fsp5 leg draws its
width from FSP5_WIDTHS (the common widths and those that leave lanes of the 16-byte filter without a unit), compares a third
of its draws on a random row range through the device entry (fsp5_ranged), and names the forms that ran in a failure's label.

Six more legs draw from tests/expression_cases.py, the generator tests/test_gpu_expression_sweep.py takes its fixed draws from:
fsp0, stored_pairs (analyzeSimilarPairs), analyze_lsh, cluster_graph, gene_pairs and gene_information, each against its C++
restatement (analyze_lsh: the oracle) with the comparison of its own test file.  FUZZ_ONLY=<leg> works for each.  A draw above
the cost cap of its leg is counted as <leg>_skipped; one that reaches a place the reference leaves open or asserts in (a makeKnn
tie or a NaN similarity of the cluster graph, bin < binCount of the two analyses -- the device entry must then answer with the
reference's text) as <leg>_discarded.  On a difference the case dict is printed: expression_cases.ENTRIES[leg].check(case,
reference) reproduces it.

Two legs draw from tests/ingest_limit_cases.py: csv_parse (random structure and numeric fields, tile size, misalignment and kept
subset through csv_binding.assert_parse, against the model of em2_dev_csv_parse) and ingest (row lengths around 512 and the LDS
row limit, value kinds, orders, duplicates, zeros and skip flags through ingest_binding.assert_same, against the restatement of
addCell's storing part).  FUZZ_ONLY=csv_parse / ingest selects them; a difference prints the draw's dict (its seed rebuilds it:
ingest_limit_cases.draw_csv_parse(None, seed) / draw_ingest(None, seed)).

One leg draws from tests/projection_limit_cases.py (FUZZ_ONLY=projection_limits): quantisation traps, float-copy traps and flip
points with random seeds, sizes and widths through capi.compute_signatures, against the oracle; a difference prints the draw
(projection_limit_cases.build(draw) rebuilds the case)."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import expression_cases  # noqa: E402
import fsp6_binding  # noqa: E402
import oracle_binding  # noqa: E402
import projection_limit_cases  # noqa: E402
import synth  # noqa: E402
from label_graphs import fast_graph  # noqa: E402
from expressionmatrix2_amd import capi  # noqa: E402

WIDTHS = [1, 32, 64, 100, 128, 192, 256, 512, 600, 1000, 1024, 1024, 1024, 1100, 2000, 2048, 2048, 4096]
FSP5_WIDTHS = WIDTHS + [384, 640, 1280, 1920, 2176, 3072, 3968]
KNOBS = ("EM2_SCAN_MODE", "EM2_MIN_SEGMENT_COLUMNS", "EM2_LOG_CAPACITY", "EM2_FULL_ROW_CELLS",
         "EM2_PREFIX_PERMILLE", "EM2_TILE_SEGMENTS", "EM2_BLOCKS_PER_CU", "EM2_SCAN_MATRIX", "EM2_MATRIX_CONVOY")


def main():
    seed = int(sys.argv[1]) if len(sys.argv) > 1 else 1
    rng = np.random.default_rng(seed)
    oracle = oracle_binding.load_oracle()
    deadline = time.time() + float(os.environ.get("SECONDS", "120"))
    restatement6 = fsp6_binding.load()
    runs = {"fsp4": 0, "fsp5": 0, "fsp6": 0, "fsp7": 0, "signatures": 0, "graph": 0, "labels": 0, "fsp6_unsupported": 0,
            "fsp6_clamp8192": 0, "fsp6_chunks": 0, "fsp7_ranged": 0, "fsp7_skipped": 0, "fsp5_ranged": 0}
    for name in expression_cases.ENTRIES:
        runs.update({name: 0, name + "_skipped": 0, name + "_discarded": 0})
    runs.update({name: 0 for name in WRITE_LEGS})
    runs["projection_limits"] = 0
    references = {}
    while time.time() < deadline:
        for key in KNOBS:
            os.environ.pop(key, None)
        if os.environ.get("FUZZ_ONLY") == "projection_limits" or (rng.random() < 0.08 and not os.environ.get("FUZZ_ONLY")):
            draw = projection_limit_cases.draw(rng)
            case = projection_limit_cases.build(draw)
            arguments = (case["gene_count"], case["vectors"], case["L"])
            expect = oracle.compute_signatures(case["toc"], case["genes"], case["counts"], *arguments)
            got = capi.compute_signatures(case["toc"], capi.make_counts(case["genes"], case["counts"]), *arguments)
            if not np.array_equal(expect, got):
                raise SystemExit("PARITY FAILURE projection_limits %r" % draw)
            runs["projection_limits"] += 1
            continue
        if os.environ.get("FUZZ_ONLY") in WRITE_LEGS or (rng.random() < 0.1 and not os.environ.get("FUZZ_ONLY")):
            write_leg(rng, os.environ.get("FUZZ_ONLY") or str(rng.choice(WRITE_LEGS)), runs)
            continue
        if os.environ.get("FUZZ_ONLY") in expression_cases.ENTRIES or (rng.random() < 0.35 and not os.environ.get("FUZZ_ONLY")):
            name = os.environ.get("FUZZ_ONLY") or str(rng.choice(list(expression_cases.ENTRIES)))
            expression_leg(rng, name, references, runs)
            continue
        if os.environ.get("FUZZ_ONLY") == "labels" or (rng.random() < 0.15 and not os.environ.get("FUZZ_ONLY")):
            # label propagation over a random k-NN-like graph: every schedule against the serial oracle
            vertices = int(rng.choice([2, 3, 50, 64, 65, 1000, 5000, 30000, 70000]))
            degree = int(rng.choice([1, 2, 5, 12, 30, 50]))
            hubs = int(rng.choice([0, 0, 1, 4, 30]))
            case = dict(vertices=vertices, degree=degree, clusters=int(rng.choice([1, 3, 10, 40])), hubs=min(hubs, vertices),
                        hub_degree=int(rng.choice([70, 150, 300, 500, 700, 3000])), parallel=int(rng.choice([0, 0, 5, 200])),
                        ties=int(rng.choice([0, 0, 2, 16])), graph_seed=int(rng.integers(1 << 30)),
                        seed=int(rng.choice([231, 1, 2 ** 33 + 7])), stable=int(rng.choice([0, 1, 3])),
                        max_iterations=int(rng.choice([0, 1, 3, 100])), ticket=str(rng.choice(["", "", "1", "3", "8"])),
                        pool=str(rng.choice(["", "", "0", "1", "3"])))
            cells, v0, v1, s = fast_graph(np.random.default_rng(case["graph_seed"]), vertices, degree, case["clusters"],
                                          case["hubs"], case["hub_degree"], case["parallel"] if vertices > 3 else 0, case["ties"])
            for name, key in (("EM2_LABEL_TICKET_BATCH", "ticket"), ("EM2_LABEL_POOL_AREAS", "pool")):
                if case[key]:
                    os.environ[name] = case[key]
            got = capi.cell_graph_label_propagation(cells, v0, v1, s, case["seed"], case["stable"], case["max_iterations"])
            for name in ("EM2_LABEL_TICKET_BATCH", "EM2_LABEL_POOL_AREAS"):
                os.environ.pop(name, None)
            expect = oracle.label_propagation(cells, v0, v1, s, case["seed"], case["stable"], case["max_iterations"])
            if got[1] != expect[1] or not np.array_equal(got[0], expect[0]):
                raise SystemExit("PARITY FAILURE labels %r" % case)
            runs["labels"] += 1
            continue
        n = int(rng.choice([1, 2, 63, 64, 65, 200, 500, 1000, 1500, 2500, 4000]))
        L = int(rng.choice(WIDTHS))
        if os.environ.get("FUZZ_WIDTHS"):
            L = int(rng.choice([int(x) for x in os.environ["FUZZ_WIDTHS"].split(",")]))
        k = int(rng.choice([1, 2, 5, 10, 33, 100, 300]))
        thr = float(rng.choice([-1.0, -0.5, 0.0, 0.1, 0.2, 0.5, 0.9]))
        clusters = int(rng.choice([1, 2, 5, 20]))
        flip = float(rng.choice([0.0, 0.02, 0.1, 0.3, 0.5]))
        sig_seed = int(rng.integers(1 << 30))
        sig = synth.clustered_signatures(n, L, cluster_count=clusters, flip=flip, seed=sig_seed)
        what = rng.choice(["fsp4", "fsp4", "fsp4", "fsp5", "fsp6", "fsp7", "signatures", "graph"])
        what = os.environ.get("FUZZ_ONLY", what)
        label = dict(n=n, L=L, k=k, thr=thr, clusters=clusters, flip=flip, sig_seed=sig_seed)
        if what == "fsp4":
            knobs = {"EM2_SCAN_MODE": str(rng.choice(["persistent", "triangle", "virtual:%d" % int(rng.choice([1, 2, 3, 4, 8])), "simple", "rows"])),
                     "EM2_MIN_SEGMENT_COLUMNS": str(int(rng.choice([64, 100, 257, 1000, 4096]))),
                     "EM2_LOG_CAPACITY": str(int(rng.choice([1, 3, 16, 256]))),
                     "EM2_FULL_ROW_CELLS": str(int(rng.choice([0, 64, 200, 1000, 100000]))),
                     "EM2_PREFIX_PERMILLE": str(int(rng.choice([50, 200, 500, 900]))),
                     "EM2_TILE_SEGMENTS": str(int(rng.choice([1, 3, 17, 256]))),
                     "EM2_BLOCKS_PER_CU": str(int(rng.choice([1, 2, 4]))),
                     "EM2_SCAN_MATRIX": str(int(rng.choice([0, 1, 1, 2, 3]))),
                     # (the convoy of the matrix walks: off, following the other blocks, or every walk n - 1 pairs of tiles in)
                     "EM2_MATRIX_CONVOY": str(int(rng.choice([0, 1, 1, 2, 3, 5, 9, 30])))}
            if os.environ.get("FUZZ_MODE"):
                knobs["EM2_SCAN_MODE"] = os.environ["FUZZ_MODE"] if os.environ["FUZZ_MODE"] != "virtual" else knobs["EM2_SCAN_MODE"] if knobs["EM2_SCAN_MODE"].startswith("virtual") else "virtual:2"
                knobs["EM2_SCAN_MATRIX"] = "1"
            os.environ.update(knobs)
            label.update(knobs)
            cell, sim, used = oracle.find_similar_pairs4(sig, L, k, thr)
            pairs, gused = capi.find_similar_pairs4(sig, L, k, thr)
        elif what == "fsp5":
            if not os.environ.get("FUZZ_WIDTHS"):
                L = int(rng.choice(FSP5_WIDTHS))
                sig = synth.clustered_signatures(n, L, cluster_count=clusters, flip=flip, seed=sig_seed)
            q = int(rng.choice([1, 3, 8, 13, 20]))
            overflow = int(rng.choice([0, 5, 1000]))
            ranged = bool(rng.random() < 0.33)
            begin, end = sorted(int(x) for x in rng.integers(0, n + 1, size=2)) if ranged else (0, n)
            knobs = {"EM2_FSP5_BATCH_LOG2": str(int(rng.choice([20, 22, 29]))), "EM2_SCRATCH_CACHE_MB": str(int(rng.choice([0, 1, 4096])))}
            os.environ.update(knobs)
            label.update(L=L, q=q, overflow=overflow, rows=[begin, end] if ranged else None, **knobs)
            if ranged:
                # the device entry on a row range, against the oracle's rows of that range
                cell, sim, used = oracle.find_similar_pairs5_rows(sig, L, k, thr, q, overflow, begin, end)
                pairs, gused = fsp5_rows(sig, L, k, thr, q, overflow, begin, end)
                runs["fsp5_ranged"] += 1
            else:
                cell, sim, used = oracle.find_similar_pairs5(sig, L, k, thr, q, overflow)
                pairs, gused = capi.find_similar_pairs5(sig, L, k, thr, q, overflow)
            if begin < end:
                info = capi.dev_find_similar_pairs5_last_launch()
                label.update(filter_form=info["filter_form"], union_form=info["union_form"], union_passes=info["union_passes"],
                             packed=info["packed"], batches=info["batches"])
            for key in knobs:
                os.environ.pop(key, None)
        elif what == "fsp6":
            rows = fsp6_case(rng, restatement6, runs, label)
            if rows is None:
                continue
            n, sig = label["n"], label.pop("sig")
            args = (label["L"], k, thr, label["P"], label["S"], label["pbits"], label["seed"])
            pairs, gused = capi.find_similar_pairs6(sig, *args)
            cell, sim, used = restatement6.find_similar_pairs6(sig, *args, rows=rows)
            pairs, gused = pairs[rows], gused[rows]
        elif what == "fsp7":
            # cell counts past the 8192 waves of the traversal (a wave then serves several rows), and k at its limit
            cells7 = int(rng.choice([n, n, n, 9000, 20000]))
            if cells7 != n:
                n = cells7
                sig = synth.clustered_signatures(n, L, cluster_count=clusters, flip=flip, seed=sig_seed)
            k = int(rng.choice([k, k, k, k, 4096]))
            lengths = sorted(set(int(x) for x in rng.choice([1, 2, 5, 8, 13, 16, 24, 33, 39, 40, 64], size=int(rng.integers(1, 4)))), reverse=True)
            max_check = int(rng.choice([0, 1, 7, 100, 100000]))
            log2b = int(rng.choice([1, 4, 10, 16, 24, 40]))
            if thr <= -1.0:
                thr = -0.9            # the reference asserts when no mismatch count is below the threshold
            ranged = bool(rng.random() < 0.5)
            begin, end = sorted(int(x) for x in rng.integers(0, n + 1, size=2)) if ranged else (0, n)
            label.update(n=n, k=k, lengths=lengths, max_check=max_check, log2b=log2b, thr=thr, rows=[begin, end] if ranged else None)
            if fsp7_oracle_is_slow(n, L, k, lengths, max_check, log2b):
                runs["fsp7_skipped"] += 1
                continue
            cell, sim, used = oracle.find_similar_pairs7(sig, L, k, thr, lengths, max_check, log2b)
            if ranged:
                # the device entry on a row range, against the oracle's rows of that range
                cell, sim, used = cell[begin:end], sim[begin:end], used[begin:end]
                pairs, gused = fsp7_rows(sig, L, k, thr, lengths, max_check, log2b, begin, end)
                runs["fsp7_ranged"] += 1
            else:
                pairs, gused = capi.find_similar_pairs7(sig, L, k, thr, lengths, max_check, log2b)
        elif what == "graph":
            cell, sim, used = oracle.find_similar_pairs4(sig, L, k, min(thr, 0.2))
            total = n + int(rng.integers(0, n + 1))
            sp_cells = np.sort(rng.choice(total, n, replace=False)).astype(np.uint32)
            graph_cells = rng.permutation(total)[:int(rng.integers(1, total + 1))].astype(np.uint32)
            g_thr = float(rng.choice([-1.0, 0.0, 0.3, 0.5, 0.9]))
            max_conn = int(rng.choice([0, 1, 3, 20, 1000]))
            expect = oracle.cell_graph_edges(cell, sim, used, sp_cells, graph_cells, g_thr, max_conn)
            pairs = np.zeros(cell.shape, dtype=capi.PAIR_DTYPE)
            pairs["cell"] = cell
            pairs["similarity"] = sim
            got = capi.cell_graph_edges(pairs, used, sp_cells, graph_cells, g_thr, max_conn)
            if not all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(expect, got)):
                raise SystemExit("PARITY FAILURE graph %r" % dict(label, g_thr=g_thr, max_conn=max_conn))
            runs[what] += 1
            continue
        else:
            cells, genes = int(rng.choice([1, 50, 300, 1000])), int(rng.choice([1, 10, 200, 1500]))
            toc, g, c = synth.expression_matrix(cells, genes, density=float(rng.choice([0.0, 0.01, 0.2])), cluster_count=3,
                                                seed=int(rng.integers(1 << 30)))
            vectors = oracle.generate_lsh_vectors(genes, L, int(rng.integers(1 << 20)))
            expect = oracle.compute_signatures(toc, g, c, genes, vectors, L)
            got = capi.compute_signatures(toc, capi.make_counts(g, c), genes, vectors, L)
            if not np.array_equal(expect, got):
                raise SystemExit("PARITY FAILURE signatures %r" % dict(cells=cells, genes=genes, L=L))
            runs[what] += 1
            continue
        ok = (np.array_equal(gused, used) and np.array_equal(pairs["cell"], cell) and
              np.array_equal(pairs["similarity"].view(np.uint32), sim.view(np.uint32)))
        if not ok:
            # which rows, and where in them (the first few)
            rows = np.nonzero((gused != used) | (pairs["cell"] != cell).any(axis=1) |
                              (pairs["similarity"].view(np.uint32) != sim.view(np.uint32)).any(axis=1))[0]
            print("differing rows: %d of %d, first %s" % (len(rows), len(used), rows[:12].tolist()))
            for r in rows[:4]:
                print(" row %d: used %d / expected %d; cells %s / expected %s" % (r, gused[r], used[r], pairs["cell"][r][:12].tolist(),
                                                                                 cell[r][:12].tolist()))
            raise SystemExit("PARITY FAILURE %s %r" % (what, label))
        runs[what] += 1
    print("fuzz ok", runs)


def expression_leg(rng, name, references, runs):
    """One draw of tests/expression_cases.py for the leg `name`: run, skipped (too slow for the CPU side) or discarded."""
    entry = expression_cases.ENTRIES[name]
    case = entry.draw(rng)
    if not expression_cases.runnable(name, case):
        runs[name + "_skipped"] += 1
        return
    if name not in references:
        references[name] = entry.reference()
    try:
        difference = entry.check(case, references[name])
    except expression_cases.Discarded:
        runs[name + "_discarded"] += 1
        return
    except AssertionError as e:
        raise SystemExit("PARITY FAILURE %s %r: %s" % (name, case, e))
    if difference:
        print(difference)
        raise SystemExit("PARITY FAILURE %s %r" % (name, case))
    runs[name] += 1


WRITE_LEGS = ("csv_parse", "ingest")


def write_leg(rng, name, runs):
    """One draw of tests/ingest_limit_cases.py for the write path: em2_dev_csv_parse against its model, or the two ingest passes
    against their restatement.  Nothing is skipped or discarded."""
    import torch
    import csv_binding
    import ingest_binding
    import ingest_limit_cases
    lib = capi.load()
    if name == "csv_parse":
        case = ingest_limit_cases.draw_csv_parse(rng)
        lib.em2_set_csv_tile_bytes(case["tile"])
        try:
            csv_binding.assert_parse(torch, case["text"], case["separators"], case["columns"], case["kept"], "fuzz",
                                     misalign=case["misalign"])
        except AssertionError as e:
            raise SystemExit("PARITY FAILURE csv_parse %r: %s" % (case, e))
        finally:
            lib.em2_set_csv_tile_bytes(0)
    else:
        case = ingest_limit_cases.draw_ingest(rng)
        lib.em2_set_ingest_lds_row_limit(case["lds_limit"])
        try:
            csr = ingest_binding.Csr.from_arrays(case["indptr"], case["indices"], case["values"], case["skip"])
            ingest_binding.assert_same(torch, csr, ingest_limit_cases.gene_map(), "fuzz")
        except AssertionError as e:
            label = {key: case[key] for key in ("lds_limit", "seed", "kind", "order")}
            raise SystemExit("PARITY FAILURE ingest %r, row lengths %r: %s" % (label, np.diff(case["indptr"].astype(np.int64)).tolist(), e))
        finally:
            lib.em2_set_ingest_lds_row_limit(0)
    runs[name] += 1


def fsp7_oracle_is_slow(n, L, k, lengths, max_check, log2b):
    """True for a draw with one of the large values (more than 4000 cells, k = 4096) that the CPU oracle would take more than
    a few seconds for; the draws of the smaller ranges are never skipped.  The bounds: cells * k at most 4300 * 4096 (the
    k = 4096 case of tests/test_gpu_fsp7.py, about 3 s); (table, cell) keys at most 3 * 10^7; cells * candidates * signature
    words at most 2 * 10^9 popcounts; and, where maxCheck does not end the walk, cells * the bucket members a cell walks
    past (buckets taken as evenly filled) at most 2 * 10^9 -- 4 * 10^9 of them were measured at 12 s."""
    if n <= 4000 and k != 4096:
        return False
    tables = sum(L // length for length in lengths)
    candidates = n if max_check == 0 else min(max_check, n)
    walked = sum((L // length) * max(1.0, n / 2.0 ** min(length, log2b)) for length in lengths) if candidates == n else candidates
    return (n * k > 4300 * 4096 or tables * n > 3 * 10 ** 7 or n * candidates * ((L - 1) // 64 + 1) > 2 * 10 ** 9 or
            n * walked > 2 * 10 ** 9)


def fsp5_rows(sig, L, k, thr, q, overflow, begin, end):
    """capi.dev_find_similar_pairs5 for rows [begin, end), as fsp7_rows."""
    import torch
    rows = end - begin
    d_sig = torch.from_numpy(sig.view(np.int64)).cuda()
    d_pairs = torch.full((max(rows, 1), k, 2), 0x5a5a5a5a, dtype=torch.int32, device="cuda")
    d_used = torch.full((max(rows, 1),), 0x5a5a5a5a, dtype=torch.int32, device="cuda")
    capi.dev_find_similar_pairs5(d_sig.data_ptr(), len(sig), begin, end, L, k, thr, q, overflow, d_pairs.data_ptr(),
                                 d_used.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    pairs = d_pairs.cpu().numpy().view(capi.PAIR_DTYPE)[:rows, :, 0]
    return pairs, d_used.cpu().numpy().view(np.uint32)[:rows]


def fsp7_rows(sig, L, k, thr, lengths, max_check, log2b, begin, end):
    """capi.dev_find_similar_pairs7 for rows [begin, end) with torch supplying the device memory; the outputs are filled with
    a non-zero pattern first.  Returns (pairs [rows, k], usedCount) as host arrays."""
    import torch
    rows = end - begin
    d_sig = torch.from_numpy(sig.view(np.int64)).cuda()
    d_pairs = torch.full((max(rows, 1), k, 2), 0x5a5a5a5a, dtype=torch.int32, device="cuda")
    d_used = torch.full((max(rows, 1),), 0x5a5a5a5a, dtype=torch.int32, device="cuda")
    capi.dev_find_similar_pairs7(d_sig.data_ptr(), len(sig), begin, end, L, k, thr, lengths, max_check, log2b, d_pairs.data_ptr(),
                                 d_used.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    pairs = d_pairs.cpu().numpy().view(capi.PAIR_DTYPE)[:rows, :, 0]
    return pairs, d_used.cpu().numpy().view(np.uint32)[:rows]


def fsp6_case(rng, restatement, runs, label):
    """Draws a findSimilarPairs6 case into `label` (n, L, P, S, pbits, seed and the signatures under "sig") and returns the
    rows to compare, or None when the case lies past the kernels' limits and was answered EM2_ERROR_UNSUPPORTED as it
    must be.  Large cases (several row chunks: more than 2^27 / effective-search rows) compare sampled rows that include
    both sides of every chunk edge."""
    big = rng.random() < 0.12
    if big:
        n = int(rng.choice([16385, 20000, 32769, 40000]))
        L = int(rng.choice([64, 128, 256, 1024]))
        P = int(rng.choice([1, 2, 4, 8]))
        S = int(rng.choice([4097, 5000, 8192, 10 ** 6]))
        pbits = int(rng.choice([1, 63, 64, 65, min(L, 128)]))
    else:
        n = int(rng.choice([1, 2, 3, 63, 64, 65, 129, 200, 257, 600, 1000, 2500]))
        L = int(rng.choice([1, 63, 64, 65, 100, 127, 129, 256, 1024, 2048, 4095, 4096]))
        P = int(rng.choice([1, 2, 5, 16, 33, 63, 64, 64, 65]))
        S = int(rng.choice([1, 10, 100, 400, 1025, 4097, 8191, 8192, 8193, 10 ** 6]))
        pbits = int(rng.choice([1, 63, 64, 65, 128, L - 1, L, int(rng.integers(1, L + 1))]))
    pbits = pbits if 1 <= pbits <= L else L
    seed = int(rng.integers(-2 ** 31, 2 ** 31))
    clusters = int(rng.choice([1, 2, 5, 20]))
    flip = float(rng.choice([0.0, 0.002, 0.02, 0.1, 0.3]))
    sig_seed = int(rng.integers(1 << 30))
    sig = synth.clustered_signatures(n, L, cluster_count=clusters, flip=flip, seed=sig_seed)
    label.update(n=n, L=L, P=P, S=S, pbits=pbits, seed=seed, clusters=clusters, flip=flip, sig_seed=sig_seed)
    effective = min(S, P * (n - 1))
    if P > 64 or effective > 8192:
        try:
            capi.find_similar_pairs6(sig, L, 5, 0.2, P, S, pbits, seed)
        except RuntimeError as e:
            if "not supported" not in str(e):
                raise SystemExit("PARITY FAILURE fsp6: %s %r" % (e, label))
            runs["fsp6_unsupported"] += 1
            return None
        raise SystemExit("PARITY FAILURE fsp6: accepted past the limits %r" % label)
    if S >= 8192 and effective == 8192:
        runs["fsp6_clamp8192"] += 1
    chunk = max(64, (1 << 30) // (max(effective, 1) * 8))
    if n > chunk:
        runs["fsp6_chunks"] += 1
    label["sig"] = sig
    if n * max(effective, 1) * max(1, L // 512) <= 4_000_000:
        return np.arange(n, dtype=np.uint32)
    edges = [0, n - 1] + [e + d for e in range(chunk, n, chunk) for d in (-2, -1, 0, 1)]
    sample = rng.choice(n, size=min(n, 192), replace=False)
    return np.union1d(np.array([e for e in edges if 0 <= e < n]), sample).astype(np.uint32)


if __name__ == "__main__":
    main()
