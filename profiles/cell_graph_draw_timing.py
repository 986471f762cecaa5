"""Timing of the colouring values and of the raster (csrc/em2_cell_values.hip, csrc/em2_draw.hip) on the cell
graphs of profiles/layout_timing.py (the bench's generator, threshold 0.2, at most 20 edges per vertex) at 10^5 and 10^6 cells:

    python profiles/cell_graph_draw_timing.py [--vertices 100000 1000000] [--genes 30000] [--limit 900] [--output DIR]

Writes the record of every size to DIR/cell_graph_draw_timing_<vertices>.json and prints one JSON line with all of them.  Per
size, in ONE process and everything in device memory: the graph is laid out (multilevel, pyramid), then after one warm-up call
each, ONE call each of em2_dev_cell_similarities_to_cell (every cell against cell 0), em2_dev_gene_expression_of_cells (L2,
the gene most cells store), em2_dev_spectral_colors of the similarities, and em2_dev_graph_draw and em2_dev_graph_compose at
1024^2 and 4096^2 pixels with the page's default view is timed (the two that do not synchronise, with a synchronisation), and
the same is computed by tests/native/em2_draw_restatement.cpp on one thread of the same box.  The results of the two are compared
(NaNs at the same places, everything else equal) and the record says so.
One process uses the GPU at a time: each size is a child process under a time limit of its own; where one fails nothing more is
started."""
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
sys.path.insert(0, os.path.join(ROOT, "profiles"))
sys.path.insert(0, os.path.join(ROOT, "tests"))


def seconds_of(call):
    begin = time.perf_counter()
    returned = call()
    return time.perf_counter() - begin, returned


def same(got, expected):
    got, expected = np.asarray(got), np.asarray(expected)
    nan = np.isnan(got)
    return bool(np.array_equal(nan, np.isnan(expected)) and np.array_equal(got[~nan], expected[~nan]))


def child(args):
    import torch
    import draw_binding
    from expressionmatrix2_amd import capi, synthetic
    from layout_timing import cell_graph
    n = args.child
    lib = capi.load()
    restatement = draw_binding.load()
    d_v0, d_v1, edges = cell_graph(n, args.genes)
    toc, data = synthetic.expression_shard(0, n, args.genes, density=0.01, device="cuda")
    d_x32 = torch.zeros(n, dtype=torch.float32, device="cuda")
    d_y32 = torch.zeros(n, dtype=torch.float32, device="cuda")
    parameters, result, levels = capi.LayoutParameters(), capi.LayoutResult(), capi.LayoutLevels()
    capi.check(lib.em2_dev_graph_layout_multilevel(n, d_v0.data_ptr(), d_v1.data_ptr(), edges, ctypes.byref(parameters),
                                                   capi.LAYOUT_DEPTH_AUTO, d_x32.data_ptr(), d_y32.data_ptr(), ctypes.byref(result),
                                                   ctypes.byref(levels)))
    d_x, d_y = d_x32.double(), d_y32.double()
    torch.cuda.synchronize()
    record = {"vertices": n, "edges": int(edges), "genes": args.genes, "stored_entries": int(data.numel())}

    h_toc, h_genes, h_counts = synthetic.csr_to_host(toc, data)
    h_data = capi.make_counts(h_genes, h_counts)
    ids = np.arange(n, dtype=np.uint32)

    # the values
    d_similarity = torch.zeros(n, dtype=torch.float64, device="cuda")
    workspace_bytes = lib.em2_dev_cell_similarities_to_cell_workspace(args.genes, n)
    d_workspace = torch.zeros(max(workspace_bytes, lib.em2_dev_gene_expression_of_cells_workspace()), dtype=torch.uint8, device="cuda")

    def similarities():
        capi.check(lib.em2_dev_cell_similarities_to_cell(toc.data_ptr(), data.data_ptr(), n, None, 0, args.genes, 0, None, n,
                                                         d_similarity.data_ptr(), d_workspace.data_ptr(), d_workspace.numel(), None))
    similarities()
    record["similarities_seconds"] = seconds_of(similarities)[0]
    record["similarities_restatement_seconds"], expected = seconds_of(
        lambda: restatement.cell_similarities(h_toc, h_data, args.genes, 0, ids))
    record["similarities_equal"] = same(d_similarity.cpu().numpy(), expected)
    record["row_vector_in_lds"] = capi.cell_similarities_row_in_lds(args.genes)

    gene = int(np.argmax(np.bincount(h_genes, minlength=args.genes)))
    d_column = torch.zeros(n, dtype=torch.float32, device="cuda")

    def column():
        capi.check(lib.em2_dev_gene_expression_of_cells(toc.data_ptr(), data.data_ptr(), n, None, 0, args.genes, gene, 2, None, n,
                                                        d_column.data_ptr(), d_workspace.data_ptr(), d_workspace.numel(), None))
    column()
    record["gene_column_seconds"] = seconds_of(column)[0]
    record["gene_column_restatement_seconds"], expected = seconds_of(lambda: restatement.gene_expression(h_toc, h_data, gene, 2, ids))
    record["gene_column_equal"] = same(d_column.cpu().numpy(), expected)
    record["gene_column_cells_storing_the_gene"] = int(np.count_nonzero(expected))

    # the colours of the similarities (em2_dev_spectral_colors does not synchronise: the timed call ends with one)
    d_rgb = torch.zeros(n, dtype=torch.int32, device="cuda")
    d_range = torch.zeros(4, dtype=torch.float64, device="cuda")
    d_color_workspace = torch.zeros(lib.em2_dev_spectral_colors_workspace(), dtype=torch.uint8, device="cuda")

    def colors():
        capi.check(lib.em2_dev_spectral_colors(d_similarity.data_ptr(), n, 0., 0., 0, 0, d_rgb.data_ptr(), d_range.data_ptr(),
                                               d_color_workspace.data_ptr(), d_color_workspace.numel(), None))
        torch.cuda.synchronize()
    colors()
    record["colors_seconds"] = seconds_of(colors)[0]
    h_similarity = d_similarity.cpu().numpy()
    record["colors_restatement_seconds"], expected = seconds_of(lambda: restatement.spectral_colors(h_similarity))
    rgb = d_rgb.cpu().numpy().view(np.uint32)
    record["colors_equal"] = bool(np.array_equal(rgb, expected[0]) and np.array_equal(d_range.cpu().numpy(), expected[1]))

    # the raster, with the page's default view
    x, y = d_x.cpu().numpy(), d_y.cpu().numpy()
    v0, v1 = d_v0[:edges].cpu().numpy().view(np.uint32), d_v1[:edges].cpu().numpy().view(np.uint32)
    d_draw_workspace = torch.zeros(lib.em2_dev_graph_draw_workspace(n, edges), dtype=torch.uint8, device="cuda")
    record["draw"] = []
    for size in (1024, 4096):
        xc, yc, half, radius, _ = draw_binding.python_default_view(x, y, float(size))
        d_top = torch.zeros((size, size), dtype=torch.int32, device="cuda")
        d_hits = torch.zeros((size, size), dtype=torch.int32, device="cuda")

        def draw():
            capi.check(lib.em2_dev_graph_draw(n, d_x.data_ptr(), d_y.data_ptr(), edges, d_v0.data_ptr(), d_v1.data_ptr(), 0, size, xc, yc,
                                              half, radius, d_top.data_ptr(), d_hits.data_ptr(), d_draw_workspace.data_ptr(),
                                              d_draw_workspace.numel(), None))
        draw()
        entry = {"size_pixels": size, "seconds": seconds_of(draw)[0]}
        entry["restatement_seconds"], expected = seconds_of(lambda: restatement.graph_draw(x, y, v0, v1, size, xc, yc, half, radius))
        top, hits = d_top.cpu().numpy().view(np.uint32), d_hits.cpu().numpy().view(np.uint32)
        entry["equal"] = bool(np.array_equal(top, expected[0]) and np.array_equal(hits, expected[1]))
        d_rgba = torch.zeros((size, size), dtype=torch.int32, device="cuda")

        def compose():
            capi.check(lib.em2_dev_graph_compose(size, d_top.data_ptr(), d_hits.data_ptr(), d_rgb.data_ptr(), 255, d_rgba.data_ptr(), None))
            torch.cuda.synchronize()
        compose()
        entry["compose_seconds"] = seconds_of(compose)[0]
        entry["compose_restatement_seconds"], image = seconds_of(lambda: restatement.graph_compose(top, hits, rgb, 255))
        entry["compose_equal"] = bool(np.array_equal(d_rgba.cpu().numpy().view(np.uint8).reshape(size, size, 4), image))
        entry["edge_steps"] = int(hits.sum(dtype=np.uint64))
        entry["most_hits_on_a_pixel"] = int(hits.max())
        entry["pixels_under_a_vertex"] = int(np.count_nonzero(top))
        record["draw"].append(entry)
    print(json.dumps(record))


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--vertices", type=int, nargs="+", default=[100000, 1000000])
    parser.add_argument("--genes", type=int, default=30000)
    parser.add_argument("--limit", type=int, default=900, help="time limit of the GPU step of one size in seconds")
    parser.add_argument("--output", default=os.path.join(ROOT, "profiles"), help="the directory of the JSON files")
    parser.add_argument("--child", type=int, default=None)
    args = parser.parse_args()
    if args.child:
        return child(args)
    sizes = []
    for n in args.vertices:
        command = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--child", str(n), "--genes",
                   str(args.genes)]
        done = subprocess.run(command, capture_output=True, text=True)
        if done.returncode != 0:
            sys.stderr.write(done.stderr[-4000:])
            raise SystemExit("the GPU step of %d vertices ended with status %d: nothing more is started" % (n, done.returncode))
        sizes.append(json.loads(done.stdout.strip().splitlines()[-1]))
        with open(os.path.join(args.output, "cell_graph_draw_timing_%d.json" % n), "w") as out:
            json.dump(sizes[-1], out, indent=1)
            out.write("\n")
    print(json.dumps({"sizes": sizes}))


if __name__ == "__main__":
    main()
