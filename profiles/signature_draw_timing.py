"""Timing of the signature graph's colour census, its raster with pies and the composition (csrc/em2_pie.hip) on
the graph profiles/signature_graph_timing.py makes (the bench's generator, 10^6 cells x 24 bits, minCellCount 1) with a
synthetic field of 20 values:

    python profiles/signature_draw_timing.py [--cells 1000000] [--genes 30000] [--lsh-count 24] [--repeats 5] [--limit 900]

Writes the record to profiles/signature_draw_timing_<cells>.json and prints it as one JSON line.  In ONE process, the inputs in
device memory: after one warm-up call each, R calls each of em2_dev_pie_census (the whole call, which ends with the slices in
host memory) and, at 1024^2 and 4096^2 pixels with the SVG's view, radii and painter order, of em2_dev_graph_draw_pies and
em2_dev_graph_compose (with a synchronisation; at 4096^2 also with heavy-tailed radii that span the three radius classes) are
timed by the host clock, the best is kept and all are listed; then once more
with EM2_TIMING=1, whose stages synchronise, for the split of the census into its passes and of the raster into its radius
classes.  The same is computed by tests/native/em2_signature_draw_restatement.cpp on one thread of the same box, the results are
compared and the record says whether they are equal.
One process uses the GPU at a time: the GPU step is a child process under a time limit of its own; where it fails nothing more
is started."""
import argparse
import ctypes
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

VALUES = 20


def seconds_of(call):
    begin = time.perf_counter()
    returned = call()
    return time.perf_counter() - begin, returned


def timed(call, repeats):
    call()                                                       # warm-up
    return [seconds_of(call)[0] for _ in range(repeats)]


def child(args):
    import torch
    import signature_draw_binding as sb
    from expressionmatrix2_amd import capi, sharded, synthetic
    lib = capi.load()
    restatement = sb.load()
    pipe = sharded.DevicePipeline(args.cells, args.genes, args.lsh_count, 1, 0.2, world_size=1, rank=0, dist=None, device="cuda")
    toc, data = synthetic.expression_shard(0, args.cells, args.genes, density=args.density)
    pipe.set_inputs(toc, data, torch.from_numpy(capi.lsh_generate_vectors(args.genes, args.lsh_count, 231)).to("cuda"))
    pipe.project()
    torch.cuda.synchronize()
    signatures = pipe.full_sig[:args.cells].contiguous()
    handle = ctypes.c_void_p(None)
    capi.check(lib.em2_dev_signature_graph_create(signatures.data_ptr(), args.cells, args.lsh_count, 1, ctypes.byref(handle)))
    graph = capi.signature_graph_take(handle)
    del pipe, toc, data, signatures
    offsets, cells, v0, v1 = graph["cellOffsets"], graph["cells"], graph["edgeVertex0"], graph["edgeVertex1"]
    vertices, edges = len(offsets) - 1, len(v0)
    counts = np.diff(offsets)
    record = {"cells": args.cells, "lsh_count": args.lsh_count, "vertices": vertices, "edges": edges, "values": VALUES,
              "most_cells_in_a_vertex": int(counts.max()), "census_wave_cells": capi.pie_census_wave_cells(),
              "vertices_above_the_census_threshold": int((counts > capi.pie_census_wave_cells()).sum()), "repeats": args.repeats}

    # a field of 20 values with unequal shares; the colour of a value from its rank, as the host does it
    rng = np.random.default_rng(231)
    ids = rng.choice(VALUES, args.cells, p=np.arange(VALUES, 0, -1) / (VALUES * (VALUES + 1) / 2)).astype(np.uint32)
    order = capi.order_by_count(np.bincount(ids[cells], minlength=VALUES).astype(np.uint64))
    colors = np.zeros(VALUES, dtype=np.uint8)
    colors[order] = np.minimum(np.arange(VALUES), 12)
    device = lambda a, kind: torch.from_numpy(np.ascontiguousarray(a).view(kind).copy()).cuda()
    d_offsets, d_cells, d_ids, d_colors = device(offsets, np.int64), device(cells, np.int32), device(ids, np.int32), device(colors, np.uint8)
    census = {}

    def run_census():
        handle = ctypes.c_void_p(None)
        capi.check(lib.em2_dev_pie_census(vertices, d_offsets.data_ptr(), d_cells.data_ptr(), len(cells), d_ids.data_ptr(), len(ids),
                                          d_colors.data_ptr(), VALUES, ctypes.byref(handle)))
        census.update(capi.pie_census_take(handle))
    record["census_seconds_all"] = timed(run_census, args.repeats)
    record["census_seconds"] = min(record["census_seconds_all"])
    record["census_restatement_seconds"], expected = seconds_of(lambda: restatement.census(offsets, cells, ids, colors))
    record["census_equal"] = all(census[key].tobytes() == expected[key].tobytes() for key in ("sliceOffsets", "sliceColor", "sliceCells", "sliceFraction"))
    record["slices"] = int(len(census["sliceColor"]))
    record["census_wave_vertices"] = census["waveVertexCount"]
    # what the passes read and write at the least: offsets, cells, an id and a colour per cell twice; counts, offsets and slices once
    record["census_bytes_at_least"] = int(2 * (8 * vertices + 4 * len(cells) * 2 + len(cells)) + 4 * vertices + 8 * vertices * 2 +
                                          13 * record["slices"] * 2)
    os.environ["EM2_TIMING"] = "1"
    print("[stage run] census", file=sys.stderr, flush=True)
    run_census()
    os.environ["EM2_TIMING"] = "0"

    # the layout, then the SVG's view, radii and painter order
    d_v0, d_v1 = device(v0, np.int32), device(v1, np.int32)
    d_x32 = torch.zeros(vertices, dtype=torch.float32, device="cuda")
    d_y32 = torch.zeros(vertices, dtype=torch.float32, device="cuda")
    parameters, result, levels = capi.LayoutParameters(), capi.LayoutResult(), capi.LayoutLevels()
    record["layout_seconds"] = seconds_of(lambda: capi.check(lib.em2_dev_graph_layout_multilevel(
        vertices, d_v0.data_ptr(), d_v1.data_ptr(), edges, ctypes.byref(parameters), capi.LAYOUT_DEPTH_AUTO, d_x32.data_ptr(),
        d_y32.data_ptr(), ctypes.byref(result), ctypes.byref(levels))))[0]
    x, y = d_x32.double().cpu().numpy(), d_y32.double().cpu().numpy()
    painter = capi.order_by_count(counts).astype(np.int64)
    position = np.empty(vertices, dtype=np.uint32)
    position[painter] = np.arange(vertices, dtype=np.uint32)
    slice_offsets = census["sliceOffsets"].astype(np.int64)
    slice_counts = np.diff(slice_offsets)[painter]
    new_offsets = np.concatenate([[0], np.cumsum(slice_counts)]).astype(np.int64)
    gather = np.repeat(slice_offsets[:-1][painter] - new_offsets[:-1], slice_counts) + np.arange(int(new_offsets[-1]), dtype=np.int64)
    record["boundaries_seconds_host"], (bx, by, arc) = seconds_of(lambda: capi.pie_boundaries(new_offsets, census["sliceFraction"][gather]))
    rgb = sb.slice_rgb(census["sliceColor"])[gather]
    x, y, v0, v1 = x[painter], y[painter], position[v0], position[v1]
    d_x, d_y = device(x, np.float64), device(y, np.float64)
    d_v0, d_v1 = device(v0, np.int32), device(v1, np.int32)
    d_slices, d_bx, d_by, d_arc = device(new_offsets, np.int64), device(bx, np.int32), device(by, np.int32), device(arc, np.uint8)
    d_rgb = device(rgb, np.int32)
    d_workspace = torch.zeros(lib.em2_dev_graph_draw_pies_workspace(vertices, edges), dtype=torch.uint8, device="cuda")
    record["draw"] = []
    # the graph's own cell counts, whose radii span a factor of two here, and at 4096^2 once more with cell counts of a heavy
    # tail (P(count >= k) = 1 / k, at most 10^6) in the same vertex order, so that the radii span all three classes
    heavy = np.minimum(1e6, np.floor(1. / (1. - rng.random(vertices))))
    for size, sizes, label in ((1024, counts[painter].astype(np.float64), "the graph's cell counts"),
                               (4096, counts[painter].astype(np.float64), "the graph's cell counts"),
                               (4096, heavy, "heavy-tailed cell counts, not in painter order")):
        xc, yc, half, _, box = sb.python_signature_view(x, y, counts, float(size))
        radius = 0.03 * box * np.sqrt(sizes / float(sizes.max()))
        d_radius = device(radius, np.float64)
        pixels = radius * (size / (2. * half))
        d_top, d_slice, d_hits, d_rgba = [torch.zeros((size, size), dtype=torch.int32, device="cuda") for _ in range(4)]

        def draw():
            capi.check(lib.em2_dev_graph_draw_pies(vertices, d_x.data_ptr(), d_y.data_ptr(), d_radius.data_ptr(), edges, d_v0.data_ptr(),
                                                   d_v1.data_ptr(), 0, size, xc, yc, half, d_slices.data_ptr(), len(bx), d_bx.data_ptr(),
                                                   d_by.data_ptr(), d_arc.data_ptr(), d_top.data_ptr(), d_slice.data_ptr(),
                                                   d_hits.data_ptr(), d_workspace.data_ptr(), d_workspace.numel(), None))

        def compose():
            capi.check(lib.em2_dev_graph_compose(size, d_slice.data_ptr(), d_hits.data_ptr(), d_rgb.data_ptr(), 255, d_rgba.data_ptr(), None))
            torch.cuda.synchronize()
        entry = {"size_pixels": size, "radii_from": label, "seconds_all": timed(draw, args.repeats), "compose_seconds_all": timed(compose, args.repeats),
                 "vertices_by_class": [int((pixels <= 4.).sum()), int(((pixels > 4.) & (pixels <= capi.graph_draw_pies_wave_radius())).sum()),
                                       int((pixels > capi.graph_draw_pies_wave_radius()).sum())],
                 "smallest_radius_pixels": float(pixels.min()), "largest_radius_pixels": float(pixels.max())}
        entry["seconds"], entry["compose_seconds"] = min(entry["seconds_all"]), min(entry["compose_seconds_all"])
        os.environ["EM2_TIMING"] = "1"
        print("[stage run] draw %d, %s" % (size, label), file=sys.stderr, flush=True)
        draw()
        os.environ["EM2_TIMING"] = "0"
        entry["restatement_seconds"], expected = seconds_of(
            lambda: restatement.graph_draw_pies(x, y, radius, v0, v1, size, xc, yc, half, new_offsets, bx, by, arc))
        layers = [d.cpu().numpy().view(np.uint32) for d in (d_top, d_slice, d_hits)]
        entry["equal"] = bool(all(np.array_equal(a, b) for a, b in zip(layers, expected)))
        import draw_binding
        entry["compose_restatement_seconds"], image = seconds_of(lambda: draw_binding.load().graph_compose(layers[1], layers[2], rgb, 255))
        entry["compose_equal"] = bool(np.array_equal(d_rgba.cpu().numpy().view(np.uint8).reshape(size, size, 4), image))
        entry["pixels_under_a_vertex"] = int(np.count_nonzero(layers[0]))
        record["draw"].append(entry)
    print(json.dumps(record))


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--cells", type=int, default=1000000)
    parser.add_argument("--genes", type=int, default=30000)
    parser.add_argument("--density", type=float, default=0.01)
    parser.add_argument("--lsh-count", type=int, default=24)
    parser.add_argument("--repeats", type=int, default=5)
    parser.add_argument("--limit", type=int, default=900, help="time limit of the GPU step in seconds")
    parser.add_argument("--output", default=os.path.join(ROOT, "profiles"), help="the directory of the JSON file")
    parser.add_argument("--child", action="store_true")
    args = parser.parse_args()
    if args.child:
        return child(args)
    command = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--child"] + \
              ["--%s=%s" % (name.replace("_", "-"), getattr(args, name)) for name in ("cells", "genes", "density", "lsh_count", "repeats")]
    done = subprocess.run(command, capture_output=True, text=True)
    if done.returncode != 0:
        sys.stderr.write(done.stderr[-4000:])
        raise SystemExit("the GPU step ended with status %d: nothing more is started" % done.returncode)
    record = json.loads(done.stdout.strip().splitlines()[-1])
    # the stage lines of the runs with EM2_TIMING=1, by the marker that precedes them
    stages, section = {}, None
    for line in done.stderr.splitlines():
        marker = re.match(r"\[stage run\] (.*)", line)
        if marker:
            section = marker.group(1)
            continue
        stage = re.match(r"\[em2 timing\] (pieCensus|graphDrawPies): (.*?) ([0-9.]+) ms", line)
        if stage and section:
            stages.setdefault(section, {})[stage.group(2)] = float(stage.group(3)) / 1000.
    record["stage_seconds_one_synchronised_call"] = stages
    with open(os.path.join(args.output, "signature_draw_timing_%d.json" % args.cells), "w") as out:
        json.dump(record, out, indent=1)
        out.write("\n")
    print(json.dumps(record))


if __name__ == "__main__":
    main()
