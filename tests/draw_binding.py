"""ctypes binding of tests/native/em2_draw_restatement.cpp (the values per cell, the colours from numbers, the raster, its
composition and the SVG text of a laid-out graph, one thread and plain loops), an independent numpy / Python statement of the
same definitions, and what the drawing tests share.  Compiled with g++ at first use.  Test infrastructure only."""
import ctypes
import functools
import math
import os
import struct
import subprocess
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE_DIR = os.path.join(ROOT, "tests", "native")
SOURCE = os.path.join(NATIVE_DIR, "em2_draw_restatement.cpp")
COUNT_DTYPE = np.dtype([("gene", "<u4"), ("count", "<f4")])
NO_VALUE = float(np.finfo(np.float64).max)
COLOR_NONE, COLOR_BLACK = 0x80000000, 0x40000000
PALETTE = ("#00ff00", "#0000ff", "#ffff00", "#ff00ff", "#00ffff", "#ff8000", "#804000", "#ffa0a0", "#308000", "#900080", "#9999ff",
           "#b0b0b0")

c = ctypes
P = c.c_void_p


def _ptr(a):
    return a.ctypes.data_as(c.c_void_p) if a is not None else None


def _packed(strings):
    return b"".join(s.encode("utf-8") + b"\0" for s in strings)


class DrawRestatement:
    def __init__(self, lib):
        self.lib = lib
        lib.em2r_cell_similarities.argtypes = [P, P, P, c.c_uint32, c.c_uint32, c.c_uint32, P, c.c_uint32, P]
        lib.em2r_cell_similarities.restype = None
        lib.em2r_gene_expression.argtypes = [P, P, P, c.c_uint32, c.c_uint32, c.c_int, P, c.c_uint32, P]
        lib.em2r_gene_expression.restype = c.c_int
        lib.em2r_spectral_colors.argtypes = [P, c.c_uint64, c.c_double, c.c_double, c.c_int, c.c_int, P, P]
        lib.em2r_spectral_colors.restype = None
        lib.em2r_graph_draw.argtypes = [c.c_uint32, P, P, c.c_uint64, P, P, c.c_int, c.c_uint32, c.c_double, c.c_double, c.c_double,
                                        c.c_double, P, P]
        lib.em2r_graph_draw.restype = c.c_int
        lib.em2r_graph_compose.argtypes = [c.c_uint32, P, P, P, c.c_uint32, P]
        lib.em2r_graph_compose.restype = None
        lib.em2r_graph_svg.argtypes = [c.c_char_p, c.c_uint32, P, P, P, c.c_uint64, P, P, c.c_int, c.c_double, c.c_double, c.c_double,
                                       c.c_double, c.c_double, c.c_double, c.c_char_p, P, c.c_uint32, P, c.c_char_p, c.c_char_p]
        lib.em2r_graph_svg.restype = c.c_int

    def cell_similarities(self, toc, data, gene_count, cell_id0, cell_ids, local_ids=None):
        toc = np.ascontiguousarray(toc, dtype=np.uint64)
        data = np.ascontiguousarray(data, dtype=COUNT_DTYPE)
        cell_ids = np.ascontiguousarray(cell_ids, dtype=np.uint32)
        local = None if local_ids is None else np.ascontiguousarray(local_ids, dtype=np.uint32)
        out = np.zeros(len(cell_ids), dtype=np.float64)
        self.lib.em2r_cell_similarities(_ptr(toc), _ptr(data), _ptr(local), 0 if local is None else len(local), gene_count, cell_id0,
                                        _ptr(cell_ids), len(cell_ids), _ptr(out))
        return out

    def gene_expression(self, toc, data, gene_id, method, cell_ids, local_ids=None):
        toc = np.ascontiguousarray(toc, dtype=np.uint64)
        data = np.ascontiguousarray(data, dtype=COUNT_DTYPE)
        cell_ids = np.ascontiguousarray(cell_ids, dtype=np.uint32)
        local = None if local_ids is None else np.ascontiguousarray(local_ids, dtype=np.uint32)
        out = np.zeros(len(cell_ids), dtype=np.float32)
        if self.lib.em2r_gene_expression(_ptr(toc), _ptr(data), _ptr(local), 0 if local is None else len(local), gene_id, int(method),
                                         _ptr(cell_ids), len(cell_ids), _ptr(out)):
            raise RuntimeError("the gene is not in the gene set")
        return out

    def spectral_colors(self, values, min_color_value=None, max_color_value=None):
        values = np.ascontiguousarray(values, dtype=np.float64)
        rgb = np.zeros(len(values), dtype=np.uint32)
        value_range = np.zeros(4, dtype=np.float64)
        self.lib.em2r_spectral_colors(_ptr(values), len(values), 0. if min_color_value is None else min_color_value,
                                      0. if max_color_value is None else max_color_value, int(min_color_value is not None),
                                      int(max_color_value is not None), _ptr(rgb), _ptr(value_range))
        return rgb, value_range

    def graph_draw(self, x, y, v0, v1, size, xc, yc, half, radius, hide_edges=False):
        """(vertexTop, edgeHits) or None for an argument error."""
        x = np.ascontiguousarray(x, dtype=np.float64)
        y = np.ascontiguousarray(y, dtype=np.float64)
        v0 = np.ascontiguousarray(v0, dtype=np.uint32)
        v1 = np.ascontiguousarray(v1, dtype=np.uint32)
        top = np.zeros((size, size), dtype=np.uint32)
        hits = np.zeros((size, size), dtype=np.uint32)
        if self.lib.em2r_graph_draw(len(x), _ptr(x), _ptr(y), len(v0), _ptr(v0), _ptr(v1), int(hide_edges), size, xc, yc, half, radius,
                                    _ptr(top), _ptr(hits)):
            return None
        return top, hits

    def graph_compose(self, top, hits, rgb, edge_shade):
        top = np.ascontiguousarray(top, dtype=np.uint32)
        hits = np.ascontiguousarray(hits, dtype=np.uint32)
        rgb = np.ascontiguousarray(rgb, dtype=np.uint32)
        rgba = np.zeros(top.shape + (4,), dtype=np.uint8)
        self.lib.em2r_graph_compose(top.shape[0], _ptr(top), _ptr(hits), _ptr(rgb), edge_shade, _ptr(rgba))
        return rgba

    def graph_svg(self, path, x, y, cell_ids, v0, v1, hide_edges, size, xc, yc, half, radius, thickness, gene_set_name, colors=None,
                  groups=None, group_colors=None):
        x = np.ascontiguousarray(x, dtype=np.float64)
        y = np.ascontiguousarray(y, dtype=np.float64)
        cell_ids = np.ascontiguousarray(cell_ids, dtype=np.uint32)
        v0 = np.ascontiguousarray(v0, dtype=np.uint32)
        v1 = np.ascontiguousarray(v1, dtype=np.uint32)
        group_colors = group_colors or {}
        ids = np.asarray(sorted(group_colors), dtype=np.int32)
        groups = None if groups is None else np.ascontiguousarray(groups, dtype=np.uint32)
        rc = self.lib.em2r_graph_svg(os.fsencode(path), len(x), _ptr(x), _ptr(y), _ptr(cell_ids), len(v0), _ptr(v0), _ptr(v1),
                                     int(hide_edges), size, xc, yc, half, radius, thickness,
                                     None if colors is None else _packed(colors), _ptr(groups), len(ids), _ptr(ids),
                                     _packed([group_colors[g] for g in sorted(group_colors)]), gene_set_name.encode("utf-8"))
        assert rc == 0
        with open(path, "rb") as f:
            return f.read()


@functools.lru_cache(maxsize=None)
def load():
    build = os.path.join(NATIVE_DIR, "build")
    os.makedirs(build, exist_ok=True)
    path = os.path.join(build, "libem2drawrestatement.so")
    if not os.path.exists(path) or os.path.getmtime(path) < os.path.getmtime(SOURCE):
        tmp = path + ".%d.tmp" % os.getpid()
        cmd = ["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-o", tmp, SOURCE]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError("draw restatement build failed: " + r.stderr)
        os.replace(tmp, path)
    return DrawRestatement(ctypes.CDLL(path))


# ---- the independent statement: sets of pixels, a loop over k, float64 numpy, '%g' ----

def python_view(size, xc, yc, half, radius):
    s256 = float(size) * 256. / (2. * half)
    return xc - half, yc - half, s256, int(math.floor(radius * s256 + 0.5))      # llround of a value that is not negative


def python_subpixels(x, y, size, xc, yc, half):
    x_min, y_min, s256, _ = python_view(size, xc, yc, half, 0.)
    limit = float(1 << 30)
    ux = np.clip(np.floor((np.asarray(x, dtype=np.float64) - x_min) * s256), -limit, limit).astype(np.int64)
    uy = np.clip(np.floor((np.asarray(y, dtype=np.float64) - y_min) * s256), -limit, limit).astype(np.int64)
    return ux.tolist(), uy.tolist()


def python_raster(x, y, v0, v1, size, xc, yc, half, radius, hide_edges=False):
    """(vertexTop, edgeHits) from a set of covered pixels per vertex and a Python loop over k per edge."""
    ux, uy = python_subpixels(x, y, size, xc, yc, half)
    R = python_view(size, xc, yc, half, radius)[3]
    top = np.zeros((size, size), dtype=np.uint32)
    hits = np.zeros((size, size), dtype=np.uint32)
    for v, (cx, cy) in enumerate(zip(ux, uy)):
        covered = {(cx >> 8, cy >> 8)}
        for j in range(max(0, (cy - R) // 256 - 1), min(size, (cy + R) // 256 + 2)):
            for i in range(max(0, (cx - R) // 256 - 1), min(size, (cx + R) // 256 + 2)):
                if (256 * i + 128 - cx) ** 2 + (256 * j + 128 - cy) ** 2 <= R * R:
                    covered.add((i, j))
        for i, j in covered:
            if 0 <= i < size and 0 <= j < size:
                top[j, i] = max(int(top[j, i]), v + 1)
    if not hide_edges:
        for a, b in zip(np.asarray(v0).tolist(), np.asarray(v1).tolist()):
            i0, j0, i1, j1 = ux[a] >> 8, uy[a] >> 8, ux[b] >> 8, uy[b] >> 8
            dx, dy = i1 - i0, j1 - j0
            major_is_x = abs(dx) >= abs(dy)
            dM, dm = (abs(dx), abs(dy)) if major_is_x else (abs(dy), abs(dx))
            sM = -1 if (dx if major_is_x else dy) < 0 else 1
            sm = -1 if (dy if major_is_x else dx) < 0 else 1
            for k in range(dM + 1):
                major = (i0 if major_is_x else j0) + sM * k
                minor = (j0 if major_is_x else i0) + (sm * ((2 * k * dm + dM) // (2 * dM)) if dM else 0)
                i, j = (major, minor) if major_is_x else (minor, major)
                if 0 <= i < size and 0 <= j < size:
                    hits[j, i] += 1
    return top, hits


def python_compose(top, hits, rgb, edge_shade):
    size = top.shape[0]
    rgba = np.full((size, size, 4), 255, dtype=np.uint8)
    grey = (255 - np.minimum(255, edge_shade * hits.astype(np.int64))).astype(np.uint8)
    edge = hits > 0
    for channel in range(3):
        rgba[..., channel][edge] = grey[edge]
    vertex = top > 0
    color = np.asarray(rgb, dtype=np.uint32)[top[vertex] - 1]
    rgba[..., 0][vertex] = (color >> 16) & 255
    rgba[..., 1][vertex] = (color >> 8) & 255
    rgba[..., 2][vertex] = color & 255
    return rgba


def python_colors(values, min_color_value=None, max_color_value=None):
    """(rgb, [minValue, maxValue, minColorValue, maxColorValue]) in float64 numpy scalars, a value at a time."""
    values = np.asarray(values, dtype=np.float64)
    low, high = np.float64(NO_VALUE), np.float64(-NO_VALUE)
    for value in values:
        if value == NO_VALUE:
            continue
        if value < low:
            low = value
        if high < value:
            high = value
    low_color = low if min_color_value is None else np.float64(min_color_value)
    high_color = high if max_color_value is None else np.float64(max_color_value)
    if low == high or high == -NO_VALUE:
        return np.full(len(values), COLOR_BLACK, dtype=np.uint32), [low, high, low_color, high_color]
    rgb = np.zeros(len(values), dtype=np.uint32)
    with np.errstate(all="ignore"):
        scale = np.float64(1.) / (high_color - low_color)
        for at, value in enumerate(values):
            if value == NO_VALUE:
                rgb[at] = COLOR_NONE
                continue
            t = scale * (value - low_color)
            if t <= 0.:
                red, green = np.float64(1.), np.float64(0.)
            elif t <= 0.5:
                red, green = np.float64(1.), np.float64(2.) * t
            elif t < 1.:
                red, green = np.float64(2.) * (np.float64(1.) - t), np.float64(1.)
            else:
                red, green = np.float64(0.), np.float64(1.)
            red, green = max(np.float64(0.), min(red, np.float64(1.))), max(np.float64(0.), min(green, np.float64(1.)))
            rgb[at] = (int(red * np.float64(255.)) << 16) | (int(green * np.float64(255.)) << 8)
    return rgb, [low, high, low_color, high_color]


def color_strings(rgb):
    return ["" if v & COLOR_NONE else ("black" if v & COLOR_BLACK else "#%06x" % (v & 0xffffff)) for v in np.asarray(rgb).tolist()]


def python_svg(x, y, cell_ids, v0, v1, hide_edges, size, xc, yc, half, radius, thickness, gene_set_name, colors=None, groups=None,
               group_colors=None):
    """CellGraph::writeSvg with '%g' for ostream's default formatting of a double."""
    n = lambda value: "%g" % value
    x, y = np.asarray(x, dtype=np.float64).tolist(), np.asarray(y, dtype=np.float64).tolist()
    cell_ids = np.asarray(cell_ids).tolist()
    out = ["<p><svg id=graphSvg width='%s' height='%s' viewBox='%s %s %s %s'>" % (n(size), n(size), n(xc - half), n(yc - half),
                                                                                   n(2. * half), n(2. * half))]
    if not hide_edges:
        out.append("<g id=edges>")
        for a, b in zip(np.asarray(v0).tolist(), np.asarray(v1).tolist()):
            out.append("<line x1='%s' y1='%s' x2='%s' y2='%s' style='stroke:black;stroke-width:%s' />"
                       % (n(x[a]), n(y[a]), n(x[b]), n(y[b]), n(thickness)))
        out.append("</g>")

    def circle(v, fill):
        return ("<a xlink:href='cell?cellId=%d&geneSetName=%s'><circle cx='%s' cy='%s' r='%s' stroke=none%s><title>Cell %d</title>"
                "</circle></a>" % (cell_ids[v], gene_set_name, n(x[v]), n(y[v]), n(radius), " fill='%s'" % fill if fill else "",
                                   cell_ids[v]))

    if not group_colors:
        out.append("<g id=vertices><g>")
        out.extend(circle(v, colors[v] if colors is not None else "") for v in range(len(x)))
        out.append("</g></g>")
    else:
        groups = np.asarray(groups).tolist()
        out.append("<g id=vertices>")
        for group in range(max(groups) + 1 if groups else 0):
            out.append("<g id=vertexGroup%d style='fill:%s'>" % (group, group_colors.get(group, "black")))
            out.extend(circle(v, "") for v in range(len(x)) if groups[v] == group)
            out.append("</g>")
        out.append("</g>")
    return "".join(out).encode("utf-8")


def python_category(values):
    """(groups, groupColors, frequencyTable, couldNotColor) of the page's "category" colouring."""
    frequency = {}
    for value in values:
        frequency[value] = frequency.get(value, 0) + 1
    table = sorted(((count, value.encode("utf-8")) for value, count in frequency.items()), key=lambda p: (-p[0], p[1]))
    # count descending, then value DESCENDING: reverse the ties
    ordered = []
    at = 0
    while at < len(table):
        end = at
        while end < len(table) and table[end][0] == table[at][0]:
            end += 1
        ordered.extend(reversed(table[at:end]))
        at = end
    table = [(count, value.decode("utf-8")) for count, value in ordered]
    group_of = {value: group for group, (_, value) in enumerate(table)}
    group_colors = {group: (PALETTE[group] if group < 12 else "black") for group in range(len(table))}
    return [group_of[v] for v in values], group_colors, table, sum(count for count, _ in table[12:])


def python_coordinate_range(x, y):
    """CellGraph::computeCoordinateRange as written: the maxima start at the smallest positive normal double."""
    x_min = y_min = float(np.finfo(np.float64).max)
    x_max = y_max = float(np.finfo(np.float64).tiny)
    for px, py in zip(np.asarray(x).tolist(), np.asarray(y).tolist()):
        x_min, x_max, y_min, y_max = min(x_min, px), max(x_max, px), min(y_min, py), max(y_max, py)
    return x_min, x_max, y_min, y_max


def python_default_view(x, y, size):
    x_min, x_max, y_min, y_max = python_coordinate_range(x, y)
    delta_x, delta_y = x_max - x_min, y_max - y_min
    if delta_x <= delta_y:
        delta = delta_y
        x_max = x_min + delta
    else:
        delta = delta_x
        y_max = y_min + delta
    delta *= 1.05
    return (x_min + x_max) / 2., (y_min + y_max) / 2., delta / 2., 1.5 * delta / size, 0.05 * delta / size


def read_png(path):
    """uint8 [height, width, 4] of an 8-bit RGBA PNG whose rows all have filter 0; checks the chunks' CRCs."""
    with open(path, "rb") as f:
        raw = f.read()
    assert raw[:8] == b"\x89PNG\r\n\x1a\n"
    at, chunks = 8, []
    while at < len(raw):
        length, = struct.unpack(">I", raw[at:at + 4])
        kind, payload = raw[at + 4:at + 8], raw[at + 8:at + 8 + length]
        assert struct.unpack(">I", raw[at + 8 + length:at + 12 + length])[0] == zlib.crc32(kind + payload) & 0xffffffff
        chunks.append((kind, payload))
        at += 12 + length
    assert [kind for kind, _ in chunks] == [b"IHDR", b"IDAT", b"IEND"]
    width, height, depth, color_type, compression, filtering, interlace = struct.unpack(">IIBBBBB", chunks[0][1])
    assert (depth, color_type, compression, filtering, interlace) == (8, 6, 0, 0, 0)
    rows = np.frombuffer(zlib.decompress(chunks[1][1]), dtype=np.uint8).reshape(height, 1 + 4 * width)
    assert not rows[:, 0].any()
    return rows[:, 1:].reshape(height, width, 4).copy()
