"""ctypes binding of tests/native/em2_signature_draw_restatement.cpp (the colour census, the value table, the random colours,
the pie raster, its boundary vectors and the SVG text of a signature graph, one thread and plain loops), an independent numpy /
Python statement of the same definitions, and what the signature drawing tests share.  Compiled with g++ at first use.  Test
infrastructure only."""
import ctypes
import functools
import math
import os
import subprocess

import numpy as np

import draw_binding as db

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE_DIR = os.path.join(ROOT, "tests", "native")
SOURCE = os.path.join(NATIVE_DIR, "em2_signature_draw_restatement.cpp")
PALETTE = db.PALETTE + ("black",)              # the colour string of a colour index 0 .. 12
PALETTE_RGB = np.asarray([int(s[1:], 16) for s in db.PALETTE] + [db.COLOR_BLACK], dtype=np.uint32)

c = ctypes
P = c.c_void_p


def _ptr(a):
    return a.ctypes.data_as(c.c_void_p) if a is not None else None


def _packed(strings):
    return b"".join(s.encode("utf-8") + b"\0" for s in strings)


class SignatureDrawRestatement:
    def __init__(self, lib):
        self.lib = lib
        lib.em2r_census.argtypes = [c.c_uint32, P, P, c.c_uint64, P, c.c_uint32, P, c.c_uint32, P, P, P, P]
        lib.em2r_census.restype = c.c_int
        lib.em2r_value_table.argtypes = [c.c_char_p, c.c_uint64, P, P, P]
        lib.em2r_value_table.restype = c.c_uint64
        lib.em2r_order_by_count.argtypes = [P, c.c_uint64, P]
        lib.em2r_order_by_count.restype = None
        lib.em2r_random_colors.argtypes = [c.c_uint32, P, P]
        lib.em2r_random_colors.restype = None
        lib.em2r_pie_boundaries.argtypes = [c.c_uint32, P, P, P, P, P]
        lib.em2r_pie_boundaries.restype = None
        lib.em2r_graph_draw_pies.argtypes = [c.c_uint32, P, P, P, c.c_uint64, P, P, c.c_int, c.c_uint32, c.c_double, c.c_double,
                                             c.c_double, P, c.c_uint64, P, P, P, P, P, P]
        lib.em2r_graph_draw_pies.restype = c.c_int
        lib.em2r_signature_graph_svg.argtypes = [c.c_char_p, c.c_uint32, P, P, P, c.c_uint64, P, P, c.c_int, c.c_double, c.c_double,
                                                 c.c_double, c.c_double, c.c_double, c.c_double, P, c.c_char_p, P, P]
        lib.em2r_signature_graph_svg.restype = c.c_int

    def census(self, cell_offsets, cells, id_of_cell, color_of_value):
        """The dict of capi.pie_census_take without its counters, or None for an id out of range."""
        cell_offsets = np.ascontiguousarray(cell_offsets, dtype=np.uint64)
        cells = np.ascontiguousarray(cells, dtype=np.uint32)
        id_of_cell = np.ascontiguousarray(id_of_cell, dtype=np.uint32)
        color_of_value = np.ascontiguousarray(color_of_value, dtype=np.uint8)
        vertices = len(cell_offsets) - 1
        offsets = np.zeros(vertices + 1, dtype=np.uint64)
        color = np.zeros(13 * vertices, dtype=np.uint8)
        count = np.zeros(13 * vertices, dtype=np.uint32)
        fraction = np.zeros(13 * vertices, dtype=np.float64)
        if self.lib.em2r_census(vertices, _ptr(cell_offsets), _ptr(cells), len(cells), _ptr(id_of_cell), len(id_of_cell),
                                _ptr(color_of_value), len(color_of_value), _ptr(offsets), _ptr(color), _ptr(count), _ptr(fraction)):
            return None
        n = int(offsets[-1])
        return {"sliceOffsets": offsets, "sliceColor": color[:n].copy(), "sliceCells": count[:n].copy(), "sliceFraction": fraction[:n].copy()}

    def value_table(self, values):
        """([(value, cells)] in the reference's sorted order, the rank of every cell's value)."""
        order = np.zeros(len(values), dtype=np.uint32)
        cells = np.zeros(len(values), dtype=np.uint64)
        rank = np.zeros(len(values), dtype=np.uint32)
        n = self.lib.em2r_value_table(_packed(values) + b"\0", len(values), _ptr(order), _ptr(cells), _ptr(rank))
        in_map_order = sorted(set(values), key=lambda s: s.encode("utf-8"))
        return [(in_map_order[order[r]], int(cells[r])) for r in range(n)], rank

    def order_by_count(self, counts):
        counts = np.ascontiguousarray(counts, dtype=np.uint64)
        order = np.zeros(len(counts), dtype=np.uint32)
        self.lib.em2r_order_by_count(_ptr(counts), len(counts), _ptr(order))
        return order

    def random_colors(self, vertex_count):
        rgb = np.zeros(vertex_count, dtype=np.uint32)
        draws = np.zeros(3 * vertex_count, dtype=np.float64)
        self.lib.em2r_random_colors(vertex_count, _ptr(rgb), _ptr(draws))
        return rgb, draws

    def pie_boundaries(self, slice_offsets, slice_fraction):
        slice_offsets = np.ascontiguousarray(slice_offsets, dtype=np.uint64)
        slice_fraction = np.ascontiguousarray(slice_fraction, dtype=np.float64)
        bx, by = np.zeros(len(slice_fraction), dtype=np.int32), np.zeros(len(slice_fraction), dtype=np.int32)
        arc = np.zeros(len(slice_fraction), dtype=np.uint8)
        self.lib.em2r_pie_boundaries(len(slice_offsets) - 1, _ptr(slice_offsets), _ptr(slice_fraction), _ptr(bx), _ptr(by), _ptr(arc))
        return bx, by, arc

    def graph_draw_pies(self, x, y, radius, v0, v1, size, xc, yc, half, slice_offsets, bx, by, arc, hide_edges=False):
        """(vertexTop, sliceTop, edgeHits) or None for an argument error."""
        x = np.ascontiguousarray(x, dtype=np.float64)
        y = np.ascontiguousarray(y, dtype=np.float64)
        radius = np.ascontiguousarray(radius, dtype=np.float64)
        v0 = np.ascontiguousarray(v0, dtype=np.uint32)
        v1 = np.ascontiguousarray(v1, dtype=np.uint32)
        slice_offsets = np.ascontiguousarray(slice_offsets, dtype=np.uint64)
        bx, by = np.ascontiguousarray(bx, dtype=np.int32), np.ascontiguousarray(by, dtype=np.int32)
        arc = np.ascontiguousarray(arc, dtype=np.uint8)
        layers = [np.zeros((size, size), dtype=np.uint32) for _ in range(3)]
        if self.lib.em2r_graph_draw_pies(len(x), _ptr(x), _ptr(y), _ptr(radius), len(v0), _ptr(v0), _ptr(v1), int(hide_edges), size, xc, yc,
                                         half, _ptr(slice_offsets), len(bx), _ptr(bx), _ptr(by), _ptr(arc), *[_ptr(a) for a in layers]):
            return None
        return tuple(layers)

    def svg(self, path, x, y, cell_counts, v0, v1, hide_edges=False, size=500., x_shift=0., y_shift=0., zoom=1., vertex_size=1.,
            edge_thickness=1., slice_offsets=None, slice_colors=None, slice_fraction=None):
        """(the file's bytes, the four svgParameters)."""
        x = np.ascontiguousarray(x, dtype=np.float64)
        y = np.ascontiguousarray(y, dtype=np.float64)
        cell_counts = np.ascontiguousarray(cell_counts, dtype=np.uint64)
        v0 = np.ascontiguousarray(v0, dtype=np.uint32)
        v1 = np.ascontiguousarray(v1, dtype=np.uint32)
        offsets = None if slice_offsets is None else np.ascontiguousarray(slice_offsets, dtype=np.uint64)
        fraction = None if slice_offsets is None else np.ascontiguousarray(slice_fraction, dtype=np.float64)
        parameters = np.zeros(4, dtype=np.float64)
        rc = self.lib.em2r_signature_graph_svg(os.fsencode(path), len(x), _ptr(x), _ptr(y), _ptr(cell_counts), len(v0), _ptr(v0), _ptr(v1),
                                               int(hide_edges), size, x_shift, y_shift, zoom, vertex_size, edge_thickness, _ptr(offsets),
                                               None if slice_offsets is None else _packed(slice_colors) + b"\0", _ptr(fraction),
                                               _ptr(parameters))
        assert rc == 0
        with open(path, "rb") as f:
            return f.read(), tuple(parameters.tolist())


@functools.lru_cache(maxsize=None)
def load():
    build = os.path.join(NATIVE_DIR, "build")
    os.makedirs(build, exist_ok=True)
    path = os.path.join(build, "libem2signaturedrawrestatement.so")
    if not os.path.exists(path) or os.path.getmtime(path) < os.path.getmtime(SOURCE):
        tmp = path + ".%d.tmp" % os.getpid()
        cmd = ["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-o", tmp, SOURCE]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError("signature draw restatement build failed: " + r.stderr)
        os.replace(tmp, path)
    return SignatureDrawRestatement(ctypes.CDLL(path))


# ---- the independent statement: dicts, Python integers, float64 numpy, '%g' ----

def python_census(cell_offsets, cells, id_of_cell, color_of_value):
    """The dict of the census from a dict per vertex (insertion order is first occurrence) and a stable sort."""
    offsets, colors, counts, fractions = [0], [], [], []
    cells, ids, color_of_value = np.asarray(cells).tolist(), np.asarray(id_of_cell).tolist(), np.asarray(color_of_value).tolist()
    bounds = np.asarray(cell_offsets).tolist()
    for begin, end in zip(bounds[:-1], bounds[1:]):
        tally = {}
        for cell in cells[begin:end]:
            color = color_of_value[ids[cell]]
            tally[color] = tally.get(color, 0) + 1
        ranked = sorted(tally.items(), key=lambda p: -p[1])                # sorted() is stable
        if ranked:
            factor = np.float64(1.) / np.float64(sum(n for _, n in ranked))
            for color, n in ranked:
                colors.append(color)
                counts.append(n)
                fractions.append(np.float64(n) * factor)
        offsets.append(len(colors))
    return {"sliceOffsets": np.asarray(offsets, dtype=np.uint64), "sliceColor": np.asarray(colors, dtype=np.uint8),
            "sliceCells": np.asarray(counts, dtype=np.uint32), "sliceFraction": np.asarray(fractions, dtype=np.float64)}


def python_value_table(values):
    """[(value, cells)] for at most 16 distinct values, where std::sort is an insertion sort and keeps the map's order among
    equal counts; and the rank of every cell's value."""
    tally = {}
    for value in values:
        tally[value] = tally.get(value, 0) + 1
    assert len(tally) <= 16
    table = sorted(sorted(tally.items(), key=lambda p: p[0].encode("utf-8")), key=lambda p: -p[1])
    rank_of = {value: rank for rank, (value, _) in enumerate(table)}
    return table, np.asarray([rank_of[v] for v in values], dtype=np.uint32)


def python_mt19937(seed, count):
    """The first `count` 32-bit outputs of std::mt19937(seed)."""
    state = [seed & 0xffffffff]
    for i in range(1, 624):
        state.append((1812433253 * (state[-1] ^ (state[-1] >> 30)) + i) & 0xffffffff)
    out, at = [], 624
    while len(out) < count:
        if at == 624:
            for i in range(624):
                y = (state[i] & 0x80000000) | (state[(i + 1) % 624] & 0x7fffffff)
                state[i] = state[(i + 397) % 624] ^ (y >> 1) ^ (0x9908b0df if y & 1 else 0)
            at = 0
        y = state[at]
        at += 1
        y ^= y >> 11
        y ^= (y << 7) & 0x9d2c5680
        y ^= (y << 15) & 0xefc60000
        y ^= y >> 18
        out.append(y)
    return out


def python_random_colors(vertex_count):
    """(rgb, draws): a draw of uniform_real_distribution<double>(0, 1.) is (lo + hi * 2^32) / 2^64 of two consecutive outputs,
    in doubles."""
    words = python_mt19937(231, 6 * vertex_count)
    draws = [(float(words[2 * i]) + float(words[2 * i + 1]) * 4294967296.) / 18446744073709551616. for i in range(3 * vertex_count)]
    rgb = [(int(max(0., min(r, 1.)) * 255) << 16) | (int(max(0., min(g, 1.)) * 255) << 8) | int(max(0., min(b, 1.)) * 255)
           for r, g, b in zip(draws[0::3], draws[1::3], draws[2::3])]
    return np.asarray(rgb, dtype=np.uint32), np.asarray(draws, dtype=np.float64)


def python_pie_boundaries(slice_offsets, slice_fraction):
    offsets = np.asarray(slice_offsets).tolist()
    fraction = np.asarray(slice_fraction, dtype=np.float64)
    bx, by, arc = [], [], []
    round_away = lambda value: int(np.copysign(np.floor(np.abs(value) + 0.5), value))
    for begin, end in zip(offsets[:-1], offsets[1:]):
        total = np.float64(0.)
        for k in range(begin, end):
            angle = fraction[k] * np.float64(2.) * np.float64(np.pi)
            bx.append(round_away(np.cos(total) * np.float64(1048576.)))
            by.append(round_away(np.sin(total) * np.float64(1048576.)))
            arc.append(int(angle > np.pi))
            total = total + angle
    return np.asarray(bx, dtype=np.int32), np.asarray(by, dtype=np.int32), np.asarray(arc, dtype=np.uint8)


def python_pie_raster(x, y, radius, v0, v1, size, xc, yc, half, slice_offsets, bx, by, arc, hide_edges=False):
    """(vertexTop, sliceTop, edgeHits): a set of covered pixels per vertex, Python integers for the cross products; the edge layer
    is draw_binding.python_raster's."""
    ux, uy = db.python_subpixels(x, y, size, xc, yc, half)
    s256 = db.python_view(size, xc, yc, half, 0.)[2]
    offsets = np.asarray(slice_offsets).tolist()
    bx, by, arc = np.asarray(bx).tolist(), np.asarray(by).tolist(), np.asarray(arc).tolist()
    top = np.zeros((size, size), dtype=np.uint32)
    for v, (cx, cy) in enumerate(zip(ux, uy)):
        R = int(math.floor(float(radius[v]) * s256 + 0.5))
        covered = {(cx >> 8, cy >> 8)}
        for j in range(max(0, (cy - R) // 256 - 1), min(size, (cy + R) // 256 + 2)):
            for i in range(max(0, (cx - R) // 256 - 1), min(size, (cx + R) // 256 + 2)):
                if (256 * i + 128 - cx) ** 2 + (256 * j + 128 - cy) ** 2 <= R * R:
                    covered.add((i, j))
        for i, j in covered:
            if 0 <= i < size and 0 <= j < size:
                top[j, i] = max(int(top[j, i]), v + 1)
    cross = lambda p, q: p[0] * q[1] - p[1] * q[0]
    slices = np.zeros((size, size), dtype=np.uint32)
    for j, i in np.argwhere(top > 0).tolist():
        v = int(top[j, i]) - 1
        first, m = offsets[v], offsets[v + 1] - offsets[v]
        d = (256 * i + 128 - ux[v], 256 * j + 128 - uy[v])
        chosen = 0
        if m >= 2 and d != (0, 0):
            chosen = m - 1
            for k in range(m - 1):
                a, b = (bx[first + k], by[first + k]), (bx[first + k + 1], by[first + k + 1])
                small = cross(a, d) >= 0 and cross(d, b) > 0
                other = cross(b, d) >= 0 and cross(d, a) > 0
                if (not other) if arc[first + k] else small:
                    chosen = k
                    break
        slices[j, i] = first + chosen + 1
    hits = db.python_raster(x, y, v0, v1, size, xc, yc, half, 0., hide_edges)[1]
    return top, slices, hits


def python_signature_view(x, y, cell_counts, size, x_shift=0., y_shift=0., zoom=1.):
    """(xCenter, yCenter, halfViewBoxSize, pixelSize, boundingBoxSize) of SignatureGraph::writeSvg as written: the maxima start at
    the smallest positive normal double."""
    x_min = y_min = float(np.finfo(np.float64).max)
    x_max = y_max = float(np.finfo(np.float64).tiny)
    for px, py in zip(np.asarray(x).tolist(), np.asarray(y).tolist()):
        x_min, x_max, y_min, y_max = min(x_min, px), max(x_max, px), min(y_min, py), max(y_max, py)
    box = max(x_max - x_min, y_max - y_min)
    view = 1.05 * box / zoom
    return (x_min + x_max) / 2. - x_shift, (y_min + y_max) / 2. - y_shift, view / 2., view / size, box


def python_signature_svg(x, y, cell_counts, v0, v1, hide_edges=False, size=500., x_shift=0., y_shift=0., zoom=1., vertex_size=1.,
                         edge_thickness=1., slice_offsets=None, slice_colors=None, slice_fraction=None):
    """SignatureGraph::writeSvg with '%g' for ostream's default formatting of a double; for at most 16 vertices, where the sort
    of the vertices is stable."""
    n = lambda value: "%g" % value
    x, y = np.asarray(x, dtype=np.float64).tolist(), np.asarray(y, dtype=np.float64).tolist()
    counts = np.asarray(cell_counts).tolist()
    assert len(x) <= 16
    xc, yc, half, _, box = python_signature_view(x, y, counts, size, x_shift, y_shift, zoom)
    out = ["<svg id=svgObject style='border:solid DarkBlue;margin:2;' width='%s' height='%s' viewBox='%s %s %s %s'>"
           % (n(size), n(size), n(xc - half), n(yc - half), n(2. * half), n(2. * half))]
    if not hide_edges:
        out.append("<g id=edges>")
        for a, b in zip(np.asarray(v0).tolist(), np.asarray(v1).tolist()):
            out.append("<line x1='%s' y1='%s' x2='%s' y2='%s' style='stroke:black;stroke-width:%s' />"
                       % (n(x[a]), n(y[a]), n(x[b]), n(y[b]), n(5.e-4 * box * edge_thickness)))
        out.append("</g>")
    out.append("<g id=vertices>")
    offsets = None if slice_offsets is None else np.asarray(slice_offsets).tolist()
    fraction = None if slice_offsets is None else np.asarray(slice_fraction, dtype=np.float64).tolist()
    largest = max(counts) if counts else 0
    for v in sorted(range(len(x)), key=lambda v: -counts[v]):
        radius = 0.03 * box * math.sqrt(float(counts[v]) / float(largest))
        transform = " transform='translate(%s %s) scale(%s)'" % (n(x[v]), n(y[v]), n(vertex_size))
        first, m = (offsets[v], offsets[v + 1] - offsets[v]) if offsets is not None else (0, 0)
        if m < 2:
            out.append("<circle cx='0' cy='0' r='%s' stroke='none' fill='%s'%s></circle>"
                       % (n(radius), slice_colors[first] if m else "black", transform))
            continue
        total = 0.
        for k in range(first, first + m):
            angle = fraction[k] * 2. * math.pi
            end = total + angle
            out.append("<path d='M 0 0 L %s %s A %s %s 0 %d 1 %s %s Z' stroke='none' fill='%s'%s></path>"
                       % (n(radius * math.cos(total)), n(radius * math.sin(total)), n(radius), n(radius), int(angle > math.pi),
                          n(radius * math.cos(end)), n(radius * math.sin(end)), slice_colors[k], transform))
            total = end
    out.append("</g></svg>")
    return "".join(out).encode("utf-8")


def slice_rgb(slice_color):
    """The packed colour of every slice of a census."""
    return PALETTE_RGB[np.asarray(slice_color, dtype=np.int64)]


def slice_strings(slice_color):
    return [PALETTE[k] for k in np.asarray(slice_color).tolist()]
