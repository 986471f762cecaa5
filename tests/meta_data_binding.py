"""ctypes binding of tests/native/em2_meta_data_restatement.cpp (the reference's cell meta data semantics with std::list,
std::map and std::vector<std::string>, its histogram, dense contingency table and computeRandIndex in their own order and
types) and the inputs the meta data tests share.  Compiled with g++ at first use.  Test infrastructure only."""
import ctypes
import functools
import os
import struct
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE_DIR = os.path.join(ROOT, "tests", "native")
SOURCE = os.path.join(NATIVE_DIR, "em2_meta_data_restatement.cpp")
CONTINGENCY_KEYS = ("rowTotals", "columnTotals", "i0", "i1", "count")

c = ctypes
P = c.c_void_p


def _ptr(a):
    return a.ctypes.data_as(c.c_void_p)


def _b(s):
    return s.encode("utf-8")


def _strings(raw):
    return [v.decode("utf-8") for v in raw.split(b"\0")[:-1]]


def double_bits(x):
    """A double as its 64 bits: NaN compares equal to the same NaN, -0.0 differs from 0.0."""
    return struct.unpack("<Q", struct.pack("<d", x))[0]


class Store:
    """The restated store of one data directory."""

    def __init__(self, lib, cell_count):
        self.lib = lib
        self.cell_count = cell_count
        self.handle = lib.em2r_md_create(cell_count)

    def __del__(self):
        self.lib.em2r_md_free(self.handle)

    def set(self, cell, name, value):
        self.lib.em2r_md_set(self.handle, cell, _b(name), _b(value))

    def remove(self, cell_set, name):
        cells = np.ascontiguousarray(cell_set, dtype=np.uint32)
        self.lib.em2r_md_remove(self.handle, _ptr(cells), len(cells), _b(name))

    def usage(self, name):
        return int(self.lib.em2r_md_usage(self.handle, _b(name)))

    def value(self, cell, name):
        size = self.lib.em2r_md_value(self.handle, cell, _b(name), None)
        out = c.create_string_buffer(max(size, 1))
        self.lib.em2r_md_value(self.handle, cell, _b(name), out)
        return out.raw[:size].decode("utf-8")

    def pairs(self, cell):
        size = self.lib.em2r_md_pairs(self.handle, cell, None)
        out = c.create_string_buffer(max(size, 1))
        self.lib.em2r_md_pairs(self.handle, cell, out)
        parts = _strings(out.raw[:size])
        return list(zip(parts[0::2], parts[1::2]))

    def select(self, field, match, use_regex):
        """The cells createCellSetUsingMetaData selects, ascending; None where the regular expression is invalid."""
        out = np.zeros(max(self.cell_count, 1), dtype=np.uint32)
        count = self.lib.em2r_md_select(self.handle, _b(field), _b(match), 1 if use_regex else 0, _ptr(out))
        return None if count < 0 else out[:count].tolist()

    def table(self, cell_set, name0, name1=None):
        """-> {"histogram0": [(value, count)], "histogram1", "dense" uint64 [n0, n1], "randIndex", "adjustedRandIndex"}; with
        one name only histogram0."""
        cells = np.ascontiguousarray(cell_set, dtype=np.uint32)
        handle = self.lib.em2r_md_table(self.handle, _ptr(cells), len(cells), _b(name0), None if name1 is None else _b(name1))
        try:
            sizes = [c.c_uint64(0) for _ in range(4)]
            self.lib.em2r_md_table_sizes(handle, *[c.byref(s) for s in sizes])
            n0, n1, bytes0, bytes1 = (int(s.value) for s in sizes)
            values = [c.create_string_buffer(max(bytes0, 1)), c.create_string_buffer(max(bytes1, 1))]
            counts = [np.zeros(n0, dtype=np.uint64), np.zeros(n1, dtype=np.uint64)]
            dense = np.zeros((n0, n1), dtype=np.uint64)
            indices = np.zeros(2, dtype=np.float64)
            self.lib.em2r_md_table_get(handle, values[0], _ptr(counts[0]), values[1], _ptr(counts[1]),
                                       _ptr(dense) if name1 is not None else None, _ptr(indices))
        finally:
            self.lib.em2r_md_table_free(handle)
        out = {"histogram0": list(zip(_strings(values[0].raw[:bytes0]), counts[0].tolist()))}
        if name1 is not None:
            out.update(histogram1=list(zip(_strings(values[1].raw[:bytes1]), counts[1].tolist())), dense=dense,
                       randIndex=float(indices[0]), adjustedRandIndex=float(indices[1]))
        return out


class MetaDataRestatement:
    def __init__(self, lib):
        self.lib = lib
        lib.em2r_md_create.argtypes, lib.em2r_md_create.restype = [c.c_uint32], P
        lib.em2r_md_free.argtypes, lib.em2r_md_free.restype = [P], None
        lib.em2r_md_set.argtypes, lib.em2r_md_set.restype = [P, c.c_uint32, c.c_char_p, c.c_char_p], None
        lib.em2r_md_remove.argtypes, lib.em2r_md_remove.restype = [P, P, c.c_uint64, c.c_char_p], None
        lib.em2r_md_usage.argtypes, lib.em2r_md_usage.restype = [P, c.c_char_p], c.c_int64
        lib.em2r_md_value.argtypes, lib.em2r_md_value.restype = [P, c.c_uint32, c.c_char_p, P], c.c_uint64
        lib.em2r_md_pairs.argtypes, lib.em2r_md_pairs.restype = [P, c.c_uint32, P], c.c_uint64
        lib.em2r_md_select.argtypes, lib.em2r_md_select.restype = [P, c.c_char_p, c.c_char_p, c.c_int, P], c.c_int64
        lib.em2r_md_table.argtypes, lib.em2r_md_table.restype = [P, P, c.c_uint64, c.c_char_p, c.c_char_p], P
        lib.em2r_md_table_sizes.argtypes, lib.em2r_md_table_sizes.restype = [P] * 5, None
        lib.em2r_md_table_get.argtypes, lib.em2r_md_table_get.restype = [P] * 7, None
        lib.em2r_md_table_free.argtypes, lib.em2r_md_table_free.restype = [P], None
        lib.em2r_rand_index.argtypes, lib.em2r_rand_index.restype = [P, c.c_uint64, c.c_uint64, P], None
        lib.em2r_contingency.argtypes, lib.em2r_contingency.restype = [P, P, c.c_uint64, c.c_uint32, c.c_uint32], P
        lib.em2r_contingency_size.argtypes, lib.em2r_contingency_size.restype = [P], c.c_uint64
        lib.em2r_contingency_get.argtypes, lib.em2r_contingency_get.restype = [P] * 7, None
        lib.em2r_contingency_free.argtypes, lib.em2r_contingency_free.restype = [P], None

    def store(self, cell_count):
        return Store(self.lib, cell_count)

    def rand_index(self, table):
        """computeRandIndex on a dense table (a 2-d array of counts) -> (randIndex, adjustedRandIndex)."""
        table = np.ascontiguousarray(table, dtype=np.uint64)
        indices = np.zeros(2, dtype=np.float64)
        self.lib.em2r_rand_index(_ptr(table), table.shape[0], table.shape[1], _ptr(indices))
        return float(indices[0]), float(indices[1])

    def contingency(self, id0, id1, n0, n1):
        """-> the dict of capi.contingency_take without n and path."""
        id0 = np.ascontiguousarray(id0, dtype=np.uint32)
        id1 = np.ascontiguousarray(id1, dtype=np.uint32)
        handle = self.lib.em2r_contingency(_ptr(id0), _ptr(id1), len(id0), n0, n1)
        try:
            size = int(self.lib.em2r_contingency_size(handle))
            out = {"rowTotals": np.zeros(n0, dtype=np.uint64), "columnTotals": np.zeros(n1, dtype=np.uint64),
                   "i0": np.zeros(size, dtype=np.uint32), "i1": np.zeros(size, dtype=np.uint32), "count": np.zeros(size, dtype=np.uint64)}
            sums = np.zeros(3, dtype=np.uint64)
            self.lib.em2r_contingency_get(handle, *[_ptr(out[key]) for key in CONTINGENCY_KEYS], _ptr(sums))
        finally:
            self.lib.em2r_contingency_free(handle)
        out["sumCells"], out["sumRows"], out["sumColumns"] = (int(x) for x in sums)
        return out


@functools.lru_cache(maxsize=None)
def load():
    build = os.path.join(NATIVE_DIR, "build")
    os.makedirs(build, exist_ok=True)
    path = os.path.join(build, "libem2metadatarestatement.so")
    if not os.path.exists(path) or os.path.getmtime(path) < os.path.getmtime(SOURCE):
        tmp = path + ".%d.tmp" % os.getpid()
        # -ffp-contract=off: computeRandIndex must round every product and sum, as the reference built for SSE4.2 does
        cmd = ["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-o", tmp, SOURCE]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError("meta data restatement build failed: " + r.stderr)
        os.replace(tmp, path)
    return MetaDataRestatement(ctypes.CDLL(path))


def sums_of(table):
    """(sum v (v - 1) over the cells, sum t (t - 1) over the row totals, over the column totals, n) of a dense table, as
    Python ints."""
    rows = [[int(v) for v in row] for row in np.asarray(table, dtype=np.uint64).tolist()]
    row_totals = [sum(row) for row in rows]
    column_totals = [sum(column) for column in zip(*rows)]
    pairs = lambda values: sum(v * (v - 1) for v in values)
    return pairs(v for row in rows for v in row), pairs(row_totals), pairs(column_totals), sum(row_totals)


def numpy_contingency(id0, id1, n0, n1):
    """The same table from np.unique and np.bincount, with Python-int sums."""
    id0 = np.asarray(id0, dtype=np.uint64)
    id1 = np.asarray(id1, dtype=np.uint64)
    keys, counts = np.unique(id0 * np.uint64(n1) + id1, return_counts=True)
    out = {"rowTotals": np.bincount(id0.astype(np.int64), minlength=n0).astype(np.uint64),
           "columnTotals": np.bincount(id1.astype(np.int64), minlength=n1).astype(np.uint64),
           "i0": (keys // np.uint64(n1)).astype(np.uint32), "i1": (keys % np.uint64(n1)).astype(np.uint32),
           "count": counts.astype(np.uint64)}
    pairs = lambda values: sum(int(v) * (int(v) - 1) for v in values.tolist())
    out["sumCells"], out["sumRows"], out["sumColumns"] = pairs(out["count"]), pairs(out["rowTotals"]), pairs(out["columnTotals"])
    return out


def assert_same_contingency(mine, theirs, what):
    for key in CONTINGENCY_KEYS:
        a, b = mine[key], theirs[key]
        assert a.dtype == b.dtype and a.shape == b.shape, "%s: %s has another size or type" % (what, key)
        assert np.array_equal(a, b), "%s: %s differs" % (what, key)
    for key in ("sumCells", "sumRows", "sumColumns"):
        assert mine[key] == theirs[key], "%s: %s %d != %d" % (what, key, mine[key], theirs[key])
