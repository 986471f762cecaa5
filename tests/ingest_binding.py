"""ctypes binding of tests/native/em2_ingest_restatement.cpp (addCell's storing part and the per-barcode loop of
addCellsFromHdf5 with the reference's types) and what the ingest tests share: the sparse inputs, the two device passes with
guarded output buffers, and the header rules of the reference's files.  Compiled with g++ at first use.  Test infrastructure
only."""
import ctypes
import functools
import os
import struct
import subprocess

import numpy as np

from expressionmatrix2_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE_DIR = os.path.join(ROOT, "tests", "native")
SOURCE = os.path.join(NATIVE_DIR, "em2_ingest_restatement.cpp")
FILL = 0x5a
GUARD = 64
NO_GENE = 0xffffffff
OK, NEGATIVE, DUPLICATE, BAD_INDEX = 0, 1, 2, 3

c = ctypes
P = c.c_void_p


def _ptr(a):
    return a.ctypes.data_as(c.c_void_p)


@functools.lru_cache(maxsize=None)
def load():
    build = os.path.join(NATIVE_DIR, "build")
    os.makedirs(build, exist_ok=True)
    path = os.path.join(build, "libem2ingestrestatement.so")
    if not os.path.exists(path) or os.path.getmtime(path) < os.path.getmtime(SOURCE):
        tmp = path + ".%d.tmp" % os.getpid()
        # the oracle's flags: the reference is built -O3 -msse4.2 and forms no FMA
        cmd = ["g++", "-std=c++11", "-O3", "-msse4.2", "-ffp-contract=off", "-fPIC", "-shared", "-o", tmp, SOURCE]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError("ingest restatement build failed: " + r.stderr)
        os.replace(tmp, path)
    lib = ctypes.CDLL(path)
    lib.em2r_ingest_csr.argtypes = [P, P, P, P, c.c_uint32, P, P, P, P, P, P, P]
    lib.em2r_ingest_csr.restype = None
    return lib


class Csr:
    """Rows of (index, value) lists as the arrays of the entries."""

    def __init__(self, rows, skip=None):
        lengths = [len(row) for row in rows]
        self.indptr = np.concatenate([[0], np.cumsum(lengths)]).astype(np.uint64)
        self.indices = np.ascontiguousarray([i for row in rows for i, _ in row], dtype=np.uint32)
        self.values = np.ascontiguousarray([v for row in rows for _, v in row], dtype=np.float32)
        self.cells = len(rows)
        self.skip = None if skip is None else np.ascontiguousarray(skip, dtype=np.uint8)

    @classmethod
    def from_arrays(cls, indptr, indices, values, skip=None):
        """The same from the arrays themselves (a million rows as lists of pairs would take minutes)."""
        self = cls.__new__(cls)
        self.indptr = np.ascontiguousarray(indptr, dtype=np.uint64)
        self.indices = np.ascontiguousarray(indices, dtype=np.uint32)
        self.values = np.ascontiguousarray(values, dtype=np.float32)
        self.cells = len(self.indptr) - 1
        assert self.indptr[0] == 0 and int(self.indptr[-1]) == len(self.indices) == len(self.values)
        assert (self.indptr[1:] >= self.indptr[:-1]).all()
        self.skip = None if skip is None else np.ascontiguousarray(skip, dtype=np.uint8)
        assert self.skip is None or len(self.skip) == self.cells
        return self


def restate(csr, gene_map):
    """-> dict(kept, status, duplicate, toc, data (bytes, 0x5a where nothing is stored), cells (bytes, likewise))."""
    gene_map = np.ascontiguousarray(gene_map, dtype=np.uint32)
    n = csr.cells
    kept, status, duplicate = np.zeros(n, np.uint32), np.zeros(n, np.uint32), np.zeros(n, np.uint32)
    toc = np.zeros(n + 1, np.uint64)
    data = np.full(8 * max(len(csr.values), 1), FILL, np.uint8)
    cells = np.full(56 * max(n, 1), FILL, np.uint8)
    load().em2r_ingest_csr(_ptr(csr.indptr), _ptr(csr.indices), _ptr(csr.values), _ptr(csr.skip) if csr.skip is not None else None, n,
                           _ptr(gene_map), _ptr(kept), _ptr(status), _ptr(duplicate), _ptr(toc), _ptr(data), _ptr(cells))
    return {"kept": kept, "status": status, "duplicate": duplicate, "toc": toc, "data": data[:8 * int(toc[n])].copy(),
            "cells": cells[:56 * n].copy()}


def _device(torch, array):
    array = np.ascontiguousarray(array)
    return torch.from_numpy(array.view(np.uint8).reshape(-1).copy()).cuda()


def device_count(torch, csr, gene_map, index_count=None):
    """em2_dev_ingest_count -> (dict(kept, status, duplicate, toc), the device arrays for the fill).  The map's buffer holds
    exactly the map, with a guard behind it; `index_count` is what the entry is told (default: the map's length)."""
    gene_map = np.ascontiguousarray(gene_map, dtype=np.uint32)
    index_count = len(gene_map) if index_count is None else index_count
    assert index_count <= len(gene_map)
    n = csr.cells
    genes = torch.full((4 * len(gene_map) + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    genes[:4 * len(gene_map)] = _device(torch, gene_map)
    d = {"indptr": _device(torch, csr.indptr), "indices": _device(torch, csr.indices), "values": _device(torch, csr.values),
         "skip": _device(torch, csr.skip) if csr.skip is not None else None, "genes": genes}
    out = {key: torch.full((4 * n + GUARD,), FILL, dtype=torch.uint8, device="cuda") for key in ("kept", "status", "duplicate")}
    out["toc"] = torch.full((8 * (n + 1) + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    capi.check(capi.load().em2_dev_ingest_count(
        d["indptr"].data_ptr(), d["indices"].data_ptr(), d["values"].data_ptr(), d["skip"].data_ptr() if d["skip"] is not None else None,
        n, d["genes"].data_ptr(), index_count, out["kept"].data_ptr(), out["status"].data_ptr(), out["duplicate"].data_ptr(),
        out["toc"].data_ptr(), None))
    torch.cuda.synchronize()
    assert (genes[4 * len(gene_map):].cpu().numpy() == FILL).all(), "the guard behind the gene map was written"
    result = {}
    for key, item, count in (("kept", 4, n), ("status", 4, n), ("duplicate", 4, n), ("toc", 8, n + 1)):
        host = out[key].cpu().numpy()
        assert (host[item * count:] == FILL).all(), "the guard behind %s was written" % key
        result[key] = host[:item * count].view(np.uint32 if item == 4 else np.uint64).copy()
    d["toc"] = out["toc"]
    d["map_length"] = index_count
    return result, d


def device_fill(torch, csr, d, entry_count, index_count=None, toc=None):
    """em2_dev_ingest_fill into buffers pre-filled with 0x5a with a guard behind each -> (data bytes, cells bytes).
    `index_count` defaults to what the count pass was told; `toc` (cells + 1 offsets) stands in for the count pass's own.
    The guards are looked at before the entry's answer is: a call that fails must have kept to its buffers too."""
    n = csr.cells
    data = torch.full((8 * entry_count + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    cells = torch.full((56 * n + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    d_toc = d["toc"]
    if toc is not None:
        toc = np.ascontiguousarray(toc, dtype=np.uint64)
        assert len(toc) == n + 1
        d_toc = _device(torch, toc)
    rc = capi.load().em2_dev_ingest_fill(
        d["indptr"].data_ptr(), d["indices"].data_ptr(), d["values"].data_ptr(), d["skip"].data_ptr() if d["skip"] is not None else None,
        n, d["genes"].data_ptr(), d["map_length"] if index_count is None else index_count, d_toc.data_ptr(), data.data_ptr(),
        cells.data_ptr(), None)
    torch.cuda.synchronize()
    data, cells = data.cpu().numpy(), cells.cpu().numpy()
    assert (data[8 * entry_count:] == FILL).all(), "the guard behind the entries was written"
    assert (cells[56 * n:] == FILL).all(), "the guard behind the Cell records was written"
    capi.check(rc)
    return data[:8 * entry_count].copy(), cells[:56 * n].copy()


def assert_same(torch, csr, gene_map, what=""):
    """Both device passes against the restatement, bit for bit: counts, statuses, reported genes, toc, and -- where no row
    fails -- the entries and the Cell records as bytes (untouched bytes must still be 0x5a).  -> the restatement's dict."""
    expected = restate(csr, gene_map)
    got, d = device_count(torch, csr, gene_map)
    for key in ("kept", "status", "duplicate", "toc"):
        assert np.array_equal(got[key], expected[key]), "%s: %s differs" % (what, key)
    if not expected["status"].any():
        data, cells = device_fill(torch, csr, d, int(expected["toc"][-1]))
        assert np.array_equal(data, expected["data"]), "%s: the entries differ" % what
        assert np.array_equal(cells, expected["cells"]), "%s: the Cell records differ" % what
    return expected


# ---- the reference's files by the header rules (src/MemoryMappedVector.hpp:141-197, :497-499) ----

VECTOR_MAGIC = 0xa3756fd4b5d8bcc1


def read_vector(path, dtype):
    """The objects of a MemoryMapped::Vector file, after the reference's open checks: header size, magic, the page-rounded
    file size the header states, capacity >= count, and the object size."""
    raw = open(path, "rb").read()
    header_size, object_size, count, pages, file_size, capacity, magic = struct.unpack("<7Q", raw[:56])
    dtype = np.dtype(dtype)
    assert header_size == 256 and magic == VECTOR_MAGIC, path
    assert file_size == len(raw) and file_size == pages * 4096, path
    assert object_size == dtype.itemsize and capacity >= count and 256 + capacity * object_size <= file_size, path
    assert raw[56:256] == bytes(200), path
    return np.frombuffer(raw, dtype=dtype, count=count, offset=256).copy()


NODE_DTYPE = np.dtype([("name", "<u4"), ("value", "<u4"), ("previous", "<u8"), ("next", "<u8")])
CELL_DTYPE = np.dtype([(name, "<f8") for name in ("sum1", "sum2", "norm2", "norm1Inverse", "norm2Inverse", "large1", "large2")])


def read_string_table(prefix):
    """-> (strings in id order, hash table)."""
    toc = read_vector(prefix + "-strings.toc", np.uint32)
    data = read_vector(prefix + "-strings.data", np.uint8).tobytes()
    table = read_vector(prefix + "-hashTable", np.uint32)
    assert len(table) & (len(table) - 1) == 0
    return [data[int(toc[i]):int(toc[i + 1])].decode("utf-8") for i in range(len(toc) - 1)], table


def read_lists(directory, prefix):
    """The (name, value) lists of CellMetaData / GeneMetaData, as strings."""
    base = os.path.join(directory, prefix + "MetaData")
    toc = read_vector(base + ".toc", np.uint64)
    nodes = read_vector(base + ".data", NODE_DTYPE)
    names, _ = read_string_table(base + "Names")
    values, _ = read_string_table(base + "Values")
    lists = []
    for end in toc.tolist():
        items, at = [], int(nodes["next"][end])
        while at != end:
            items.append((names[int(nodes["name"][at])], values[int(nodes["value"][at])]))
            at = int(nodes["next"][at])
        lists.append(items)
    return lists


def read_store(directory):
    """The content of a complete store: what a test compares between two stores, object counts and objects -- no capacity."""
    j = lambda name: os.path.join(directory, name)
    gene_names, _ = read_string_table(j("GeneNames"))
    cell_names, _ = read_string_table(j("CellNames"))
    return {
        "geneNames": gene_names, "cellNames": cell_names,
        "geneMetaData": read_lists(directory, "Gene"), "cellMetaData": read_lists(directory, "Cell"),
        "geneUsage": read_vector(j("GeneMetaDataNamesUsageCount"), np.uint32).tolist(),
        "cellUsage": read_vector(j("CellMetaDataNamesUsageCount"), np.uint32).tolist(),
        "geneFreeSlots": read_vector(j("GeneMetaData.freeSlots"), np.uint64).tolist(),
        "cellFreeSlots": read_vector(j("CellMetaData.freeSlots"), np.uint64).tolist(),
        "toc": read_vector(j("CellExpressionCounts.toc"), np.uint64).tolist(),
        "data": read_vector(j("CellExpressionCounts.data"), capi.COUNT_DTYPE).tobytes(),
        "cells": read_vector(j("Cells"), CELL_DTYPE).tobytes(),
        "allCells": read_vector(j("CellSet-AllCells"), np.uint32).tolist(),
        "allGenesGlobal": read_vector(j("GeneSet-AllGenes-GlobalIds"), np.uint32).tolist(),
        "allGenesLocal": read_vector(j("GeneSet-AllGenes-LocalIds"), np.uint32).tolist(),
    }


def file_bytes(directory):
    return {name: open(os.path.join(directory, name), "rb").read() for name in sorted(os.listdir(directory))}
