"""ExpressionMatrix: the reference's Python-bound class (src/PythonModule.cpp:158-1275) restricted to the methods of
the LSH similar-pairs path, with the same names, keyword arguments, defaults and error behaviour.

    e = ExpressionMatrix(directoryName)
    e.findSimilarPairs4(similarPairsName="Lsh")                       # tests/CaseStudy1/compute1.py:12
    e.computeLshSignatures(lshName="L"); e.findSimilarPairs5(lshName="L", similarPairsName="P", lshSliceLength=16)

Like the reference the methods return None and leave their result as files in the data directory
(SimilarPairs-<name>-*, Lsh-<name>-*), addressed by name; errors surface as RuntimeError with the reference's
message text.  The work happens in libem2lsh.so (HIP, MI355X); when torch.distributed is initialised with more
than one rank the calls are collective and the scan is row-sharded over the ranks (sharded.py)."""
import ctypes
import enum
import math

import numpy as np

from . import capi, files

_REQUIRED = object()

# getDenseExpressionMatrix fills its result in chunks of rows of at most this many bytes (one row at least): the bound of its
# device buffer.  Tests set it small to run several chunks.
DENSE_CHUNK_BYTES = 1 << 30

# addCellsFromCsr hands its barcodes to the GPU in chunks whose arrays take at most this many bytes (one barcode at least).
# Tests set it small to run several chunks.
INGEST_CHUNK_BYTES = 1 << 30

# addCells hands the text of the expression counts file to the GPU in chunks of whole lines of at most this many bytes (one
# line at least).  Tests set it small to run several chunks.  CSV_USE_DEVICE = False parses the file on the host instead.
CSV_CHUNK_BYTES = 256 << 20
CSV_USE_DEVICE = True

INVALID_ID = 0xffffffff        # invalidGeneId, invalidCellId (src/Ids.hpp)


class NormalizationMethod(enum.IntEnum):
    """NormalizationMethod (src/NormalizationMethod.hpp:11-16) with the members the reference's module exposes
    (src/PythonModule.cpp); `none` because None is a keyword."""
    none = 0
    L1 = 1
    L2 = 2


class CellGraphVertexInfo:
    """CellGraphVertexInfo (src/CellGraph.hpp:127-155) as the reference's module exposes it: cellId, x(), y(), and an
    equality that compares the cell id and the position."""
    __slots__ = ("cellId", "position")

    def __init__(self, cellId=INVALID_ID, position=(0., 0.)):
        self.cellId = cellId
        self.position = (float(position[0]), float(position[1]))

    def x(self):
        return self.position[0]

    def y(self):
        return self.position[1]

    def __eq__(self, that):
        if not isinstance(that, CellGraphVertexInfo):
            return NotImplemented
        return self.cellId == that.cellId and self.position == that.position

    __hash__ = None

    def __repr__(self):
        return "CellGraphVertexInfo(cellId=%d, x=%r, y=%r)" % (self.cellId, self.position[0], self.position[1])


# The twelve colours the page gives the twelve most frequent categories (colorPalette1, src/color.cpp:113-136).
CATEGORY_PALETTE = ("#00ff00", "#0000ff", "#ffff00", "#ff00ff", "#00ffff", "#ff8000", "#804000", "#ffa0a0", "#308000", "#900080",
                    "#9999ff", "#b0b0b0")


def _rgb_of(color):
    """0x00rrggbb of "#rrggbb"; "" (no colour) is black, as the SVG draws it.  Colour names are not parsed."""
    if color == "":
        return 0
    if len(color) == 7 and color[0] == "#" and all(c in "0123456789abcdefABCDEF" for c in color[1:]):
        return int(color[1:], 16)
    raise ValueError("drawCellGraph(): the colour %r is not of the form #rrggbb" % (color,))


def _slice_rgb_of(color):
    """0x00rrggbb of a slice's colour string: "#rrggbb", or "black"."""
    if color == "black":
        return 0
    if len(color) == 7 and color[0] == "#" and all(c in "0123456789abcdefABCDEF" for c in color[1:]):
        return int(color[1:], 16)
    raise ValueError("drawSignatureGraph(): the colour %r is neither of the form #rrggbb nor black" % (color,))


def write_png(fileName, image):
    """An uint8 [height, width, 4] array as an 8-bit RGBA PNG: one IDAT, every row with filter 0."""
    import struct
    import zlib
    image = np.ascontiguousarray(image, dtype=np.uint8)
    if image.ndim != 3 or image.shape[2] != 4:
        raise ValueError("write_png(): an uint8 [height, width, 4] array is required")
    height, width = image.shape[:2]
    rows = np.zeros((height, 1 + width * 4), dtype=np.uint8)
    rows[:, 1:] = image.reshape(height, width * 4)

    def chunk(kind, payload):
        return struct.pack(">I", len(payload)) + kind + payload + struct.pack(">I", zlib.crc32(kind + payload) & 0xffffffff)

    with open(fileName, "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", width, height, 8, 6, 0, 0, 0)) +
                chunk(b"IDAT", zlib.compress(rows.tobytes(), 6)) + chunk(b"IEND", b""))


def _b(s):
    if not isinstance(s, str):
        raise TypeError("expected a string, got %r" % (s,))
    return s.encode("utf-8")


def _distributed():
    """(dist module, world_size) if torch.distributed is up with more than one rank, else (None, 1)."""
    import sys
    if "torch" not in sys.modules:
        return None, 1
    import torch.distributed as dist
    if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
        return dist, dist.get_world_size()
    return None, 1


def topGenes(result, n):
    """Per group of a result of rankGenesByMetaData, rankGenesByClusterGraph or compareCellSets, the global ids of the n genes
    of largest z, ties broken by ascending gene id -> {group name: [gene id]}."""
    geneIds = np.asarray(result["geneIds"])
    out = {}
    for name, z in zip(result["groupNames"], np.asarray(result["zScore"])):
        order = np.lexsort((geneIds, -z))
        out[name] = geneIds[order[:int(n)]].tolist()
    return out


class ExpressionMatrix:
    def __init__(self, directoryName, allowReadOnly=False):
        # src/PythonModule.cpp:164-176 / src/ExpressionMatrix.cpp:39-52.  The reference creates the directory when it
        # does not exist; here that is the explicit ExpressionMatrix.create(directoryName), and a missing directory
        # stays an error of the constructor.  allowReadOnly is accepted for signature compatibility.
        self.directoryName = directoryName
        self._handle = ctypes.c_void_p(None)
        self._cellGraphs = {}          # ExpressionMatrix::cellGraphs (src/ExpressionMatrix.hpp): in memory only
        self._clusterGraphs = {}       # ExpressionMatrix::clusterGraphs, likewise
        self._signatureGraphs = {}     # ExpressionMatrix::signatureGraphs, likewise
        self._geneGraphs = {}          # ExpressionMatrix::geneGraphs, likewise
        capi.check(capi.load().em2_matrix_open(_b(directoryName), ctypes.byref(self._handle)))

    @classmethod
    def create(cls, directoryName):
        """ExpressionMatrix::createNew (src/ExpressionMatrix.cpp:56-101): a new directory with every file of an empty store,
        and the open matrix on it.  It is an error if the directory exists.  (The constructor never creates: a missing
        directory stays its error.)"""
        self = cls.__new__(cls)
        self.directoryName = directoryName
        self._handle = ctypes.c_void_p(None)
        self._cellGraphs, self._clusterGraphs, self._signatureGraphs, self._geneGraphs = {}, {}, {}, {}
        capi.check(capi.load().em2_matrix_create(_b(directoryName), ctypes.byref(self._handle)))
        return self

    # ---- ingest: src/PythonModule.cpp addGene, addCell, addCellsFromHdf5; the lookups of src/ExpressionMatrix.cpp:822-874 ----
    def geneCount(self):
        n = ctypes.c_uint32(0)
        capi.check(capi.load().em2_matrix_gene_count(self._handle, ctypes.byref(n)))
        return n.value

    def cellCount(self):
        n = ctypes.c_uint32(0)
        capi.check(capi.load().em2_matrix_cell_count(self._handle, ctypes.byref(n)))
        return n.value

    def addGene(self, geneName):
        """ExpressionMatrix::addGene (src/ExpressionMatrixGenes.cpp:12-39): True if the gene was added, False if the store
        had it."""
        added = ctypes.c_int(0)
        capi.check(capi.load().em2_matrix_add_gene(self._handle, _b(geneName), ctypes.byref(added)))
        return bool(added.value)

    def geneName(self, geneId):
        return self._bytes_of(capi.load().em2_matrix_gene_name, int(geneId)).decode("utf-8", "surrogateescape")

    def geneIdFromName(self, geneName):
        """The gene's id, INVALID_ID (0xffffffff, the reference's invalidGeneId) for a name the store does not have."""
        found = ctypes.c_uint32(0)
        capi.check(capi.load().em2_matrix_gene_id_from_name(self._handle, _b(geneName), ctypes.byref(found)))
        return found.value

    def cellIdFromString(self, s):
        """ExpressionMatrix::cellIdFromString (src/ExpressionMatrix.cpp:822-836): a decimal number below the cell count is that
        cell id; anything else is looked up as a cell name; INVALID_ID where there is none."""
        found = ctypes.c_uint32(0)
        capi.check(capi.load().em2_matrix_cell_id_from_string(self._handle, _b(s), ctypes.byref(found)))
        return found.value

    @staticmethod
    def _pack(strings):
        return b"".join(_b(s) + b"\0" for s in strings)

    def addCell(self, metaData, expressionCounts):
        """ExpressionMatrix::addCell (src/ExpressionMatrix.cpp:165-294): metaData is a list of (name, value) with a CellName,
        expressionCounts a list of (geneName, count); returns the cell id.  Unlike the reference's, a failing call leaves
        the store unchanged."""
        pairs = self._pack([s for pair in metaData for s in pair])
        names = self._pack([name for name, _ in expressionCounts])
        counts = np.ascontiguousarray([count for _, count in expressionCounts], dtype=np.float32)
        cell = ctypes.c_uint32(0)
        capi.check(capi.load().em2_matrix_add_cell(self._handle, pairs, len(pairs), len(metaData), names, len(names), capi._ptr(counts),
                                                   len(counts), ctypes.byref(cell)))
        return cell.value

    def addCellsFromCsr(self, geneNames, cellNames, indptr, indices, data, cellNamePrefix="", cellMetaData=(),
                        totalExpressionCountThreshold=0.):
        """The arrays of a 10X file as ExpressionMatrix::addCellsFromHdf5 (src/ExpressionMatrixHdf5.cpp:45-218) adds them:
        every gene of geneNames, then barcode i as the cell cellNamePrefix + "-" + cellNames[i] with the counts
        float(data[j]) of the genes geneNames[indices[j]], j in [indptr[i], indptr[i + 1]), and the cellMetaData pairs behind
        its CellName.  A barcode whose counts sum to less than totalExpressionCountThreshold is skipped: neither named nor
        checked.  data is an integer array (the threshold is decided on the exact row sums) or float32 (the threshold must
        be 0).  The cells' entries are prepared on the GPU in chunks of at most INGEST_CHUNK_BYTES bytes.  All or nothing:
        on any error no gene and no cell is added, and the error is that of the lowest failing barcode.  Returns the ids of
        the added cells as a range."""
        indptr = np.asarray(indptr)
        indices = np.asarray(indices)
        data = np.asarray(data)
        if indptr.ndim != 1 or indices.ndim != 1 or data.ndim != 1 or len(indptr) != len(cellNames) + 1 or len(indices) != len(data):
            raise RuntimeError("addCellsFromCsr: indptr must have one entry more than cellNames, indices as many as data")
        if len(indptr) and (np.any(indptr < 0) or np.any(indices < 0)):
            raise RuntimeError("addCellsFromCsr: a negative offset or index")
        if len(indices) and int(indices.max()) >= len(geneNames):
            raise RuntimeError("addCellsFromCsr: an index is not below the number of gene names")
        indptr = np.ascontiguousarray(indptr, dtype=np.uint64)
        indices = np.ascontiguousarray(indices, dtype=np.uint32)
        threshold = float(totalExpressionCountThreshold)
        skip = None
        if data.dtype.kind in "iu":
            if threshold > 0.:
                # the reference adds the uint32 counts in double; exact while the sums stay below 2^53, as are these
                ends = np.concatenate([[0], np.cumsum(data.astype(object) if data.dtype.itemsize == 8 else data.astype(np.int64))])
                ok = len(indptr) and indptr[0] == 0 and np.all(np.diff(indptr.astype(np.int64)) >= 0) and indptr[-1] == len(data)
                if ok:
                    sums = ends[indptr[1:].astype(np.int64)] - ends[indptr[:-1].astype(np.int64)]
                    skip = np.ascontiguousarray(np.asarray([s < threshold for s in sums], dtype=np.uint8))
        elif data.dtype == np.float32:
            if threshold != 0.:
                raise RuntimeError("addCellsFromCsr: float32 data takes no totalExpressionCountThreshold")
        else:
            raise RuntimeError("addCellsFromCsr: data must be an integer array or float32")
        values = np.ascontiguousarray(data, dtype=np.float32)
        genes, cells = self._pack(geneNames), self._pack(cellNames)
        pairs = self._pack([s for pair in cellMetaData for s in pair])
        first, added = ctypes.c_uint32(0), ctypes.c_uint32(0)
        capi.check(capi.load().em2_matrix_add_cells_csr(
            self._handle, genes, len(genes), len(geneNames), cells, len(cells), len(cellNames), capi._ptr(indptr), capi._ptr(indices),
            capi._ptr(values), len(values), capi._ptr(skip) if skip is not None else None, _b(cellNamePrefix), pairs, len(pairs),
            len(cellMetaData), int(INGEST_CHUNK_BYTES), ctypes.byref(first), ctypes.byref(added)))
        return range(first.value, first.value + added.value)

    def addCells(self, expressionCountsFileName=_REQUIRED, expressionCountsFileSeparators=",", cellMetaDataFileName=_REQUIRED,
                 cellMetaDataFileSeparators=",", additionalCellMetaData=()):
        """ExpressionMatrix::addCells (src/ExpressionMatrix.cpp:380-654): the cells named both by the header of the expression
        counts file (genes x cells, a gene per line) and by the first column of the cell meta data file, in the order of the
        expression counts file's columns, each with additionalCellMetaData, its CellName and the meta data file's fields.
        Every gene line adds its gene.  The text of the expression counts file is parsed on the GPU in chunks of whole lines
        of at most CSV_CHUNK_BYTES bytes; a separator string of more than 8 characters, or one with a quote, a backslash or a
        line end, and CSV_USE_DEVICE = False send the whole file down the host path, with the same result.  All or nothing;
        the reference's error texts (include/em2_lsh.h, em2_matrix_add_cells_csv, lists the departures).  Returns None, like
        the reference; lastCsvDeferredFieldCount is the number of fields the GPU left to the host in this call."""
        if expressionCountsFileName is _REQUIRED or cellMetaDataFileName is _REQUIRED:
            raise TypeError("addCells() needs expressionCountsFileName and cellMetaDataFileName")
        additionalCellMetaData = list(additionalCellMetaData)
        pairs = self._pack([s for pair in additionalCellMetaData for s in pair])
        first, added, deferred = ctypes.c_uint32(0), ctypes.c_uint32(0), ctypes.c_uint64(0)
        capi.check(capi.load().em2_matrix_add_cells_csv(
            self._handle, _b(expressionCountsFileName), _b(expressionCountsFileSeparators), _b(cellMetaDataFileName),
            _b(cellMetaDataFileSeparators), pairs, len(pairs), len(additionalCellMetaData), int(CSV_CHUNK_BYTES),
            1 if CSV_USE_DEVICE else 0, ctypes.byref(first), ctypes.byref(added), ctypes.byref(deferred)))
        self.lastCsvDeferredFieldCount = deferred.value

    def addCellMetaData(self, cellMetaDataFileName):
        """ExpressionMatrix::addCellMetaData (src/ExpressionMatrixBioHub.cpp:337-392): a comma separated file whose first
        column names cells of the store and whose other columns are meta data fields, named by the header (its first token is
        ignored, a column with an empty name is skipped); setCellMetaData per cell and field, in file order.  Host only.
        All or nothing, unlike the reference's."""
        capi.check(capi.load().em2_matrix_add_cell_meta_data_csv(self._handle, _b(cellMetaDataFileName)))

    def close(self):
        self._signatureGraphs = {}
        self._geneGraphs = {}
        if self._handle:
            lib = capi.load()
            try:
                capi.check(lib.em2_matrix_flush(self._handle))       # (em2_matrix_close flushes too, but cannot say that it failed)
            finally:
                lib.em2_matrix_close(self._handle)
                self._handle = ctypes.c_void_p(None)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- src/PythonModule.cpp:802-824 ----
    def findSimilarPairs4(self, geneSetName="AllGenes", cellSetName="AllCells", similarPairsName=_REQUIRED, k=100,
                          similarityThreshold=0.2, lshCount=1024, seed=231):
        if similarPairsName is _REQUIRED:
            raise TypeError("findSimilarPairs4(): missing required argument 'similarPairsName'")
        dist, world = _distributed()
        if dist is not None:
            from . import sharded
            return sharded.find_similar_pairs4_collective(self, geneSetName, cellSetName, similarPairsName, k,
                                                          similarityThreshold, lshCount, seed, dist)
        capi.check(capi.load().em2_matrix_find_similar_pairs4(self._handle, _b(geneSetName), _b(cellSetName),
                                                              _b(similarPairsName), k, similarityThreshold,
                                                              lshCount, seed))

    # ---- src/PythonModule.cpp:776-801: the exact all-pairs search ("slow", the reference says; here it is a device scan) ----
    def findSimilarPairs0(self, geneSetName="AllGenes", cellSetName="AllCells", similarPairsName=_REQUIRED, k=100,
                          similarityThreshold=0.2):
        if similarPairsName is _REQUIRED:
            raise TypeError("findSimilarPairs0(): missing required argument 'similarPairsName'")
        capi.check(capi.load().em2_matrix_find_similar_pairs0(self._handle, _b(geneSetName), _b(cellSetName),
                                                              _b(similarPairsName), k, similarityThreshold))

    # ---- src/PythonModule.cpp:966-980: gene-gene correlations, all pairs ----
    def findSimilarGenePairs0(self, geneSetName="AllGenes", cellSetName="AllCells", normalizationMethod=NormalizationMethod.L2,
                              similarGenePairsName=_REQUIRED, k=100, similarityThreshold=0.2, writeCsv=False):
        """ExpressionMatrix::findSimilarGenePairs0 (src/ExpressionMatrixFindSimilarGenePairs.cpp:16-198): writes
        SimilarGenePairs-<name>-{Info,Pairs,GeneInfo}."""
        if similarGenePairsName is _REQUIRED:
            raise TypeError("findSimilarGenePairs0(): missing required argument 'similarGenePairsName'")
        if writeCsv:
            raise NotImplementedError("findSimilarGenePairs0(): writeCsv=True (two text lines per pair of genes) is not "
                                      "implemented; read the stored pairs with files.read_similar_gene_pairs")
        method = NormalizationMethod(normalizationMethod)                   # (ValueError for anything else, None included)
        capi.apply_gene_pairs_buffer()
        capi.check(capi.load().em2_matrix_find_similar_gene_pairs0(self._handle, _b(geneSetName), _b(cellSetName), int(method),
                                                                   _b(similarGenePairsName), k, similarityThreshold))

    def removeSimilarGenePairs(self, similarGenePairsName):
        capi.check(capi.load().em2_matrix_remove_similar_gene_pairs(self._handle, _b(similarGenePairsName)))

    # ---- src/PythonModule.cpp:506-537 ----
    def createGeneSetUsingInformationContent(self, existingGeneSetName="AllGenes", cellSetName="AllCells",
                                             normalizationMethod=_REQUIRED, geneInformationContentThreshold=_REQUIRED,
                                             newGeneSetName=_REQUIRED):
        """ExpressionMatrix::createGeneSetUsingInformationContent (src/ExpressionMatrix.cpp:2022-2082): the genes of the
        existing set whose information content over the cell set exceeds the threshold (bits), as a new gene set that the
        next call can name."""
        if _REQUIRED in (normalizationMethod, geneInformationContentThreshold, newGeneSetName):
            raise TypeError("createGeneSetUsingInformationContent(): normalizationMethod, geneInformationContentThreshold and "
                            "newGeneSetName are required")
        method = NormalizationMethod(normalizationMethod)
        capi.check(capi.load().em2_matrix_create_gene_set_using_information_content(
            self._handle, _b(existingGeneSetName), _b(cellSetName), int(method), geneInformationContentThreshold,
            _b(newGeneSetName)))

    # ---- src/PythonModule.cpp:586-602 ----
    def createWellExpressedGeneSet(self, inputGeneSetName="AllGenes", inputCellSetName="AllCells", outputGeneSetName=_REQUIRED,
                                   minCellCount=_REQUIRED):
        """ExpressionMatrix::createWellExpressedGeneSet (src/ExpressionMatrixGeneSets.cpp:314-362): the genes of the input set
        with a stored entry in at least minCellCount cells of the cell set."""
        if _REQUIRED in (outputGeneSetName, minCellCount):
            raise TypeError("createWellExpressedGeneSet(): outputGeneSetName and minCellCount are required")
        if not 0 <= int(minCellCount) <= 0xffffffff:             # CellId (src/Ids.hpp) is unsigned, 32 bits
            raise ValueError("createWellExpressedGeneSet(): minCellCount must be in [0, 2**32)")
        capi.check(capi.load().em2_matrix_create_well_expressed_gene_set(self._handle, _b(inputGeneSetName), _b(inputCellSetName),
                                                                         _b(outputGeneSetName), int(minCellCount)))

    def removeGeneSet(self, geneSetName):
        """ExpressionMatrix::removeGeneSet (src/ExpressionMatrixGeneSets.cpp:12-32)."""
        capi.check(capi.load().em2_matrix_remove_gene_set(self._handle, _b(geneSetName)))

    # ---- src/PythonModule.cpp:539-584 ----
    def _gene_set_operation(self, entry, *names):
        created = ctypes.c_int(0)
        capi.check(entry(self._handle, *[_b(name) for name in names], ctypes.byref(created)))
        if not created.value:
            print(capi.last_error())             # the reference writes the line to cout and returns false; it does not throw
        return bool(created.value)

    def createGeneSetIntersection(self, inputSets, outputSet):
        """ExpressionMatrix::createGeneSetIntersection (src/ExpressionMatrixGeneSets.cpp:183-250): inputSets is a
        comma-separated list of gene set names.  False, and a printed line, when the output exists or an input is missing."""
        return self._gene_set_operation(capi.load().em2_matrix_create_gene_set_intersection, inputSets, outputSet)

    def createGeneSetUnion(self, inputSets, outputSet):
        """ExpressionMatrix::createGeneSetUnion (src/ExpressionMatrixGeneSets.cpp:187-250), as createGeneSetIntersection."""
        return self._gene_set_operation(capi.load().em2_matrix_create_gene_set_union, inputSets, outputSet)

    def createGeneSetDifference(self, inputSet0, inputSet1, outputSet):
        """ExpressionMatrix::createGeneSetDifference (src/ExpressionMatrixGeneSets.cpp:254-305): the genes of inputSet0 that
        are not in inputSet1.  False, and a printed line, when the output exists or an input is missing."""
        return self._gene_set_operation(capi.load().em2_matrix_create_gene_set_difference, inputSet0, inputSet1, outputSet)

    def getGeneSetGenes(self, geneSetName):
        """The global ids of the genes of a gene set, ascending (src/ExpressionMatrixGeneSets.cpp:57-63)."""
        lib = capi.load()
        count = ctypes.c_uint32(0)
        capi.check(lib.em2_matrix_gene_set(self._handle, _b(geneSetName), ctypes.byref(count), None))
        ids = np.zeros(count.value, dtype=np.uint32)
        capi.check(lib.em2_matrix_gene_set(self._handle, _b(geneSetName), ctypes.byref(count), capi._ptr(ids)))
        return ids.tolist()

    def computeGeneInformationContent(self, geneSetName, cellSetName, normalizationMethod):
        """ExpressionMatrix::computeGeneInformationContent (src/ExpressionMatrix.cpp:1947-2018) -> float32 array, one value
        (bits) per gene of the gene set.  The reference keeps this method private and shows its values only in its HTTP page;
        it is public here because createGeneSetUsingInformationContent is a threshold on exactly these floats."""
        method = NormalizationMethod(normalizationMethod)
        lib = capi.load()
        count = ctypes.c_uint32(0)
        capi.check(lib.em2_matrix_gene_set(self._handle, _b(geneSetName), ctypes.byref(count), None))
        out = np.zeros(count.value, dtype=np.float32)
        capi.check(lib.em2_matrix_gene_information_content(self._handle, _b(geneSetName), _b(cellSetName), int(method), capi._ptr(out)))
        return out

    # ---- rank-sum marker genes (the reference has no such test) ----
    def _rank_genes(self, geneSetName, cellSetName, normalizationMethod, group, groupNames):
        """em2_matrix_rank_genes over the cells of a cell set: group is uint32 per cell of the set, in its order (a group,
        capi.NO_GROUP, or capi.GROUP_EXCLUDED for a cell that is not part of the universe) -> the dict of the public methods."""
        method = NormalizationMethod(normalizationMethod)
        geneIds = np.asarray(self.getGeneSetGenes(geneSetName), dtype=np.uint32)
        group = np.ascontiguousarray(group, dtype=np.uint32)
        groupCount = len(groupNames)
        if groupCount == 0:
            raise ValueError("there is no group to rank genes for")
        out = capi.rank_genes_arrays(len(geneIds), groupCount)
        capi.check(capi.load().em2_matrix_rank_genes(self._handle, _b(geneSetName), _b(cellSetName), int(method), capi._ptr(group),
                                                     groupCount, capi._ptr(out["groupSize"]), capi._ptr(out["nonZeroCount"]),
                                                     capi._ptr(out["rankSum2"]), capi._ptr(out["tieSum"]), capi._ptr(out["zScore"]),
                                                     capi._ptr(out["auc"])))
        zScore = np.ascontiguousarray(out["zScore"].T)
        pValue = np.array([math.erfc(abs(z) / math.sqrt(2.)) for z in zScore.reshape(-1).tolist()], dtype=np.float64).reshape(zScore.shape)
        return {"groupNames": list(groupNames), "groupSizes": out["groupSize"], "geneIds": geneIds, "zScore": zScore,
                "auc": np.ascontiguousarray(out["auc"].T), "pValue": pValue, "nonZeroCount": np.ascontiguousarray(out["nonZeroCount"].T),
                "rankSum2": np.ascontiguousarray(out["rankSum2"].T), "tieSum": out["tieSum"]}

    def rankGenesByMetaData(self, geneSetName="AllGenes", cellSetName="AllCells", metaDataName=_REQUIRED,
                            normalizationMethod=NormalizationMethod.L2):
        """The rank-sum (Mann-Whitney / Wilcoxon) test of every gene of the gene set, for every value of a meta data field over
        the cell set against the cells of all other values, on the GPU (em2_matrix_rank_genes).  The groups are the values in
        the order of histogramMetaData (count descending, then value ascending); a cell without the field has the value ""
        like any other.  A cell's value for a gene is its count times the cell's norm inverse (over its whole row), 0 where
        nothing is stored.  -> dict of numpy arrays: groupNames, groupSizes [K], geneIds (global) [G], zScore, auc, pValue
        (two-sided, normal approximation without continuity correction, erfc(|z| / sqrt(2))), nonZeroCount, rankSum2, each
        [K][G], and tieSum [G].  The integers (nonZeroCount, rankSum2 = twice the group's rank sum, tieSum) determine the rest."""
        if metaDataName is _REQUIRED:
            raise TypeError("rankGenesByMetaData(): metaDataName is required")
        self.getGeneSetGenes(geneSetName)                                # "Gene set X does not exist."
        cells = self._cell_set(cellSetName)                               # "Cell set X does not exist."
        if len(cells) == 0:
            raise RuntimeError("Cell set " + cellSetName + " is empty.")
        handle = ctypes.c_void_p(None)
        capi.check(capi.load().em2_matrix_meta_data_table(self._handle, _b(cellSetName), _b(metaDataName), None, ctypes.byref(handle)))
        t = capi.meta_data_table_take(handle, cell_rows=True)
        return self._rank_genes(geneSetName, cellSetName, normalizationMethod, t["cellRow"], t["values0"])

    def rankGenesByClusterGraph(self, clusterGraphName, geneSetName=None, normalizationMethod=NormalizationMethod.L2):
        """rankGenesByMetaData for the clusters of a cluster graph: the universe is the cells of the cluster graph's cell
        graph, the groups are its clusters in the order of getClusterGraphVertices (groupNames holds their ids), and a cell of
        the graph that is in no cluster belongs to no group but to every "rest".  geneSetName None: the graph's own gene set."""
        c = self._cluster_graph(clusterGraphName)
        clusterIds = self.getClusterGraphVertices(clusterGraphName)
        r = c["result"]
        cellSetName = c["cellSetName"]
        cells = self._cell_set(cellSetName)
        groupOfCell = {}
        for group, clusterId in enumerate(clusterIds):
            at = c["position"][clusterId]
            for cellId in c["vertexCellIds"][r["cells"][int(r["cellOffsets"][at]):int(r["cellOffsets"][at + 1])]].tolist():
                groupOfCell[cellId] = group
        inGraph = set(c["vertexCellIds"].tolist())
        group = np.array([groupOfCell.get(cellId, capi.NO_GROUP) if cellId in inGraph else capi.GROUP_EXCLUDED for cellId in cells.tolist()],
                         dtype=np.uint32)
        return self._rank_genes(c["geneSetName"] if geneSetName is None else geneSetName, cellSetName, normalizationMethod, group,
                                clusterIds)

    def compareCellSets(self, geneSetName=_REQUIRED, cellSetName0=_REQUIRED, cellSetName1=_REQUIRED,
                        normalizationMethod=NormalizationMethod.L2):
        """rankGenesByMetaData for two cell sets against each other: the universe is their union, the groups are the two sets
        (groupNames holds their names), so z of group 0 is minus z of group 1.  Sets that share a cell raise ValueError."""
        if _REQUIRED in (geneSetName, cellSetName0, cellSetName1):
            raise TypeError("compareCellSets(): geneSetName, cellSetName0 and cellSetName1 are required")
        self.getGeneSetGenes(geneSetName)
        cells0, cells1 = self._cell_set(cellSetName0), self._cell_set(cellSetName1)
        if len(np.intersect1d(cells0, cells1)):
            raise ValueError("compareCellSets(): the cell sets " + cellSetName0 + " and " + cellSetName1 + " share a cell")
        allCells = self._cell_set("AllCells")
        group = np.full(len(allCells), capi.GROUP_EXCLUDED, dtype=np.uint32)
        group[np.isin(allCells, cells0)] = 0
        group[np.isin(allCells, cells1)] = 1
        return self._rank_genes(geneSetName, "AllCells", normalizationMethod, group, [cellSetName0, cellSetName1])

    # ---- src/PythonModule.cpp:755-771 ----
    def computeCellSimilarity(self, geneSetName="AllGenes", cellId0=_REQUIRED, cellId1=_REQUIRED):
        """The exact similarity of two cells (global ids) over the genes of a gene set."""
        if cellId0 is _REQUIRED or cellId1 is _REQUIRED:
            raise TypeError("computeCellSimilarity(): cellId0 and cellId1 are required")
        similarity = ctypes.c_double(0.)
        capi.check(capi.load().em2_matrix_compute_cell_similarity(self._handle, _b(geneSetName), cellId0, cellId1,
                                                                  ctypes.byref(similarity)))
        return similarity.value

    # ---- src/PythonModule.cpp:921-925: bound without argument names or defaults ("Only intended to be used for testing") ----
    def analyzeSimilarPairs(self, similarPairsName, csvDownsample):
        """Writes <similarPairsName>-analysis.csv and <similarPairsName>-analysis-statistics.csv into the working
        directory (src/ExpressionMatrixLsh.cpp:72, :133)."""
        capi.check(capi.load().em2_matrix_analyze_similar_pairs(self._handle, _b(similarPairsName), csvDownsample, None))

    # ---- src/PythonModule.cpp:935-939 ("Only intended to be used for testing") ----
    def compareSimilarPairs(self, similarPairsName0, similarPairsName1):
        """Writes CompareSimilarPairs.csv into the working directory (src/ExpressionMatrixLsh.cpp:1212)."""
        capi.check(capi.load().em2_matrix_compare_similar_pairs(self._handle, _b(similarPairsName0), _b(similarPairsName1),
                                                                None))

    # ---- src/PythonModule.cpp:945-953 ----
    def computeLshSignatures(self, geneSetName="AllGenes", cellSetName="AllCells", lshName=_REQUIRED, lshCount=1024,
                             seed=231):
        if lshName is _REQUIRED:
            raise TypeError("computeLshSignatures(): missing required argument 'lshName'")
        capi.check(capi.load().em2_matrix_compute_lsh_signatures(self._handle, _b(geneSetName), _b(cellSetName),
                                                                 _b(lshName), lshCount, seed))

    # ---- src/PythonModule.cpp:940-944: bound without argument names or defaults ("Only intended to be used for testing") ----
    def analyzeLsh(self, geneSetName, cellSetName, lshCount, seed, csvDownsample):
        """Writes Lsh-analysis.csv and LSH-analysis-statistics.csv into the working directory
        (src/ExpressionMatrixLsh.cpp:1303, :1345)."""
        capi.check(capi.load().em2_matrix_analyze_lsh(self._handle, _b(geneSetName), _b(cellSetName), lshCount, seed,
                                                      csvDownsample, None))

    # ---- src/PythonModule.cpp:954-962 ----
    def analyzeLshSignatures(self, geneSetName="AllGenes", cellSetName="AllCells", lshCount=1024, seed=231):
        """ExpressionMatrix::analyzeLshSignatures (src/ExpressionMatrixLsh.cpp:1372-1474): writes Signatures.csv, Histogram.csv
        and LshSignatureStatistics.csv into the working directory.  The cells are grouped by signature and the bits counted on
        the GPU (em2_analyze_lsh_signatures)."""
        capi.check(capi.load().em2_matrix_analyze_lsh_signatures(self._handle, _b(geneSetName), _b(cellSetName), lshCount, seed,
                                                                 None))

    # ---- src/PythonModule.cpp:984-1004 ----
    def createSignatureGraph(self, signatureGraphName=_REQUIRED, cellSetName="AllCells", lshName=_REQUIRED,
                             minCellCount=_REQUIRED):
        """ExpressionMatrix::createSignatureGraph (src/ExpressionMatrixSignatureGraph.cpp:42-150): a vertex per signature that
        at least minCellCount cells of the cell set share, an edge between signatures that differ in one bit
        (em2_signature_graph_create, on the GPU).  The graph lives in memory, like the reference's; SignatureGraph.svg is not
        written."""
        if _REQUIRED in (signatureGraphName, lshName, minCellCount):
            raise TypeError("createSignatureGraph(): signatureGraphName, lshName and minCellCount are required")
        _b(signatureGraphName)
        if isinstance(minCellCount, float) or not 0 <= int(minCellCount) < 2 ** 64:        # size_t (:46)
            raise ValueError("createSignatureGraph(): minCellCount must be an integer in [0, 2**64)")
        if signatureGraphName in self._signatureGraphs:
            raise RuntimeError("Signature graph " + signatureGraphName + " already exists.")       # :22-24
        handle = ctypes.c_void_p(None)
        capi.check(capi.load().em2_matrix_create_signature_graph(self._handle, _b(cellSetName), _b(lshName), int(minCellCount),
                                                                 ctypes.byref(handle)))
        graph = capi.signature_graph_take(handle)
        graph["cellSet"] = self._cell_set(cellSetName)
        self._signatureGraphs[signatureGraphName] = graph

    def removeSignatureGraph(self, signatureGraphName):
        self._signature_graph(signatureGraphName)
        del self._signatureGraphs[signatureGraphName]

    def _signature_graph(self, signatureGraphName):
        if signatureGraphName not in self._signatureGraphs:
            raise RuntimeError("Signature graph " + signatureGraphName + " does not exists.")      # sic, :34, :157
        return self._signatureGraphs[signatureGraphName]

    # The reference shows a signature graph through its HTTP pages only; these four accessors are this package's.
    def getSignatureGraphNames(self):
        return sorted(self._signatureGraphs)

    def getSignatureGraphVertices(self, signatureGraphName):
        """(signatures uint64 [vertices, words], cell counts uint64 [vertices]), in vertex order: the order of the reference's
        std::map of signatures."""
        g = self._signature_graph(signatureGraphName)
        return g["vertexSignatures"].copy(), np.diff(g["cellOffsets"])

    def getSignatureGraphCells(self, signatureGraphName, vertexId):
        """(local cell ids, global cell ids) of a vertex: SignatureGraphVertex::localCellIds / globalCellIds, ascending."""
        g = self._signature_graph(signatureGraphName)
        if not 0 <= vertexId < len(g["cellOffsets"]) - 1:
            raise RuntimeError("Vertex " + str(vertexId) + " of signature graph " + signatureGraphName + " does not exist.")
        local = g["cells"][int(g["cellOffsets"][vertexId]):int(g["cellOffsets"][vertexId + 1])]
        return local.copy(), g["cellSet"][local]

    def getSignatureGraphEdges(self, signatureGraphName):
        """(vertex 0, vertex 1) per edge, uint32, in the order SignatureGraph::createEdges adds them; vertex 1 > vertex 0."""
        g = self._signature_graph(signatureGraphName)
        return g["edgeVertex0"].copy(), g["edgeVertex1"].copy()

    # ---- SignatureGraph::computeLayout, the colourings and SignatureGraph::writeSvg (src/SignatureGraph.cpp:105-321,
    # src/ExpressionMatrixSignatureGraph.cpp:163-278, src/ExpressionMatrixHttpServerSignatureGraphs.cpp:45-95) without the page ----
    def computeSignatureGraphLayout(self, signatureGraphName, seed=231, maxIterationCount=300, tolerance=0.01, gravity=0.02,
                                    repulsion="exact", levels="single"):
        """SignatureGraph::computeLayout (src/SignatureGraph.cpp:105-171).  The reference runs Graphviz's sfdp; here the layout
        entries of computeCellGraphLayout run over the graph's edges, with the same arguments, the same meaning and the same
        validation (em2_graph_layout, em2_graph_layout_pyramid, em2_graph_layout_multilevel).  The reference also hands sfdp a
        width per vertex and a weight per edge (computed from source(e) twice, :93-97); neither enters this force model.
        Computed once per graph, like the reference's layoutWasComputed: a second call does nothing."""
        if repulsion not in ("exact", "pyramid"):
            raise ValueError('repulsion must be "exact" or "pyramid", not %r' % (repulsion,))
        if levels not in ("single", "multi"):
            raise ValueError('levels must be "single" or "multi", not %r' % (levels,))
        g = self._signature_graph(signatureGraphName)
        if "layout" in g:
            return
        vertexCount = len(g["cellOffsets"]) - 1
        v0, v1 = g["edgeVertex0"], g["edgeVertex1"]
        parameters = capi.LayoutParameters(seed=seed, maxIterationCount=maxIterationCount, tolerance=tolerance, gravity=gravity)
        if levels == "multi":
            depth = capi.LAYOUT_DEPTH_EXACT if repulsion == "exact" else capi.LAYOUT_DEPTH_AUTO
            x, y = capi.graph_layout_multilevel(vertexCount, v0, v1, parameters, depth)[:2]
        else:
            layout = capi.graph_layout if repulsion == "exact" else capi.graph_layout_pyramid
            x, y, _, _, _ = layout(vertexCount, v0, v1, parameters)
        g["layout"] = (x.astype(np.float64), y.astype(np.float64))

    def _laid_out_signature_graph(self, signatureGraphName):
        g = self._signature_graph(signatureGraphName)
        if "layout" not in g:
            raise RuntimeError("Layout for signature graph " + signatureGraphName + " is not available.")
        return g

    def getSignatureGraphLayout(self, signatureGraphName):
        """(x, y) of the vertices, float64 copies, in vertex order."""
        x, y = self._laid_out_signature_graph(signatureGraphName)["layout"]
        return x.copy(), y.copy()

    def computeSignatureGraphColors(self, signatureGraphName, coloringOption="random", metaDataName=None, metaDataMeaning="category"):
        """The colouring of the page's request (src/ExpressionMatrixHttpServerSignatureGraphs.cpp:81-94), stored with the graph
        for writeSignatureGraphSvg and drawSignatureGraph and returned as a dict: every vertex gets a list of (colour,
        fraction), its slices.
          coloringOption "byMetaData"  by the field metaDataName; metaDataMeaning "category" (colorByMetaDataInterpretedAsCategory:
                                       the values by their cells over the graph's vertices, the twelve colours of the palette
                                       and "black" from the thirteenth value on; per vertex the cells of each colour, counted
                                       on the GPU: em2_matrix_pie_census); "color" and "number" raise the reference's
                                       "... is not implemented.";
                         "random"      colorRandom: a colour per vertex from std::mt19937(231);
                         anything else colorBlack.
        Returns sliceOffsets (uint64 [vertices + 1]), sliceCells (uint32), sliceFraction (float64) and colors (a str) per slice,
        sliceColor (the colour index 0 .. 12 per slice, "category" only, else None) and valueTable ([(value, cells, colour)] in
        the reference's sorted order, "category" only, else [])."""
        g = self._signature_graph(signatureGraphName)
        cellOffsets = np.ascontiguousarray(g["cellOffsets"], dtype=np.uint64)
        vertexCount = len(cellOffsets) - 1
        whole = {"sliceOffsets": np.arange(vertexCount + 1, dtype=np.uint64), "sliceColor": None,
                 "sliceCells": np.diff(cellOffsets).astype(np.uint32), "sliceFraction": np.ones(vertexCount, dtype=np.float64),
                 "valueTable": []}
        if coloringOption == "byMetaData":
            if metaDataMeaning == "number":
                raise RuntimeError("Signature graph coloring by meta data interpreted as number is not implemented.")      # :277
            if metaDataMeaning == "color":
                raise RuntimeError("Signature graph coloring by meta data interpreted as color is not implemented.")       # :270
            if metaDataName is None:
                raise TypeError("computeSignatureGraphColors(): byMetaData needs metaDataName")
            cells = np.ascontiguousarray(g["cells"], dtype=np.uint32)
            cellSet = np.ascontiguousarray(g["cellSet"], dtype=np.uint32)
            handle = ctypes.c_void_p(None)
            capi.check(capi.load().em2_matrix_pie_census(self._handle, vertexCount, capi._ptr(cellOffsets), capi._ptr(cells), len(cells),
                                                         capi._ptr(cellSet), len(cellSet), _b(metaDataName), ctypes.byref(handle)))
            census = capi.pie_census_take(handle)
            palette = CATEGORY_PALETTE + ("black",)
            result = {key: census[key] for key in ("sliceOffsets", "sliceColor", "sliceCells", "sliceFraction")}
            result["colors"] = [palette[index] for index in census["sliceColor"].tolist()]
            result["valueTable"] = [(value, count, palette[min(rank, 12)])
                                    for rank, (value, count) in enumerate(zip(census["values"], census["valueCells"]))]
        elif coloringOption == "random":
            result = dict(whole, colors=capi.color_strings(capi.signature_graph_random_colors(vertexCount)))
        else:
            result = dict(whole, colors=["black"] * vertexCount)
        g["coloring"] = result
        return dict(result)

    @staticmethod
    def _signature_graph_view(g, xShift, yShift, zoomFactor):
        """SignatureGraph::writeSvg's view (src/SignatureGraph.cpp:194-229), as written: like CellGraph's, the maxima start at
        numeric_limits<double>::min() (see _cell_graph_view).  -> xCenter, yCenter, halfViewBoxSize, boundingBoxSize."""
        x, y = g["layout"]
        largest, tiny = float(np.finfo(np.float64).max), float(np.finfo(np.float64).tiny)
        xMin, xMax = min([largest] + ([float(x.min())] if len(x) else [])), max([tiny] + ([float(x.max())] if len(x) else []))
        yMin, yMax = min([largest] + ([float(y.min())] if len(y) else [])), max([tiny] + ([float(y.max())] if len(y) else []))
        boundingBoxSize = max(xMax - xMin, yMax - yMin)
        viewBoxSize = 1.05 * boundingBoxSize / float(zoomFactor)
        return (xMin + xMax) / 2. - float(xShift), (yMin + yMax) / 2. - float(yShift), viewBoxSize / 2., boundingBoxSize

    def writeSignatureGraphSvg(self, signatureGraphName, fileName, hideEdges=False, svgSizePixels=500, xShift=0., yShift=0.,
                               zoomFactor=1., vertexSizeFactor=1., edgeThicknessFactor=1.):
        """SignatureGraph::writeSvg (src/SignatureGraph.cpp:183-321) into fileName, byte for byte, with the colouring
        computeSignatureGraphColors stored last; before any, every vertex is the black circle that the reference's
        createSignatureGraph writes into SignatureGraph.svg.  The arguments are SvgParameters' (src/SignatureGraph.hpp:84-100).
        A vertex is a circle whose area follows its cell count, a pie chart where it has several colours; the vertices are
        written by decreasing cell count, in std::sort's order.  Written by the host (em2_signature_graph_write_svg).
        Returns the four fields the reference fills in: {"xCenter", "yCenter", "halfViewBoxSize", "pixelSize"}."""
        g = self._laid_out_signature_graph(signatureGraphName)
        x, y = g["layout"]
        coloring = g.get("coloring")
        parameters = capi.signature_graph_write_svg(
            fileName, x, y, np.diff(g["cellOffsets"]), g["edgeVertex0"], g["edgeVertex1"], hideEdges, svgSizePixels, xShift, yShift,
            zoomFactor, vertexSizeFactor, edgeThicknessFactor, slice_offsets=coloring["sliceOffsets"] if coloring else None,
            slice_colors=coloring["colors"] if coloring else None, slice_fraction=coloring["sliceFraction"] if coloring else None)
        return dict(zip(("xCenter", "yCenter", "halfViewBoxSize", "pixelSize"), parameters))

    def drawSignatureGraph(self, signatureGraphName, fileName=None, sizePixels=1024, edgeShade=255, hideEdges=False, xShift=0.,
                           yShift=0., zoomFactor=1., vertexSizeFactor=1.):
        """The picture of writeSignatureGraphSvg as an image, rastered on the GPU (em2_graph_draw_pies, em2_graph_compose; the
        definition is in include/em2_lsh.h): uint8 [sizePixels, sizePixels, 4], rows from the top, r g b a.  The view is the
        SVG's with sizePixels in the place of svgSizePixels; a vertex has the SVG's radius, vertexSizeFactor * (0.03 *
        boundingBoxSize * sqrt(cells / most cells)), and the vertices are painted in the SVG's order.  The slice boundaries
        come from the SVG's angles (em2_pie_boundaries).  No anti-aliasing; the edges are one-pixel lines as in drawCellGraph.
        Before any colouring every vertex is black.  A colour that is neither #rrggbb nor "black" raises ValueError.
        With fileName the image is also written as a PNG."""
        g = self._laid_out_signature_graph(signatureGraphName)
        x, y = g["layout"]
        xc, yc, half, boundingBoxSize = self._signature_graph_view(g, xShift, yShift, zoomFactor)
        cellCounts = np.diff(np.ascontiguousarray(g["cellOffsets"], dtype=np.uint64))
        vertexCount = len(cellCounts)
        coloring = g.get("coloring")
        if coloring:
            offsets, fraction = coloring["sliceOffsets"].astype(np.int64), coloring["sliceFraction"]
            rgb = np.asarray([_slice_rgb_of(c) for c in coloring["colors"]], dtype=np.uint32)
        else:
            offsets, fraction, rgb = np.arange(vertexCount + 1, dtype=np.int64), np.ones(vertexCount), np.zeros(vertexCount, dtype=np.uint32)
        if (np.diff(offsets) < 1).any():
            raise RuntimeError("drawSignatureGraph(): a vertex of signature graph " + signatureGraphName + " has no cell")
        largest = float(np.uint32(cellCounts.max(initial=0)))
        with np.errstate(all="ignore"):
            radius = float(vertexSizeFactor) * (0.03 * boundingBoxSize * np.sqrt(cellCounts.astype(np.uint32).astype(np.float64) / largest))
        # the SVG's painter order: sortedVertices
        order = capi.order_by_count(cellCounts)
        position = np.empty(vertexCount, dtype=np.uint32)
        position[order] = np.arange(vertexCount, dtype=np.uint32)
        sliceCounts = np.diff(offsets)[order]
        newOffsets = np.concatenate([[0], np.cumsum(sliceCounts)]).astype(np.int64)
        gather = np.repeat(offsets[:-1][order] - newOffsets[:-1], sliceCounts) + np.arange(int(newOffsets[-1]), dtype=np.int64)
        bx, by, arc = capi.pie_boundaries(newOffsets, fraction[gather])
        _, sliceTop, edgeHits = capi.graph_draw_pies(x[order], y[order], radius[order], position[g["edgeVertex0"]], position[g["edgeVertex1"]],
                                                     sizePixels, xc, yc, half, newOffsets, bx, by, arc, hideEdges)
        image = capi.graph_compose(sliceTop, edgeHits, rgb[gather], edgeShade)
        if fileName is not None:
            write_png(fileName, image)
        return image

    # ---- src/PythonModule.cpp:1137-1161 ----
    def createGeneGraph(self, geneGraphName=_REQUIRED, geneSetName="AllGenes", similarGenePairsName=_REQUIRED, k=_REQUIRED,
                        similarityThreshold=_REQUIRED):
        """ExpressionMatrix::createGeneGraph (src/ExpressionMatrixGeneGraph.cpp:44-89): a vertex per gene of the gene set, an
        edge to each of the first k stored similar genes at or above similarityThreshold that are in the gene set too (k <= 0:
        no limit), the vertices without an edge removed (em2_gene_graph_create, on the GPU).  Prints the reference's message.
        The graph lives in memory, like the reference's; nothing is laid out or drawn."""
        if _REQUIRED in (geneGraphName, similarGenePairsName, k, similarityThreshold):
            raise TypeError("createGeneGraph(): geneGraphName, similarGenePairsName, k and similarityThreshold are required")
        _b(geneGraphName)
        if isinstance(k, float) or not -2 ** 31 <= int(k) < 2 ** 31:                       # int (:48)
            raise ValueError("createGeneGraph(): k must be an integer that fits an int")
        if geneGraphName in self._signatureGraphs:                                         # sic: the signature graphs (:63)
            raise RuntimeError("Signature graph " + geneGraphName + " already exists.")
        handle = ctypes.c_void_p(None)
        capi.check(capi.load().em2_matrix_create_gene_graph(self._handle, _b(geneSetName), _b(similarGenePairsName), int(k),
                                                            similarityThreshold, ctypes.byref(handle)))
        graph = capi.gene_graph_take(handle)
        graph["geneSet"] = np.array(self.getGeneSetGenes(geneSetName), dtype=np.uint32)
        print("The gene graph has %d vertices and %d edges\nafter %d vertices were removed. " % (
            len(graph["vertices"]), len(graph["edgeGene0"]), graph["removedCount"]))       # src/GeneGraph.cpp:101-103
        self._geneGraphs.setdefault(geneGraphName, graph)       # map::insert (:88): under an existing name the FIRST graph stays

    def removeGeneGraph(self, geneGraphName):
        self._gene_graph(geneGraphName)
        del self._geneGraphs[geneGraphName]

    def _gene_graph(self, geneGraphName):
        if geneGraphName not in self._geneGraphs:
            raise RuntimeError("Gene graph " + geneGraphName + " does not exists.")        # sic, :29, :97
        return self._geneGraphs[geneGraphName]

    def getGeneGraphConnectivity(self, geneGraphName):
        """ExpressionMatrix::getGeneGraphConnectivity (src/ExpressionMatrixGeneGraph.cpp:103-110): for every local gene id of
        the graph's gene set the list of (local gene id of the neighbour, similarity); empty for a gene whose vertex was
        removed.  Within a list the neighbours ascend by local id (the reference's order there is that of heap addresses)."""
        g = self._gene_graph(geneGraphName)
        offsets = g["connectivityOffsets"].tolist()
        pairs = list(zip(g["connectivityGenes"].tolist(), g["connectivitySimilarities"].tolist()))
        return [pairs[offsets[v]:offsets[v + 1]] for v in range(len(offsets) - 1)]

    # The reference shows a gene graph through getGeneGraphConnectivity and its HTTP pages only; these accessors are this package's.
    def getGeneGraphNames(self):
        return sorted(self._geneGraphs)

    def getGeneGraphVertices(self, geneGraphName):
        """The global ids of the genes that kept a vertex, ascending (uint32)."""
        g = self._gene_graph(geneGraphName)
        return g["geneSet"][g["vertices"]]

    def getGeneGraphEdges(self, geneGraphName):
        """(local gene id 0, local gene id 1, similarity) per edge, in the order the reference's add_edge created them; the ids
        are local to the graph's gene set, as in getGeneGraphConnectivity."""
        g = self._gene_graph(geneGraphName)
        return g["edgeGene0"].copy(), g["edgeGene1"].copy(), g["edgeSimilarity"].copy()

    # ---- src/PythonModule.cpp:852-865 ----
    def findSimilarPairs5(self, geneSetName="AllGenes", cellSetName="AllCells", lshName=_REQUIRED,
                          similarPairsName=_REQUIRED, k=100, similarityThreshold=0.2, lshSliceLength=_REQUIRED,
                          bucketOverflow=1000):
        for name, value in (("lshName", lshName), ("similarPairsName", similarPairsName),
                            ("lshSliceLength", lshSliceLength)):
            if value is _REQUIRED:
                raise TypeError("findSimilarPairs5(): missing required argument '%s'" % name)
        dist, world = _distributed()
        if dist is not None:
            from . import sharded
            return sharded.find_similar_pairs5_collective(self, geneSetName, cellSetName, lshName, similarPairsName,
                                                          k, similarityThreshold, lshSliceLength, bucketOverflow,
                                                          dist)
        capi.check(capi.load().em2_matrix_find_similar_pairs5(self._handle, _b(geneSetName), _b(cellSetName),
                                                              _b(lshName), _b(similarPairsName), k,
                                                              similarityThreshold, lshSliceLength, bucketOverflow))

    # ---- src/PythonModule.cpp:866-880 ("Prototype code, see the code for details. Use findSimilarPairs4 instead.") ----
    def findSimilarPairs6(self, geneSetName="AllGenes", cellSetName="AllCells", lshName=_REQUIRED,
                          similarPairsName=_REQUIRED, k=100, similarityThreshold=0.2, permutationCount=_REQUIRED,
                          searchCount=_REQUIRED, permutedBitCount=64, seed=231):
        if _REQUIRED in (lshName, similarPairsName, permutationCount, searchCount):
            raise TypeError("findSimilarPairs6(): lshName, similarPairsName, permutationCount and searchCount are required")
        capi.check(capi.load().em2_matrix_find_similar_pairs6(self._handle, _b(geneSetName), _b(cellSetName), _b(lshName),
                                                              _b(similarPairsName), k, similarityThreshold, permutationCount,
                                                              searchCount, permutedBitCount, seed))

    # ---- src/PythonModule.cpp:882-897 ("Prototype code. Use findSimilarPairs4 instead.") ----
    def findSimilarPairs7(self, geneSetName="AllGenes", cellSetName="AllCells", lshName=_REQUIRED,
                          similarPairsName=_REQUIRED, k=100, similarityThreshold=0.2, lshSliceLengths=_REQUIRED,
                          maxCheck=_REQUIRED, log2BucketCount=_REQUIRED):
        if _REQUIRED in (lshName, similarPairsName, lshSliceLengths, maxCheck, log2BucketCount):
            raise TypeError("findSimilarPairs7(): lshName, similarPairsName, lshSliceLengths, maxCheck and "
                            "log2BucketCount are required")
        lengths = np.ascontiguousarray([int(x) for x in lshSliceLengths], dtype=np.int32)
        capi.check(capi.load().em2_matrix_find_similar_pairs7(self._handle, _b(geneSetName), _b(cellSetName), _b(lshName),
                                                              _b(similarPairsName), k, similarityThreshold,
                                                              capi._ptr(lengths), len(lengths), maxCheck, log2BucketCount))

    # ---- src/PythonModule.cpp:926-934 ----
    def removeSimilarPairs(self, similarPairsName):
        capi.check(capi.load().em2_matrix_remove_similar_pairs(self._handle, _b(similarPairsName)))

    # ---- src/PythonModule.cpp:616-750: cell sets (createCellSetUsingMetaData is below, with the meta data) ----
    def createCellSet(self, cellSetName, cellIds):
        """ExpressionMatrix::createCellSet (src/ExpressionMatrix.cpp:1626-1633): the cells with these global ids, sorted and
        deduplicated, as CellSet-<cellSetName>, usable by name at once.  "Cell set X already exists."; an id not below the
        cell count is refused (the reference stores it)."""
        ids = [int(i) for i in cellIds]
        if any(not 0 <= i <= 0xffffffff for i in ids):                   # CellId (src/Ids.hpp) is unsigned, 32 bits
            raise ValueError("createCellSet(): cell ids must be in [0, 2**32)")
        ids = np.ascontiguousarray(ids, dtype=np.uint32)
        capi.check(capi.load().em2_matrix_create_cell_set(self._handle, _b(cellSetName), capi._ptr(ids), len(ids)))

    def createCellSetIntersection(self, inputSetsNames, outputSetName):
        """ExpressionMatrix::createCellSetIntersection (src/ExpressionMatrix.cpp:1642-1696): inputSetsNames is a comma-separated
        list of cell set names.  Returns None and raises RuntimeError where the output exists or an input is missing (the
        reference throws, whatever its docstring says)."""
        capi.check(capi.load().em2_matrix_create_cell_set_intersection(self._handle, _b(inputSetsNames), _b(outputSetName)))

    def createCellSetUnion(self, inputSetsNames, outputSetName):
        """ExpressionMatrix::createCellSetUnion (src/ExpressionMatrix.cpp:1646-1696), as createCellSetIntersection."""
        capi.check(capi.load().em2_matrix_create_cell_set_union(self._handle, _b(inputSetsNames), _b(outputSetName)))

    def createCellSetDifference(self, inputSetName0, inputSetName1, outputSetName):
        """ExpressionMatrix::createCellSetDifference (src/ExpressionMatrix.cpp:1700-1737): the cells of inputSetName0 that are
        not in inputSetName1."""
        capi.check(capi.load().em2_matrix_create_cell_set_difference(self._handle, _b(inputSetName0), _b(inputSetName1),
                                                                     _b(outputSetName)))

    def downsampleCellSet(self, inputCellSetName="AllCells", newCellSetName=_REQUIRED, probability=_REQUIRED, seed=_REQUIRED):
        """ExpressionMatrix::downsampleCellSet (src/ExpressionMatrix.cpp:1742-1777): every cell of the input set is kept with
        the given probability, one draw of mt19937(seed) per cell in set order.  seed is the reference's int: it wraps to 32
        bits.  A new set's name that exists is refused (the reference overwrites the file)."""
        if _REQUIRED in (newCellSetName, probability, seed):
            raise TypeError("downsampleCellSet(): newCellSetName, probability and seed are required")
        if isinstance(seed, float):
            raise TypeError("downsampleCellSet(): seed must be an integer")
        wrapped = int(seed) & 0xffffffff
        wrapped -= (wrapped & 0x80000000) << 1
        capi.check(capi.load().em2_matrix_downsample_cell_set(self._handle, _b(inputCellSetName), _b(newCellSetName),
                                                              float(probability), wrapped))

    def getCellSetNames(self):
        """The names of the cell sets, in std::map order (src/ExpressionMatrix.cpp, getCellSetNames)."""
        lib = capi.load()
        size = ctypes.c_uint64(0)
        capi.check(lib.em2_matrix_cell_set_names(self._handle, ctypes.byref(size), None))
        buffer = ctypes.create_string_buffer(max(int(size.value), 1))
        capi.check(lib.em2_matrix_cell_set_names(self._handle, ctypes.byref(size), buffer))
        return [name.decode("utf-8") for name in buffer.raw[:size.value].split(b"\0")[:-1]]

    def getCellSet(self, cellSetName):
        """The global cell ids of a cell set, ascending; an empty list for a name that does not exist
        (src/ExpressionMatrixHttpServerCells.cpp:865-875)."""
        if cellSetName not in self.getCellSetNames():
            return []
        return self._cell_set(cellSetName).tolist()

    def removeCellSet(self, cellSetName):
        """ExpressionMatrix::removeCellSet (src/CellSets.cpp:88-97): "Cell set X does not exist."; the file goes.  AllCells
        cannot be removed (this package's guard)."""
        capi.check(capi.load().em2_matrix_remove_cell_set(self._handle, _b(cellSetName)))

    # ---- src/PythonModule.cpp:328-400, 622-644, 1122: cell meta data ----
    def setCellMetaData(self, cellId, name, value):
        """ExpressionMatrix::setCellMetaData (src/ExpressionMatrix.cpp:942-967): the value of the cell's field `name`, replaced
        where the cell has one.  The reference binds no Python name for it (its users write meta data through ingest); here it
        is the way in.  The store lives in memory until close() or flush() write it to the CellMetaData* files."""
        capi.check(capi.load().em2_matrix_set_cell_meta_data(self._handle, int(cellId), _b(name), _b(value)))

    def _bytes_of(self, entry, *arguments):
        size = ctypes.c_uint64(0)
        capi.check(entry(self._handle, *arguments, ctypes.byref(size), None))
        buffer = ctypes.create_string_buffer(max(int(size.value), 1))
        capi.check(entry(self._handle, *arguments, ctypes.byref(size), buffer))
        return buffer.raw[:size.value]

    def getCellMetaDataValue(self, cellId, metaDataName):
        """getCellMetaData(cellId, name) (src/ExpressionMatrix.cpp:880-907): "" for an unknown name or a cell without it."""
        raw = self._bytes_of(capi.load().em2_matrix_get_cell_meta_data_value, int(cellId), _b(metaDataName))
        return raw.decode("utf-8", "surrogateescape")

    def getCellMetaData(self, cellId):
        """[(name, value)] of a cell, in list order (src/ExpressionMatrix.cpp:913-922)."""
        raw = self._bytes_of(capi.load().em2_matrix_get_cell_meta_data, int(cellId))
        parts = [p.decode("utf-8", "surrogateescape") for p in raw.split(b"\0")[:-1]]
        return list(zip(parts[0::2], parts[1::2]))

    def getCellsMetaData(self, cellIds):
        """getCellMetaData for every cell of cellIds, in their order (src/ExpressionMatrix.cpp:928-937)."""
        return [self.getCellMetaData(cellId) for cellId in cellIds]

    def removeCellMetaData(self, cellSetName, metaDataName):
        """ExpressionMatrix::removeCellMetaData (src/ExpressionMatrix.cpp:998-1029): the field goes from every cell of the
        cell set; a name no cell ever had does nothing.  "Cell set X not found." """
        capi.check(capi.load().em2_matrix_remove_cell_meta_data(self._handle, _b(cellSetName), _b(metaDataName)))

    def createCellSetUsingMetaData(self, cellSetName, metaDataFieldName, matchString, useRegex):
        """ExpressionMatrix::createCellSetUsingMetaData (src/ExpressionMatrix.cpp:1560-1622): the cells, of ALL cells, whose
        field equals matchString or, with useRegex, matches it as a whole (std::regex, default flags)."""
        capi.check(capi.load().em2_matrix_create_cell_set_using_meta_data(self._handle, _b(cellSetName), _b(metaDataFieldName),
                                                                          _b(matchString), 1 if useRegex else 0))

    def createMetaDataFromClusterGraph(self, clusterGraphName, metaDataName):
        """ExpressionMatrix::createMetaDataFromClusterGraph (src/ExpressionMatrix.cpp:2308-2333): the cluster id of every
        clustered cell as the field metaDataName, cluster by cluster in the graph's vertex order, then "Unclustered-<cellId>"
        for every unclustered cell in unclusteredCells order (the order decides the value ids in the files)."""
        c = self._cluster_graph(clusterGraphName)
        _b(metaDataName)
        r = c["result"]
        for at, clusterId in enumerate(r["clusterIds"].tolist()):
            value = str(clusterId)
            for cellId in c["vertexCellIds"][r["cells"][int(r["cellOffsets"][at]):int(r["cellOffsets"][at + 1])]].tolist():
                self.setCellMetaData(cellId, metaDataName, value)
        for cellId in self._cluster_graph_unclustered_cells(clusterGraphName):
            self.setCellMetaData(cellId, metaDataName, "Unclustered-" + str(cellId))

    def computeMetaDataRandIndex(self, cellSetName="AllCells", metaDataName0=_REQUIRED, metaDataName1=_REQUIRED):
        """ExpressionMatrix::computeMetaDataRandIndex (src/ExpressionMatrix.cpp:1328-1390) -> (randIndex, adjustedRandIndex)
        of two fields over a cell set, the reference's doubles bit for bit.  The contingency table is counted on the GPU
        (em2_contingency_create) from one integer per cell and field; the strings are not touched."""
        if metaDataName0 is _REQUIRED or metaDataName1 is _REQUIRED:
            raise TypeError("computeMetaDataRandIndex(): metaDataName0 and metaDataName1 are required")
        ri, ari = ctypes.c_double(0.), ctypes.c_double(0.)
        capi.check(capi.load().em2_matrix_compute_meta_data_rand_index(self._handle, _b(cellSetName), _b(metaDataName0),
                                                                       _b(metaDataName1), ctypes.byref(ri), ctypes.byref(ari)))
        return ri.value, ari.value

    # The reference shows these two through its HTTP pages only (metaDataHistogram, metaDataContingencyTable): no public name.
    def _meta_data_histogram(self, cellSetName, metaDataName):
        """histogramMetaData (src/ExpressionMatrix.cpp:1301-1323): [(value, count)], count descending, then value ascending."""
        handle = ctypes.c_void_p(None)
        capi.check(capi.load().em2_matrix_meta_data_table(self._handle, _b(cellSetName), _b(metaDataName), None, ctypes.byref(handle)))
        t = capi.meta_data_table_take(handle)
        return list(zip(t["values0"], t["counts0"]))

    def _meta_data_contingency_table(self, cellSetName, metaDataName0, metaDataName1):
        """(triples, histogram0, histogram1, path): the cells of the contingency table (src/ExpressionMatrix.cpp:1369-1381)
        that are not zero as (row, column, count), rows and columns numbered in the two histograms' order, ascending by (row,
        column); path is the one em2_contingency_create took (capi.CONTINGENCY_LDS or capi.CONTINGENCY_SORT)."""
        handle = ctypes.c_void_p(None)
        capi.check(capi.load().em2_matrix_meta_data_table(self._handle, _b(cellSetName), _b(metaDataName0), _b(metaDataName1),
                                                          ctypes.byref(handle)))
        t = capi.meta_data_table_take(handle)
        return t["triples"], list(zip(t["values0"], t["counts0"])), list(zip(t["values1"], t["counts1"])), t["path"]

    def flush(self):
        """Writes the meta data store to its files (close() does it too)."""
        capi.check(capi.load().em2_matrix_flush(self._handle))

    # ---- src/PythonModule.cpp:404-478: the stored counts of cells (global ids) ----
    def _gene_id(self, geneId):
        """A gene id, or a gene name where the directory has the GeneNames table (a store that create() made): "Gene X does
        not exist." (src/ExpressionMatrix.cpp:1051-1061, :1096-1106)."""
        if isinstance(geneId, str):
            found = ctypes.c_uint32(0)
            if capi.load().em2_matrix_gene_id_from_name(self._handle, _b(geneId), ctypes.byref(found)) != capi.EM2_OK:
                raise TypeError("gene names are not offered: this directory has no GeneNames table; pass a gene id")
            if found.value == INVALID_ID:
                raise RuntimeError("Gene " + geneId + " does not exist.")
            return found.value
        return int(geneId)

    def _cell_counts(self, cellId):
        lib = capi.load()
        count = ctypes.c_uint64(0)
        capi.check(lib.em2_matrix_cell_expression_counts(self._handle, int(cellId), ctypes.byref(count), None))
        entries = np.zeros(count.value, dtype=capi.COUNT_DTYPE)
        capi.check(lib.em2_matrix_cell_expression_counts(self._handle, int(cellId), ctypes.byref(count), capi._ptr(entries)))
        return entries

    def getCellExpressionCounts(self, cellId):
        """[(geneId, count)] of a cell, every stored entry (a stored zero too), ascending by gene id
        (src/ExpressionMatrix.cpp:1066-1075).  A cell id out of range raises RuntimeError (the reference reads out of bounds)."""
        entries = self._cell_counts(cellId)
        return list(zip(entries["gene"].tolist(), entries["count"].tolist()))

    def getCellsExpressionCounts(self, cellIds):
        """getCellExpressionCounts for every cell of cellIds, in their order (src/ExpressionMatrix.cpp:1113-1122)."""
        return [self.getCellExpressionCounts(cellId) for cellId in cellIds]

    def getCellExpressionCount(self, cellId, geneId):
        """The count of a gene in a cell, 0.0 where nothing is stored: a binary search of the cell's entries
        (src/ExpressionMatrix.cpp:1035-1046)."""
        geneId = self._gene_id(geneId)
        entries = self._cell_counts(cellId)
        at = int(np.searchsorted(entries["gene"], geneId))
        if at == len(entries) or int(entries["gene"][at]) != geneId:
            return 0.0
        return float(entries["count"][at])

    def getCellsExpressionCount(self, cellIds, geneId):
        """getCellExpressionCount for every cell of cellIds, in their order (src/ExpressionMatrix.cpp:1083-1091)."""
        geneId = self._gene_id(geneId)
        return [self.getCellExpressionCount(cellId, geneId) for cellId in cellIds]

    def getCellsExpressionCountsForGenes(self, cellIds, geneIds):
        """For every cell of cellIds, in their order, its stored (global gene id, count) entries whose gene is in geneIds
        (src/ExpressionMatrix.cpp:1132-1168)."""
        wanted = np.unique(np.asarray([self._gene_id(g) for g in geneIds], dtype=np.int64))
        result = []
        for cellId in cellIds:
            entries = self._cell_counts(cellId)
            entries = entries[np.isin(entries["gene"], wanted)]
            result.append(list(zip(entries["gene"].tolist(), entries["count"].tolist())))
        return result

    # ---- src/PythonModule.cpp:479-496 ----
    def getDenseExpressionMatrix(self, geneSetName="AllGenes", cellSetName="AllCells", normalizationMethod=NormalizationMethod.none,
                                 dtype=np.float64):
        """ExpressionMatrix::getDenseExpressionMatrix (src/PythonModule.cpp:78-154): ndarray [cells of the cell set][genes of
        the gene set], indexed by the ids local to the sets; every stored count times the cell's factor (none: 1, L1:
        1 / sum, L2: 1 / sqrt(sum of squares), over the cell's entries within the gene set), zero elsewhere.  There is no guard
        against a zero sum, as in the reference: such a cell's stored entries are NaN or inf.

        dtype is np.float64 (the reference's) or np.float32, which holds the same values: every element is a float before
        the reference widens it.  The matrix is filled on the GPU (em2_matrix_dense_expression) in chunks of rows, so that
        the device buffer holds at most DENSE_CHUNK_BYTES bytes (a module attribute, 1 GiB) or one row, whichever is
        larger, whatever the size of the result."""
        method = NormalizationMethod(normalizationMethod) if normalizationMethod in (0, 1, 2) else None
        element_type = capi.dense_element_type(dtype)
        lib = capi.load()
        gene, cell = _b(geneSetName), _b(cellSetName)
        # the reference's checks, in its order, before anything is sized (an unknown method is its "Invalid normalization method.")
        capi.check(lib.em2_matrix_dense_expression(self._handle, gene, cell, int(method) if method is not None else -1, element_type,
                                                   0, 0, None))
        gene_count = ctypes.c_uint32(0)
        capi.check(lib.em2_matrix_gene_set(self._handle, gene, ctypes.byref(gene_count), None))
        cell_count = len(self._cell_set(cellSetName))
        out = np.empty((cell_count, gene_count.value), dtype=dtype)
        row_bytes = gene_count.value * out.itemsize
        chunk_rows = max(1, int(DENSE_CHUNK_BYTES) // row_bytes)
        for row_begin in range(0, cell_count, chunk_rows):
            row_end = min(cell_count, row_begin + chunk_rows)
            capi.check(lib.em2_matrix_dense_expression(self._handle, gene, cell, int(method), element_type, row_begin, row_end,
                                                       capi._ptr(out[row_begin:row_end])))
        return out

    def _cell_set(self, cellSetName):
        lib = capi.load()
        count = ctypes.c_uint32(0)
        capi.check(lib.em2_matrix_cell_set(self._handle, _b(cellSetName), ctypes.byref(count), None))
        ids = np.zeros(count.value, dtype=np.uint32)
        capi.check(lib.em2_matrix_cell_set(self._handle, _b(cellSetName), ctypes.byref(count), capi._ptr(ids)))
        return ids

    # ---- src/PythonModule.cpp:1007-1034: the consumer of SimilarPairs ----
    def getCellGraphNames(self):
        return sorted(self._cellGraphs)          # std::map order (src/ExpressionMatrix.cpp:1782-1789)

    def createCellGraph(self, graphName=_REQUIRED, cellSetName="AllCells", similarPairsName=_REQUIRED,
                        similarityThreshold=0.5, k=20, keepIsolatedVertices=False):
        """ExpressionMatrix::createCellGraph (src/ExpressionMatrix.cpp:1795-1845).  The graph lives in memory, like
        the reference's; its edges are built on the GPU (em2_cell_graph_edges) in the reference's insertion order."""
        if graphName is _REQUIRED or similarPairsName is _REQUIRED:
            raise TypeError("createCellGraph(): graphName and similarPairsName are required")
        _b(graphName)
        if graphName in self._cellGraphs:
            raise RuntimeError("Graph " + graphName + " already exists.")
        try:
            graphCells = self._cell_set(cellSetName)
        except RuntimeError:
            raise RuntimeError("Cell set " + cellSetName + " does not exists.") from None   # sic, :1813
        _, _, _, similarPairsCellSetName = files.similar_pairs_info(self.directoryName, similarPairsName)
        storedK, pairs, used = files.read_similar_pairs(self.directoryName, similarPairsName)
        similarPairsCells = self._cell_set(similarPairsCellSetName)
        v0, v1, similarity = capi.cell_graph_edges(pairs, used, similarPairsCells, graphCells, similarityThreshold, k)
        vertices = graphCells
        edgeVertices = (v0, v1)
        isolatedRemoved = 0
        if not keepIsolatedVertices:                # CellGraph::removeIsolatedVertices (src/CellGraph.cpp:189-205)
            connected = np.zeros(len(graphCells), dtype=bool)
            connected[v0] = True
            connected[v1] = True
            isolatedRemoved = int(len(graphCells) - connected.sum())
            vertices = graphCells[connected]
            position = np.cumsum(connected, dtype=np.int64) - 1     # vertex index once the isolated ones are gone
            edgeVertices = (position[v0].astype(np.uint32), position[v1].astype(np.uint32))
        self._cellGraphs[graphName] = {
            "cellSetName": cellSetName, "similarPairsName": similarPairsName,
            "similarityThreshold": similarityThreshold, "maxConnectivity": k,
            "vertexCount": int(len(vertices)), "edgeCount": int(len(v0)),
            "isolatedRemovedVertexCount": isolatedRemoved,
            "vertexCellIds": vertices, "edgeCellIds": (graphCells[v0], graphCells[v1]), "edgeSimilarity": similarity,
            "edgeVertices": edgeVertices,
        }

    def _cell_graph(self, graphName):
        if graphName not in self._cellGraphs:
            raise RuntimeError("Graph " + graphName + " does not exist.")
        return self._cellGraphs[graphName]

    def getCellGraphEdges(self, graphName):
        """[(cellId0, cellId1)] per edge, in edge-list order (src/ExpressionMatrix.cpp:1892-1913)."""
        c0, c1 = self._cell_graph(graphName)["edgeCellIds"]
        return list(zip(c0.tolist(), c1.tolist()))

    def computeCellGraphLayout(self, graphName, seed=231, maxIterationCount=300, tolerance=0.01, gravity=0.02, repulsion="exact",
                               levels="single"):
        """ExpressionMatrix::computeCellGraphLayout (src/ExpressionMatrix.cpp:1850-1864).  The reference runs Graphviz's sfdp
        on the graph; here the model sfdp minimises is iterated on the GPU at a single level (em2_graph_layout, DESIGN.md
        3.19), in units of the natural edge length.  The keyword arguments are this project's (the reference has none).
        repulsion: "exact", the N-body sum over all vertices, or "pyramid", which approximates it beyond a vertex's
        neighbourhood (em2_graph_layout_pyramid at the automatic depth): the choice for large graphs.
        levels: "single", or "multi": the graph is coarsened by matching, the coarsest graph laid out and the layout refined
        level by level, as sfdp does it (em2_graph_layout_multilevel) -- every level exact with
        repulsion="exact"; with "pyramid" level 0 always uses the pyramid, as the single-level "pyramid" does, and a coarse
        level uses it above 4 096 vertices and the exact sum below.  So on a graph of a few thousand vertices
        levels="multi", repulsion="pyramid" approximates level 0 where the exact sum would be cheaper and better: use
        repulsion="exact" there.
        Computed once per graph, like the reference's layoutWasComputed: a second call does nothing."""
        if repulsion not in ("exact", "pyramid"):
            raise ValueError('repulsion must be "exact" or "pyramid", not %r' % (repulsion,))
        if levels not in ("single", "multi"):
            raise ValueError('levels must be "single" or "multi", not %r' % (levels,))
        g = self._cell_graph(graphName)
        if "layout" in g:
            return
        v0, v1 = g["edgeVertices"]
        parameters = capi.LayoutParameters(seed=seed, maxIterationCount=maxIterationCount, tolerance=tolerance, gravity=gravity)
        if levels == "multi":
            depth = capi.LAYOUT_DEPTH_EXACT if repulsion == "exact" else capi.LAYOUT_DEPTH_AUTO
            x, y = capi.graph_layout_multilevel(g["vertexCount"], v0, v1, parameters, depth)[:2]
        else:
            layout = capi.graph_layout if repulsion == "exact" else capi.graph_layout_pyramid
            x, y, _, _, _ = layout(g["vertexCount"], v0, v1, parameters)
        g["layout"] = (x.astype(np.float64), y.astype(np.float64))

    def getCellGraphVertices(self, graphName):
        """[CellGraphVertexInfo] per vertex, in vertex order (src/ExpressionMatrix.cpp:1869-1888)."""
        g = self._cell_graph(graphName)
        if "layout" not in g:
            raise RuntimeError("Layout for graph " + graphName + " is not available.")
        x, y = g["layout"]
        return [CellGraphVertexInfo(cellId, (px, py)) for cellId, px, py in zip(g["vertexCellIds"].tolist(), x.tolist(), y.tolist())]

    # ---- ExpressionMatrix::exploreCellGraph (src/ExpressionMatrixHttpServerGraphs.cpp:350-1150) without its page ----
    def _laid_out_cell_graph(self, graphName):
        g = self._cell_graph(graphName)
        if "layout" not in g:
            raise RuntimeError("Layout for graph " + graphName + " is not available.")
        return g

    def computeCellGraphColors(self, graphName, coloringOption="noColoring", geneId=None, cellId=None, metaDataName=None,
                               metaDataMeaning="category", normalizationMethod=NormalizationMethod.L2, minColorValue=None,
                               maxColorValue=None, reuseColors=False):
        """The colouring of the page's request (:788-1040), stored in the graph for writeCellGraphSvg and drawCellGraph and
        returned as a dict.  The keyword names are the page's request parameters.
          coloringOption "byGeneExpression"  the value of gene geneId (an id or a name) in every vertex's cell, normalized over the
                                             gene set of the graph's SimilarPairs (em2_matrix_gene_expression_of_cells, GPU);
                         "bySimilarity"      the exact similarity of cell cellId to every vertex's cell over that gene set
                                             (em2_matrix_cell_similarities_to_cell, GPU);
                         "byMetaData"        by the field metaDataName, read as metaDataMeaning: "category" (a group per value,
                                             by frequency over the graph's vertices descending, then value descending; the
                                             twelve colours of the reference's palette, "black" from the thirteenth group
                                             on; counted on the host), "color" (the value is the colour string) or "number"
                                             (strtod of the whole value; what does not parse has no value and no colour);
                         anything else       no colouring.
        Numbers become colours on the GPU (em2_spectral_colors): red at minColorValue through yellow to green at
        maxColorValue, which default to the smallest and largest value.
        Returns values (float64 per vertex or None; capi.NO_VALUE is "no value"), groups (int per vertex), colors (a str per
        vertex, "" for none; in "category" the vertex's group colour), groupColors ({group: colour}, empty unless "category"),
        frequencyTable ([(count, value)] in group order), couldNotColor, minValue and maxValue (None unless numbers).
        Errors in the reference's words: "Gene not found.", "Invalid cell id.".  The keyword reuseColors=True raises
        NotImplementedError, as it always did: CellGraph::assignColorsToGroups is a step of its own here, reuseCellGraphColors,
        to be called after a "category" colouring."""
        g = self._laid_out_cell_graph(graphName)
        if reuseColors:
            raise NotImplementedError("reuseColors (CellGraph::assignColorsToGroups) is not built")
        lib = capi.load()
        vertices = np.ascontiguousarray(g["vertexCellIds"], dtype=np.uint32)
        n = len(vertices)
        result = {"coloringOption": coloringOption, "values": None, "groups": np.zeros(n, dtype=np.uint32), "colors": [""] * n,
                  "groupColors": {}, "frequencyTable": [], "couldNotColor": 0, "minValue": None, "maxValue": None, "rgb": None}
        values = None
        if coloringOption in ("byGeneExpression", "bySimilarity"):
            _, _, geneSetName, _ = files.similar_pairs_info(self.directoryName, g["similarPairsName"])      # :818-819
        if coloringOption == "byGeneExpression":
            try:
                gene = self._gene_id(geneId) if geneId is not None else INVALID_ID
            except (RuntimeError, ValueError):
                gene = INVALID_ID
            if not 0 <= gene < INVALID_ID:
                raise RuntimeError("Gene not found.")                                        # :790-793
            method = int(NormalizationMethod(normalizationMethod))
            column = np.zeros(n, dtype=np.float32)
            capi.check(lib.em2_matrix_gene_expression_of_cells(self._handle, _b(geneSetName), gene, method, capi._ptr(vertices), n,
                                                               capi._ptr(column)))
            values = column.astype(np.float64)                                               # vertex.value = p.second, :829
        elif coloringOption == "bySimilarity":
            if cellId is None or int(cellId) < 0 or int(cellId) >= self.cellCount():
                raise RuntimeError("Invalid cell id.")                                       # :839-842
            values = np.zeros(n, dtype=np.float64)
            capi.check(lib.em2_matrix_cell_similarities_to_cell(self._handle, _b(geneSetName), int(cellId), capi._ptr(vertices), n,
                                                                capi._ptr(values)))
        elif coloringOption == "byMetaData":
            if metaDataName is None:
                raise TypeError("computeCellGraphColors(): byMetaData needs metaDataName")
            if metaDataMeaning in ("category", "color", "number"):
                metaData = [self.getCellMetaDataValue(c, metaDataName) for c in vertices.tolist()]
            if metaDataMeaning == "category":                                                # :863-927
                raw = [m.encode("utf-8", "surrogateescape") for m in metaData]
                frequency = {}
                for m in raw:
                    frequency[m] = frequency.get(m, 0) + 1
                table = sorted(((count, m) for m, count in frequency.items()), reverse=True)  # std::greater<pair<int, string>>
                groupOf = {m: group for group, (_, m) in enumerate(table)}
                result["groups"] = np.asarray([groupOf[m] for m in raw], dtype=np.uint32)
                result["groupColors"] = {group: (CATEGORY_PALETTE[group] if group < 12 else "black") for group in range(len(table))}
                result["frequencyTable"] = [(count, m.decode("utf-8", "surrogateescape")) for count, m in table]
                result["couldNotColor"] = sum(count for count, _ in table[12:])
                result["colors"] = [result["groupColors"][group] for group in result["groups"].tolist()]
                palette = np.asarray([int(c[1:], 16) for c in CATEGORY_PALETTE] + [capi.COLOR_BLACK], dtype=np.uint32)
                result["rgb"] = palette[np.minimum(result["groups"], 12)]
            elif metaDataMeaning == "color":                                                 # :935-943
                result["colors"] = metaData
            elif metaDataMeaning == "number":                                                # :949-964
                parsed = {}
                for m in metaData:
                    if m not in parsed:
                        parsed[m] = capi.meta_data_number(m)
                values = np.asarray([parsed[m] for m in metaData], dtype=np.float64)
        if values is not None:                                                               # :1003-1040
            rgb, valueRange = capi.spectral_colors(values, minColorValue, maxColorValue)
            result.update(values=values, rgb=rgb, colors=capi.color_strings(rgb), minValue=float(valueRange[0]),
                          maxValue=float(valueRange[1]))
        g["coloring"] = result
        return {key: value for key, value in result.items() if key not in ("rgb", "coloringOption")}

    def reuseCellGraphColors(self, graphName):
        """The page's reuseColors (:900-913) on the stored "category" colouring of computeCellGraphColors:
        CellGraph::assignColorsToGroups (src/CellGraph.cpp:794-862) gives every group a colour index such that no two groups
        joined by an edge share one (the group graph on the GPU, em2_graph_group_colors; the greedy on the host), and a group
        is painted with the palette entry of that index where it is below 12, else "black".  Rewrites the stored groupColors,
        colors and rgb, so that writeCellGraphSvg and drawCellGraph draw the new colours (the painter order stays by group),
        and returns the dict of computeCellGraphColors plus colorTable (uint32 per group).  couldNotColor becomes the number of
        vertices that are still black.  RuntimeError where the stored colouring is not the "category" one."""
        g = self._laid_out_cell_graph(graphName)
        result = g.get("coloring")
        if not result or result["coloringOption"] != "byMetaData" or not result["frequencyTable"]:
            raise RuntimeError("reuseCellGraphColors(): the colouring stored for graph " + graphName + " is not a \"category\" "
                               "colouring (computeCellGraphColors with coloringOption=\"byMetaData\", metaDataMeaning=\"category\").")
        v0, v1 = g["edgeVertices"]
        table = capi.graph_group_colors(result["groups"], v0, v1)["colorTable"]
        groupCount = len(result["frequencyTable"])
        assert len(table) == groupCount or g["vertexCount"] == 0
        colorOf = np.minimum(table, 12)
        result["groupColors"] = {group: (CATEGORY_PALETTE[int(colorOf[group])] if colorOf[group] < 12 else "black")
                                 for group in range(len(table))}
        result["colors"] = [result["groupColors"][group] for group in result["groups"].tolist()]
        palette = np.asarray([int(c[1:], 16) for c in CATEGORY_PALETTE] + [capi.COLOR_BLACK], dtype=np.uint32)
        result["rgb"] = palette[colorOf[result["groups"]]] if len(table) else np.zeros(0, dtype=np.uint32)
        result["couldNotColor"] = int((colorOf[result["groups"]] == 12).sum()) if len(table) else 0
        result["colorTable"] = table
        return {key: value for key, value in result.items() if key not in ("rgb", "coloringOption")}

    def compareCellGraphs(self, graphName0, graphName1):
        """ExpressionMatrix::compareCellGraphs (src/ExpressionMatrixHttpServerGraphs.cpp:104-345) without its HTML, on the GPU
        (em2_cell_graph_compare).  Returns a dict: "graphs", per graph the stored creation parameters and counts
        the page prints (cellSetName, similarPairsName, similarityThreshold, maxConnectivity, vertexCount,
        isolatedRemovedVertexCount, and edgeCount: the distinct unordered cell pairs, the size of the reference's edge map);
        commonVertexCount, commonEdgeCount, commonIdenticalEdgeCount; histogramDelta (float32) and histogramCount (uint64), the
        distribution of similarity1 - similarity0 over the common edges in bins of 0.01, ascending.
        RuntimeError in the page's words where a graph is missing or both names are the same."""
        if graphName0 not in self._cellGraphs or graphName1 not in self._cellGraphs:
            raise RuntimeError("Did not find one or both of the cell graphs to be compared.")            # :117-118
        if graphName0 == graphName1:
            raise RuntimeError("Comparison of a cell graph with itself requested. ")                     # :122-123
        stored = [self._cellGraphs[graphName0], self._cellGraphs[graphName1]]
        c = capi.cell_graph_compare(*[(g["vertexCellIds"], g["edgeVertices"][0], g["edgeVertices"][1], g["edgeSimilarity"])
                                      for g in stored])
        graphs = []
        for g, edgeCount in zip(stored, (c["edgeCount0"], c["edgeCount1"])):
            information = {key: g[key] for key in ("cellSetName", "similarPairsName", "similarityThreshold", "maxConnectivity",
                                                   "vertexCount", "isolatedRemovedVertexCount")}
            information["edgeCount"] = edgeCount
            graphs.append(information)
        return {"graphs": graphs, "commonVertexCount": c["commonVertexCount"], "commonEdgeCount": c["commonEdgeCount"],
                "commonIdenticalEdgeCount": c["commonIdenticalEdgeCount"], "histogramDelta": c["binDelta"],
                "histogramCount": c["binCount"]}

    def _cell_graph_view(self, g, sizePixels, xViewBoxCenter, yViewBoxCenter, viewBoxHalfSize, vertexRadius, edgeThickness):
        """The page's defaults (:411-438): the coordinate range enlarged to a square and by 5 %, a radius of 1.5 pixels and
        a thickness of 0.05 pixel.  CellGraph::computeCoordinateRange (src/CellGraph.cpp:270-290) is reproduced as written:
        its maxima start at numeric_limits<double>::min(), the smallest positive normal double, not at lowest(), so a layout
        entirely at negative x has xMax = 2.2e-308, not its largest x."""
        x, y = g["layout"]
        largest, tiny = float(np.finfo(np.float64).max), float(np.finfo(np.float64).tiny)
        xMin, xMax = min([largest] + ([float(x.min())] if len(x) else [])), max([tiny] + ([float(x.max())] if len(x) else []))
        yMin, yMax = min([largest] + ([float(y.min())] if len(y) else [])), max([tiny] + ([float(y.max())] if len(y) else []))
        deltaX, deltaY = xMax - xMin, yMax - yMin
        if deltaX <= deltaY:
            delta = deltaY
            xMax = xMin + delta
        else:
            delta = deltaX
            yMax = yMin + delta
        delta *= 1.05
        sizePixels = float(sizePixels)
        return (float((xMin + xMax) / 2.) if xViewBoxCenter is None else float(xViewBoxCenter),
                float((yMin + yMax) / 2.) if yViewBoxCenter is None else float(yViewBoxCenter),
                float(delta / 2.) if viewBoxHalfSize is None else float(viewBoxHalfSize),
                float(1.5 * delta / sizePixels) if vertexRadius is None else float(vertexRadius),
                float(0.05 * delta / sizePixels) if edgeThickness is None else float(edgeThickness))

    def writeCellGraphSvg(self, graphName, fileName, hideEdges=False, svgSizePixels=600, xViewBoxCenter=None, yViewBoxCenter=None,
                          viewBoxHalfSize=None, vertexRadius=None, edgeThickness=None):
        """CellGraph::writeSvg (src/CellGraph.cpp:301-439) into fileName, byte for byte what the page embeds for the same
        request, with the colouring computeCellGraphColors stored last (none before it was called).  The view's defaults
        are the page's: see _cell_graph_view, which also states a quirk of the reference that is kept.  Written by the host
        (em2_graph_write_svg); at a million vertices it is hundreds of MB of text: use drawCellGraph there."""
        g = self._laid_out_cell_graph(graphName)
        xc, yc, half, radius, thickness = self._cell_graph_view(g, svgSizePixels, xViewBoxCenter, yViewBoxCenter, viewBoxHalfSize,
                                                                vertexRadius, edgeThickness)
        coloring = g.get("coloring")
        _, _, geneSetName, _ = files.similar_pairs_info(self.directoryName, g["similarPairsName"])
        x, y = g["layout"]
        v0, v1 = g["edgeVertices"]
        capi.graph_write_svg(fileName, x, y, g["vertexCellIds"], v0, v1, hideEdges, svgSizePixels, xc, yc, half, radius, thickness,
                             geneSetName, vertex_colors=coloring["colors"] if coloring else None,
                             vertex_groups=coloring["groups"] if coloring else None,
                             group_colors=coloring["groupColors"] if coloring else None)

    def drawCellGraph(self, graphName, fileName=None, sizePixels=1024, edgeShade=255, hideEdges=False, xViewBoxCenter=None,
                      yViewBoxCenter=None, viewBoxHalfSize=None, vertexRadius=None):
        """The picture of writeCellGraphSvg as an image, rastered on the GPU (em2_graph_draw, em2_graph_compose; the
        definition is in include/em2_lsh.h): uint8 [sizePixels, sizePixels, 4], rows from the top, r g b a.  The same view
        parameters and defaults, sizePixels in the place of svgSizePixels.  No anti-aliasing; the edges are one-pixel lines
        whatever the thickness (the reference's default is a hairline of 0.05 pixel), black at edgeShade=255, and with a
        smaller edgeShade a pixel darkens with the number of edges through it.  A vertex without a colour is black, as in the
        SVG.  With groups the vertices are painted in the SVG's order: group ascending, then vertex order.
        A "color" value that is not #rrggbb raises ValueError naming it: colour names are not parsed (the SVG passes them on).
        With fileName the image is also written as a PNG (zlib and struct only, filter 0)."""
        g = self._laid_out_cell_graph(graphName)
        xc, yc, half, radius, _ = self._cell_graph_view(g, sizePixels, xViewBoxCenter, yViewBoxCenter, viewBoxHalfSize, vertexRadius, None)
        x, y = g["layout"]
        v0, v1 = g["edgeVertices"]
        coloring = g.get("coloring")
        rgb = None
        if coloring:
            rgb = coloring["rgb"]
            if rgb is None:
                rgb = np.asarray([_rgb_of(c) for c in coloring["colors"]], dtype=np.uint32)
            if coloring["groupColors"]:
                order = np.argsort(coloring["groups"], kind="stable")                # the SVG's painter order
                position = np.empty(len(order), dtype=np.uint32)
                position[order] = np.arange(len(order), dtype=np.uint32)
                x, y, rgb = x[order], y[order], rgb[order]
                v0, v1 = position[v0], position[v1]
        vertexTop, edgeHits = capi.graph_draw(x, y, v0, v1, sizePixels, xc, yc, half, radius, hideEdges)
        image = capi.graph_compose(vertexTop, edgeHits, rgb if rgb is not None else np.zeros(len(x), dtype=np.uint32), edgeShade)
        if fileName is not None:
            write_png(fileName, image)
        return image

    def labelPropagationClustering(self, graphName, seed=231, stableIterationCountThreshold=3, maxIterationCount=100):
        """CellGraph::labelPropagationClustering (src/CellGraph.cpp:443-612), the first step of
        ExpressionMatrix::createClusterGraph (src/ExpressionMatrix.cpp:2145-2149; defaults from
        ClusterGraphCreationParameters, src/ClusterGraph.hpp:48-50).  The reference keeps the result in the
        clusterId of every graph vertex; here it is returned: (cellIds, clusterIds), one entry per vertex, clusters
        numbered from 0 by decreasing size.  createClusterGraph runs this and the rest (ClusterGraph)."""
        g = self._cell_graph(graphName)
        v0, v1 = g["edgeVertices"]
        clusters, iterations = capi.cell_graph_label_propagation(g["vertexCellIds"], v0, v1, g["edgeSimilarity"], seed,
                                                                 stableIterationCountThreshold, maxIterationCount)
        g["clusterIds"] = clusters
        g["labelPropagationIterations"] = iterations
        return g["vertexCellIds"].copy(), clusters

    # ---- src/PythonModule.cpp:1064-1119 ----
    def createClusterGraph(self, cellGraphName=_REQUIRED, clusterGraphName=_REQUIRED, stableIterationCount=3,
                           maxIterationCount=100, seed=231, minClusterSize=100, k=3, similarityThreshold=0.5,
                           similarityThresholdForMerge=0.9):
        """ExpressionMatrix::createClusterGraph (src/ExpressionMatrix.cpp:2087-2185): label propagation on the cell graph,
        then the ClusterGraph -- merge of similar clusters, removal of small ones, average expression and similarities
        (em2_cluster_graph_create, on the GPU), weak edges, k-NN, renumbering by decreasing size.  The gene set is that of
        the cell graph's SimilarPairs object (:2129-2131).  The graph lives in memory, like the reference's."""
        if cellGraphName is _REQUIRED or clusterGraphName is _REQUIRED:
            raise TypeError("createClusterGraph(): cellGraphName and clusterGraphName are required")
        _b(clusterGraphName)
        if cellGraphName not in self._cellGraphs:
            raise RuntimeError("Cell graph " + cellGraphName + " does not exist.")
        g = self._cellGraphs[cellGraphName]
        _, _, geneSetName, _ = files.similar_pairs_info(self.directoryName, g["similarPairsName"])
        if clusterGraphName in self._clusterGraphs:
            raise RuntimeError("Cluster graph " + clusterGraphName + " already exists.")
        vertexCellIds, labels = self.labelPropagationClustering(cellGraphName, seed, stableIterationCount, maxIterationCount)
        geneCount, toc, data = self._subset(geneSetName, g["cellSetName"])
        graphCells = self._cell_set(g["cellSetName"])
        order = np.argsort(graphCells, kind="stable")
        vertexRows = order[np.searchsorted(graphCells, vertexCellIds, sorter=order)].astype(np.uint32)
        v0, v1 = g["edgeVertices"]
        result = capi.cluster_graph_create(toc, data, geneCount, vertexRows, v0, v1, labels, minClusterSize, k,
                                           similarityThreshold, similarityThresholdForMerge)
        self._clusterGraphs[clusterGraphName] = {
            "geneSetName": geneSetName, "cellSetName": g["cellSetName"], "vertexCellIds": vertexCellIds, "result": result,
            "position": {int(clusterId): i for i, clusterId in enumerate(result["clusterIds"].tolist())},
        }

    def _cluster_graph(self, clusterGraphName):
        if clusterGraphName not in self._clusterGraphs:
            raise RuntimeError("Cluster graph " + clusterGraphName + " does not exist.")
        return self._clusterGraphs[clusterGraphName]

    def _cluster(self, clusterGraphName, clusterId):
        c = self._cluster_graph(clusterGraphName)
        if clusterId not in c["position"]:
            raise RuntimeError("Cluster " + str(clusterId) + " of cluster graph " + clusterGraphName + " does not exist.")
        return c, c["position"][clusterId]

    def getClusterGraphVertices(self, clusterGraphName):
        """The cluster ids, in the order of ClusterGraph::vertexMap (src/ExpressionMatrix.cpp:2210-2227): ascending."""
        return sorted(self._cluster_graph(clusterGraphName)["position"])

    def getClusterGraphGenes(self, clusterGraphName):
        """The global ids of the genes the cluster graph was built on (src/ExpressionMatrix.cpp:2232-2244)."""
        c = self._cluster_graph(clusterGraphName)
        lib = capi.load()
        count = ctypes.c_uint32(0)
        capi.check(lib.em2_matrix_gene_set(self._handle, _b(c["geneSetName"]), ctypes.byref(count), None))
        ids = np.zeros(count.value, dtype=np.uint32)
        capi.check(lib.em2_matrix_gene_set(self._handle, _b(c["geneSetName"]), ctypes.byref(count), capi._ptr(ids)))
        return ids.tolist()

    def getClusterCells(self, clusterGraphName, clusterId):
        """The global cell ids of a cluster, in the order the reference stores them (src/ExpressionMatrix.cpp:2249-2272)."""
        c, at = self._cluster(clusterGraphName, clusterId)
        r = c["result"]
        return c["vertexCellIds"][r["cells"][int(r["cellOffsets"][at]):int(r["cellOffsets"][at + 1])]].tolist()

    def getClusterAverageExpression(self, clusterGraphName, clusterId):
        """The L2-normalized average expression of a cluster, one value per gene of getClusterGraphGenes
        (src/ExpressionMatrix.cpp:2279-2303)."""
        c, at = self._cluster(clusterGraphName, clusterId)
        return c["result"]["averages"][at].tolist()

    def _cluster_graph_edges(self, clusterGraphName):
        """[(clusterId0, clusterId1, similarity)] in the order the edges were created; the reference shows its edges
        through Graphviz only (ClusterGraph::write), hence no public name.  unclusteredCells likewise:
        _cluster_graph_unclustered_cells."""
        r = self._cluster_graph(clusterGraphName)["result"]
        return list(zip(r["edgeCluster0"].tolist(), r["edgeCluster1"].tolist(), r["edgeSimilarity"].tolist()))

    def _cluster_graph_unclustered_cells(self, clusterGraphName):
        c = self._cluster_graph(clusterGraphName)
        return c["vertexCellIds"][c["result"]["unclusteredCells"]].tolist()

    def _cell_graph_information(self, graphName):
        """The CellGraphInformation fields stored beside the graph (src/ExpressionMatrix.cpp:1824-1839); the
        reference shows them in its HTTP UI only, hence no public name here."""
        g = self._cell_graph(graphName)
        return {key: g[key] for key in ("cellSetName", "similarPairsName", "similarityThreshold", "maxConnectivity",
                                        "vertexCount", "edgeCount", "isolatedRemovedVertexCount")}

    def _subset_sizes(self, geneSetName, cellSetName):
        """(geneCount, cellCount, nnz) of the subset; raises the reference's lookup / emptiness errors."""
        genes = ctypes.c_uint32(0)
        cells = ctypes.c_uint32(0)
        nnz = ctypes.c_uint64(0)
        capi.check(capi.load().em2_matrix_subset(self._handle, _b(geneSetName), _b(cellSetName), ctypes.byref(genes),
                                                 ctypes.byref(cells), ctypes.byref(nnz), None, None))
        return int(genes.value), int(cells.value), int(nnz.value)

    # ---- helper used by the sharded driver and by tests (ExpressionMatrixSubset as arrays) ----
    def _subset(self, geneSetName, cellSetName):
        lib = capi.load()
        genes = ctypes.c_uint32(0)
        cells = ctypes.c_uint32(0)
        nnz = ctypes.c_uint64(0)
        capi.check(lib.em2_matrix_subset(self._handle, _b(geneSetName), _b(cellSetName), ctypes.byref(genes),
                                         ctypes.byref(cells), ctypes.byref(nnz), None, None))
        toc = np.zeros(cells.value + 1, dtype=np.uint64)
        data = np.zeros(nnz.value, dtype=capi.COUNT_DTYPE)
        capi.check(lib.em2_matrix_subset(self._handle, _b(geneSetName), _b(cellSetName), ctypes.byref(genes),
                                         ctypes.byref(cells), ctypes.byref(nnz), capi._ptr(toc), capi._ptr(data)))
        return int(genes.value), toc, data
