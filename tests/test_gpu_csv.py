"""addCells on the GPU: em2_dev_csv_parse against a model of its outputs (csv_binding.model_parse: getline, the quote rule,
the exactness rule that test_csv_cpu.py holds against strtof) with nothing discarded and no tolerance -- line table, token
counts, statuses, first-field ranges, the set of decided counts with their bits, the deferred fields -- and
ExpressionMatrix.addCells on the GPU path against the reference's loops replayed through addGene / addCell and against the
host path."""
import os
import random

import numpy as np
import pytest

import csv_binding as cb
import ingest_binding as ib
from expressionmatrix2_amd import ExpressionMatrix, capi, files
from test_csv_cpu import CASES, META

pytestmark = pytest.mark.gpu

NONE = cb.NONE


@pytest.fixture(scope="module")
def torch():
    import torch
    capi.load()
    return torch


@pytest.fixture()
def tile():
    """The tile size for one test; the default comes back behind it."""
    yield capi.load().em2_set_csv_tile_bytes
    capi.load().em2_set_csv_tile_bytes(0)


def kept_all(columns):
    """Every column but the first is kept."""
    return [NONE] + list(range(columns - 1))


def pattern(n):
    """n bytes of three-column lines, cut where n says."""
    return (b"ab,1,22\n" + b"c,0,3.5\n" + b"\"d,e\",7,0.\n") * (n // 8 + 1)


@pytest.mark.parametrize("tile_bytes", [16, 64, 0])
def test_text_lengths_around_a_load_and_a_tile(torch, tile, tile_bytes):
    tile(tile_bytes)
    t = tile_bytes or 16384
    for n in sorted({0, 1, 15, 16, 17, t - 1, t, t + 1, 2 * t + 5}):
        text = pattern(n)[:n]
        cb.assert_parse(torch, text, ",", 3, [NONE, 0, 1], "%d bytes" % n)
    for misalign in (1, 7, 15):                                               # an unaligned device pointer
        cb.assert_parse(torch, pattern(333)[:333], ",", 3, [NONE, 0, 1], "misaligned by %d" % misalign, misalign=misalign)


STRUCTURES = [
    ("one line longer than several tiles", b"g," + b",".join(b"%d" % (i % 13) for i in range(120)) + b"\nh,1\n", 121),
    ("many lines inside one load", b"a,1\nb,2\nc,3\nd,4\ne,5\n", 2),
    ("a field across a tile boundary", b"gene,1234567,89012345,6.25\nx,1,2,3\n", 4),
    ("a quoted run across a tile boundary", b"gene,1,\"a,b,c,d,e,f,g\",2\ny,\"3\",4,5\n", 4),
    ("a line end of two bytes across a tile boundary", b"gene,10,200,30\r\nz,1,2,3\r\n", 4),
    ("quotes that close two tiles later", b"g,\"1,2,3,4,5,6,7,8,9,10,11,12,13,14,15,16,17\",5,6\nh,1,2,3\n", 4),
    ("an open quote ends with its line", b"g,\"1,2\nh,3,4\n\"i\",5,6\n", 3),
    ("a line with an escape between ordinary lines", b"a,1,2\nb\\,c,3,4\nd,5,6\n\\\ne,7,8", 3),
    ("the last field of the last line without a line end", b"a,1,2\nb,3,4.5", 3),
    ("empty lines, a lone carriage return, wrong counts", b"a,1,2\n\n\r\nb,3\nc,4,5,6\n,,\n", 3),
    ("only line ends", b"\n\n\n", 3),
    ("blanks and empty fields", b" a , 1 ,\t2\t\n b,, \n", 3),
]


@pytest.mark.parametrize("tile_bytes", [16, 48, 0])
@pytest.mark.parametrize("case", STRUCTURES, ids=[case[0] for case in STRUCTURES])
def test_structures(torch, tile, tile_bytes, case):
    tile(tile_bytes)
    _, text, columns = case
    for shift in range(0, 16, 5):                                             # move the boundaries through the text
        shifted = b"p" + b",0" * (columns - 1) + b"\n" + b"q" * shift + text
        got = cb.assert_parse(torch, shifted, ",", columns, kept_all(columns), "%s shifted by %d" % (case[0], shift))
        if case[0].startswith("a line with an escape"):
            assert sorted(got["lines"][:, 3].tolist()).count(cb.ESCAPE) == 2


@pytest.mark.parametrize("separators", [",", ";\t", ",;|:/!# "])
def test_separator_strings(torch, tile, separators):
    tile(32)
    rng = random.Random(len(separators))
    lines = []
    for i in range(20):
        fields = ["g%d" % i] + [rng.choice(["0", "1", "2.5", "\"%s\"" % separators, "17", ""]) for _ in range(5)]
        lines.append("".join(f + rng.choice(separators) for f in fields[:-1]) + fields[-1])
    text = ("\n".join(lines) + "\n").encode()
    cb.assert_parse(torch, text, separators, 6, kept_all(6), "separators %r" % separators)
    with pytest.raises(RuntimeError, match="separator"):
        cb.device_parse(torch, b"a,b\n", ",\"", 2, [NONE, 0])
    with pytest.raises(RuntimeError, match="separator"):
        cb.device_parse(torch, b"a,b\n", "123456789", 2, [NONE, 0])


@pytest.mark.parametrize("columns", [1, 63, 64, 65, 1025])
def test_column_counts(torch, tile, columns):
    tile(64)
    rng = random.Random(columns)
    rows = [",".join(["g%d" % r] + [rng.choice(["0", "0", "0", "3", "12", "1.5"]) for _ in range(columns - 1)]) for r in range(5)]
    rows.append(",".join(["short"] + ["1"] * max(columns - 2, 0)) + ("," if columns == 1 else ""))          # a wrong count
    text = ("\n".join(rows) + "\n").encode()
    kept = [NONE] + [i if i % 3 else NONE for i in range(columns - 1)]        # a kept subset
    cb.assert_parse(torch, text, ",", columns, kept, "%d columns" % columns)


def test_numbers_first_last_and_mid_line(torch, tile):
    tile(48)
    numbers = [n for n in cb.NUMBERS if "," not in n]
    lines = []
    for n in numbers:
        lines += [n + ",1,2", "1," + n + ",2", "1,2," + n]
    text = ("\n".join(lines) + "\n").encode()
    got = cb.assert_parse(torch, text, ",", 3, [0, 1, 2], "the numbers", line_base=1000)
    bits = {(line, cell): b for cell, line, b in got["triples"]}
    at = lambda n, place: 1000 + 3 * numbers.index(n) + place
    assert bits[(at("16777216", 1), 1)] == 0x4b800000 and bits[(at("16777218", 2), 2)] == 0x4b800001
    assert (at("16777217", 0), 0) not in bits and any(d[:2] == (at("16777217", 0), 0) for d in got["deferred"])
    assert bits[(at("-0", 2), 2)] == 0x80000000 and bits[(at(" 7 ", 1), 1)] == 0x40e00000 and (at("0.", 0), 0) not in bits


def test_an_all_integer_matrix_defers_nothing(torch, tile):
    """Integers below 2^24 are always decided (at most 8 digits, q = 0, an exact float: no midpoint)."""
    tile(256)
    rng = np.random.default_rng(3)
    values = rng.integers(0, 2 ** 24, size=(40, 30))
    values[rng.random(values.shape) < .8] = 0
    text = "".join("g%d,%s\n" % (r, ",".join(str(v) for v in row)) for r, row in enumerate(values)).encode()
    got = cb.assert_parse(torch, text, ",", 31, kept_all(31), "integers")
    assert got["counts"][2] == 0 and got["deferred"] == set() and got["counts"][1] == int((values != 0).sum())


def test_random_texts(torch, tile):
    rng = random.Random(11)
    alphabet = "0123456789" * 3 + ",,,,,," + "\n\n" + "\"\r .e-+\\x"
    for seed in range(40):
        tile(rng.choice([16, 32, 80]))
        text = "".join(rng.choice(alphabet) for _ in range(rng.randint(1, 400))).encode()
        columns = rng.randint(1, 6)
        kept = [rng.choice([NONE, i]) for i in range(columns)]
        cb.assert_parse(torch, text, ",", columns, kept, "random text %d" % seed, misalign=rng.randint(0, 15))


def test_capacities_are_respected(torch, tile):
    tile(16)
    text = b"a,1,x\nb,2,y\nc,3,z\nd,4,\n"
    full = cb.assert_parse(torch, text, ",", 3, [NONE, 0, 1], "full")
    assert full["counts"] == [4, 4, 4]
    short = cb.device_parse(torch, text, ",", 3, [NONE, 0, 1], capacities=(2, 4, 4))            # the guards are checked inside
    assert short["counts"][0] == 4 and "lines" not in short
    short = cb.device_parse(torch, text, ",", 3, [NONE, 0, 1], capacities=(4, 1, 2))
    assert short["counts"] == [4, 4, 4] and len(short["triples"]) == 1 and len(short["deferred"]) == 2
    assert short["triples"] <= full["triples"] and short["deferred"] <= full["deferred"]


# ---- addCells through the facade ----

def toy(name):
    return os.path.join(cb.GOLDEN, name)


def test_toy_files_and_find_similar_pairs0(torch, tmp_path):
    import toytest1
    steps = [(toy("ToyTest1/ExpressionMatrix.csv"), ",", toy("ToyTest1/MetaData.csv"), ",", [])]
    error, directory, deferred = cb.check_add_cells(tmp_path / "toy1", steps, True)
    assert error is None and deferred == [0]
    steps = [(toy("ToyTest2/ExpressionMatrix1.csv"), ",", toy("ToyTest2/MetaData1.csv"), ",", []),
             (toy("ToyTest2/ExpressionMatrix2.csv"), ",", toy("ToyTest2/MetaData2.csv"), ",", [])]
    assert cb.check_add_cells(tmp_path / "toy2", steps, True)[0] is None
    steps = [(toy("ToyTest4/ExpressionMatrix.csv"), ",", toy("ToyTest4/MetaData.csv"), ",", [("Batch", "4")])]
    assert cb.check_add_cells(tmp_path / "toy4", steps, True)[0] is None
    # the reference's ToyTest1: findSimilarPairs0 on the loaded store equals the same matrix written from arrays
    gene_count, toc, genes, counts = toytest1.load()
    tool = str(tmp_path / "tool")
    files.create_directory(tool, gene_count, toc, capi.make_counts(genes, counts))
    results = []
    for d in (directory, tool):
        e = ExpressionMatrix(d)
        e.findSimilarPairs0(similarPairsName="Exact")
        e.close()
        results.append(files.read_similar_pairs(d, "Exact"))
    (k0, pairs0, used0), (k1, pairs1, used1) = results
    assert k0 == k1 and np.array_equal(used0, used1) and pairs0.tobytes() == pairs1.tobytes() and used0.sum() > 0


@pytest.fixture(scope="module")
def generated(tmp_path_factory):
    """300 genes x 700 cells, 90 % "0", quoted names as R's write.csv writes them; a meta data file that names a subset of the
    columns in another order, and cells the expression file does not have; a second pair of files with overlapping genes in
    another order."""
    base = tmp_path_factory.mktemp("generated")
    rng = random.Random(5)
    cells = ["\"cell.%d\"" % i for i in range(700)]
    genes = ["\"gene-%d\"" % i for i in range(300)]

    def matrix(gene_names, cell_names, path):
        lines = ["\"\"," + ",".join(cell_names)]
        for g in gene_names:
            fields = []
            for _ in cell_names:
                u = rng.random()
                fields.append("0" if u < .9 else str(rng.randint(1, 500)) if u < .97 else rng.choice(
                    ["0.5", "12.25", "1e2", " 3 ", "0.1", "16777217", "0.0", "\"8\"", "7.125", "1234.5678", "0.30000001192092896"]))
            lines.append(g + "," + ",".join(fields))
        return cb.write(base / path, "\n".join(lines) + "\n")

    def meta(cell_names, path):
        lines = ["\"\",\"tissue\",\"batch\""] + ["%s,\"t%d\",%d" % (name, rng.randint(0, 4), rng.randint(0, 9)) for name in cell_names]
        return cb.write(base / path, "\n".join(lines) + "\n")

    kept = [name for name in cells if rng.random() < .6]
    rng.shuffle(kept)
    first = (matrix(genes, cells, "e1.csv"), ",", meta(kept + ["\"elsewhere\""], "m1.csv"), ",", [("run", "1")])
    cells2 = ["\"second.%d\"" % i for i in range(40)]
    genes2 = genes[250:] + ["\"new-%d\"" % i for i in range(20)] + genes[:30]
    rng.shuffle(genes2)
    second = (matrix(genes2, cells2, "e2.csv"), ",", meta(cells2[5:], "m2.csv"), ",", [])
    return [first, second]


@pytest.mark.parametrize("chunks", ["one", "two", "many"])
def test_generated_files_in_chunks(torch, tmp_path, generated, chunks):
    size = os.path.getsize(generated[0][0])
    chunk_bytes = {"one": 1 << 30, "two": size // 2 + 2000, "many": 4096}[chunks]
    error, device_dir, deferred = cb.check_add_cells(tmp_path / "device", generated, True, chunk_bytes=chunk_bytes)
    assert error is None and deferred[0] > 0
    if chunks == "many":                                                      # and against the host path: identical stores
        error, host_dir, none = cb.check_add_cells(tmp_path / "host", generated, False)
        assert error is None and none == [0, 0]
        assert ib.read_store(device_dir) == ib.read_store(host_dir)
        store = ib.read_store(device_dir)
        assert len(store["geneNames"]) == 320 and store["cellNames"][0].startswith("cell.") and len(store["cellNames"]) > 400


@pytest.mark.parametrize("case", CASES, ids=[case[0] for case in CASES])
def test_the_cases_of_the_host_path_on_the_gpu_path(torch, tmp_path, tile, case):
    tile(32)
    _, expression, meta, expression_separators, meta_separators, additional, expected = case
    steps = [(cb.write(tmp_path / "e.csv", expression), expression_separators, cb.write(tmp_path / "m.csv", meta), meta_separators, additional)]
    error, directory, _ = cb.check_add_cells(tmp_path / "stores", steps, True, chunk_bytes=16)
    assert (error is None) if expected is None else (error is not None and expected in error)


def late(lines, bad):
    """40 ordinary lines with a decoy in the unkept column, then the failing line."""
    return "g,c0,zz,c1\n" + "".join("G%d,%d,%s,0\n" % (i, i, lines) for i in range(40)) + bad


LATE = [
    ("an invalid count", late("x", "H,1,2,y\n"), "Invalid expression count y encountered at line 42 of file"),
    ("an empty count", late("", "H,,2,3\n"), "Invalid expression count (empty) encountered at line 42 of file"),
    ("a wrong token count", late("1\\,2", "H,1,2\n"), "Unexpected number of items in line of expression counts file"),
    ("a duplicate gene", late("\"1,2\"", "G7,1,2,3\n"), "Duplicate entry for gene G7 in cell expression counts file"),
    ("an empty line", late("-1", "\nH,1,2,3\n"), "Empty line in expression counts file"),
    ("an escape in a deferred line", late("nan", "H\\q,1,2,3\n"), "unknown escape sequence"),
    ("a negative count", late("-5", "H,1,x,-3\n"), "Negative expression count encountered."),
    ("a negative count the host resolves", late("-5", "H,1,x,\"-3\"\n"), "Negative expression count encountered."),
]


@pytest.mark.parametrize("case", LATE, ids=[case[0] for case in LATE])
@pytest.mark.parametrize("chunk_bytes", [1 << 30, 64])
def test_late_errors_behind_decoys(torch, tmp_path, case, chunk_bytes):
    _, expression, expected = case
    steps = [(cb.write(tmp_path / "e.csv", "g,c0\nA,1\n"), ",", cb.write(tmp_path / "m0.csv", "Cell,Organ\nc0,Brain\n"), ",", []),
             (cb.write(tmp_path / "f.csv", expression.replace("c0", "c7")), ",",
              cb.write(tmp_path / "m.csv", META.replace("c0", "c7")), ",", [("Lab", "x")])]
    error, _, _ = cb.check_add_cells(tmp_path / "stores", steps, True, chunk_bytes=chunk_bytes)          # all or nothing is checked inside
    assert error is not None and expected in error
