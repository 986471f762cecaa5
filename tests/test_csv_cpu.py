"""addCells and addCellMetaData on the host: the tokenizer against an independent Python one, the exactness rule of the
device pass against libc's strtof, and the host path of addCells end to end against the reference's loops
(tests/native/em2_csv_restatement.cpp) replayed through addGene / addCell."""
import os
import random

import numpy as np
import pytest

import csv_binding as cb
import ingest_binding as ib
from expressionmatrix2_amd import ExpressionMatrix

TOY = cb.GOLDEN

LINES = [
    "", "a", "a,b", "a,,b", "a,b,", ",", ",,", " a , b\t,\r c \v\f", '"a,b",c', '"a,b', 'a"b"c,"",d', '""', 'a\\nb,c', 'a\\,b,c', 'a\\"b,"c\\"d"',
    "a\\\\b", "a\\", "a\\x", "a,\\", '"a\\', "a;b,c;d", "a\tb c", '"a;b",c', "a\\;b", "  ", " , ", "\r", 'x,"y\nz"', "a,b\r", '"', '","', 'é,ü',
]


@pytest.mark.parametrize("separators", [",", ";,", "\t ", ",;|:/!#~"])
@pytest.mark.parametrize("trim", [False, True])
def test_tokenizer_against_an_independent_one(separators, trim):
    for line in LINES:
        try:
            expected = cb.python_tokenize(separators, line, trim)
        except cb.Failure as failure:
            with pytest.raises(cb.Failure, match=str(failure)):
                cb.restated_tokenize(separators, line, trim)
            with pytest.raises(RuntimeError, match=str(failure)):
                cb.product_tokenize(separators, line, trim)
            continue
        assert cb.restated_tokenize(separators, line, trim) == expected, repr(line)
        assert cb.product_tokenize(separators, line, trim) == expected, repr(line)


def test_tokenizer_rules_one_by_one():
    t = lambda line, trim=False, separators=",": cb.product_tokenize(separators, line, trim)
    assert t("") == [] and t("a,") == ["a", ""] and t("a,,b") == ["a", "", "b"] and t(",") == ["", ""]
    assert t('"a,b",c') == ["a,b", "c"] and t('"a,b') == ["a,b"] and t('a"b"c') == ["abc"]
    assert t("a\\nb") == ["a\nb"] and t("a\\,b") == ["a,b"] and t('a\\"b') == ['a"b'] and t("a\\\\b") == ["a\\b"]
    assert t("a\\;b;c", separators=";") == ["a;b", "c"]
    assert t(" a\t, \r\n\v\fb ", True) == ["a", "b"] and t(" a ", False) == [" a "]
    for line, text in (("a\\", "cannot end with escape"), ("a\\x", "unknown escape sequence"), ("a\\;", "unknown escape sequence")):
        with pytest.raises(RuntimeError, match=text):
            t(line)


def test_exactness_rule_against_strtof():
    """Every field the rule decides has strtof's bits; the rule defers what it must."""
    rng = random.Random(20)
    fields = list(cb.NUMBERS)
    for _ in range(4000):
        digits = rng.randint(1, 17)
        mantissa = "".join(rng.choice("0123456789") for _ in range(digits))
        point = rng.randint(0, digits)
        text = mantissa[:point] + "." + mantissa[point:] if rng.random() < .7 else mantissa
        if rng.random() < .3:
            text += "e%+d" % rng.randint(-30, 30)
        fields.append(rng.choice(["", "", "-", "+"]) + text)
    for value in list(range(0, 3000)) + [2 ** 24 - 1, 2 ** 24, 2 ** 24 + 1, 2 ** 24 + 2, 2 ** 25 + 2, 2 ** 31, 2 ** 32 + 1]:
        fields.append(str(value))
    decided = deferred = 0
    for field in fields:
        kind = cb.decide(field.encode())
        if kind[0] == "value":
            bits, consumed = cb.strtof_bits(field.strip(cb.BLANKS).encode())
            assert consumed == len(field.strip(cb.BLANKS)) and kind[1] == bits, field
            decided += 1
        elif kind[0] == "skip":
            assert field.strip(cb.BLANKS) in ("0", "0.")
        else:
            deferred += 1
    must_defer = ["16777217", "12345678901234567890", "1e23", "1e-23", "1e-50", "3abc", "0x10", "inf", "nan", "1e999", "", "\"7\"", "33554434"]
    for field in must_defer:
        assert cb.decide(field.encode()) == ("defer",), field
    for field in ("16777216", "16777218", "1e22", "1e-22", ".5", "5.", "+5", "-1", "1E+5", " 7 ", "0.0", "-0", "00", "1234567"):
        assert cb.decide(field.encode())[0] == "value", field
    for value in range(1, 1 << 24, 9973):                                     # integers below 2^24: always decided
        assert cb.decide(str(value).encode()) == ("value", int(np.array([value], np.float32).view(np.uint32)[0]))
    print("exactness rule: %d decided, %d deferred of %d generated fields" % (decided, deferred, len(fields)))


def test_deferred_share_of_random_decimals():
    """A measurement, not a gate: the share of random decimals of up to 17 digits the rule defers."""
    rng = random.Random(7)
    n, deferred = 5000, 0
    for _ in range(n):
        digits = rng.randint(1, 17)
        mantissa = "".join(rng.choice("0123456789") for _ in range(digits))
        point = rng.randint(0, digits)
        field = (mantissa[:point] or "0") + "." + mantissa[point:]
        kind = cb.decide(field.encode())
        if kind[0] == "value":
            assert kind[1] == cb.strtof_bits(field.encode())[0], field
        deferred += kind[0] == "defer"
    print("deferred share of %d random decimals of up to 17 digits: %.4f" % (n, deferred / n))
    assert deferred < n


def toy(name):
    return os.path.join(TOY, name)


def test_toy_files_on_the_host_path(tmp_path):
    steps1 = [(toy("ToyTest1/ExpressionMatrix.csv"), ",", toy("ToyTest1/MetaData.csv"), ",", [])]
    error, directory, _ = cb.check_add_cells(tmp_path / "toy1", steps1, False)
    assert error is None
    store = ib.read_store(directory)
    assert store["geneNames"] == ["Gene0", "Gene1", "Gene3"] and store["cellNames"] == ["Cell0", "Cell1", "Cell2"]
    assert store["cellMetaData"][2] == [("CellName", "Cell2"), ("Organ", "Pancreas"), ("Tumor", "No")] and store["toc"] == [0, 2, 4, 5]
    steps2 = [(toy("ToyTest2/ExpressionMatrix1.csv"), ",", toy("ToyTest2/MetaData1.csv"), ",", []),
              (toy("ToyTest2/ExpressionMatrix2.csv"), ",", toy("ToyTest2/MetaData2.csv"), ",", [])]
    error, directory, _ = cb.check_add_cells(tmp_path / "toy2", steps2, False)
    assert error is None
    store = ib.read_store(directory)
    assert store["geneNames"] == ["Ge%(ne0", "Ge=ne1", "G?en&e3", "Gene3", "Gene5", "Gene1"] and store["cellNames"][1] == "Cel?l1"
    steps4 = [(toy("ToyTest4/ExpressionMatrix.csv"), ",", toy("ToyTest4/MetaData.csv"), ",", [("Batch", "4")])]
    assert cb.check_add_cells(tmp_path / "toy4", steps4, False)[0] is None


META = "Cell,Organ\nc0,Brain\nc1,Liver\nc2,Lung\n"

# (name, expression file, meta data file, expression separators, meta data separators, additional, error or None)
CASES = [
    ("column order, an unkept column with garbage", "g,c2,zz,c0\nA,1,x!,2\nB,0,,0.5\nC, 3 ,\"q,q\",0.\n", META, ",", ",", [], None),
    ("header one token short", "c0,c1\nA,1,2\nB,3,4\n", "Organ\nc0,Brain\nc1,Liver\n", ",", ",", [], None),
    ("CRLF and no final newline", "g,c0,c1\r\nA,1,2\r\nB,0,4", "Cell,Organ\r\nc0,Brain\r\nc1,Liver", ",", ",", [], None),
    ("additional pairs and the swap", "g,c0,c1\nA,1,2\n", META, ",", ",", [("Lab", "x"), ("Run", "7")], None),
    ("an additional CellName", "g,c0\nA,1\n", META, ",", ",", [("Lab", "x"), ("CellName", "mine")], None),
    ("an additional CellName for two cells", "g,c0,c1\nA,1,2\n", META, ",", ",", [("CellName", "mine")], "Cell name mine already exists."),
    ("quotes, escapes and blanks", "g,\"c0\", c1 \n\"A,1\",1e1, 2.50\nB\\,x,\"3\",\\n4\n\"C\"\"\",+0.0,-0\n", META, ",", ",", [], None),
    ("other separators", "g;c0\tc1\nA;1\t2\nB\t0;7\n", "Cell|Organ\nc0|Brain\nc1|Liv,er\n", ";\t", "|", [], None),
    ("a long separator string", "g;c0\tc1\nA;1\t2\n", META, ";\t|:/!#~@", ",", [], None),
    ("the meta data file is not trimmed", "g,c0,c1\nA,1,2\n", "Cell,Organ\n c0,Brain\nc1, Liver \n", ",", ",", [], None),
    ("no cell is kept, the genes stay", "g,x,y\nA,1,2\nB,q,\n", META, ",", ",", [], None),
    ("every count is zero", "g,c0,c1\nA,0,0.\nB,0,0\n", META, ",", ",", [], None),
    ("accepted by strtof", "g,c0,c1,c2\nA,3abc,0x10,inf\nB,1e999,nan,1e-50\nC,16777217,.5,5.\n", META, ",", ",", [], None),
    ("a gene twice", "g,c0\nA,1\nB,2\nA,3\n", META, ",", ",", [], "Duplicate entry for gene A in cell expression counts file"),
    ("an invalid count", "g,c0,c1\nA,1,2\nB,x,y\n", META, ",", ",", [], "Invalid expression count x encountered at line 3 of file"),
    ("an empty count", "g,c1,c0\nA,1,2\nB,3,4\nC,,y\n", META, ",", ",", [], "Invalid expression count (empty) encountered at line 4 of file"),
    ("kept order decides the invalid count", "g,c1,zz,c0\nA,p,q,r\n", META, ",", ",", [], "Invalid expression count p encountered at line 2"),
    ("token count before duplicate gene before invalid count", "g,c0\nA,1\nA,x,3\n", META, ",", ",", [], "Unexpected number of items in line of expression counts file"),
    ("duplicate gene before invalid count", "g,c0\nA,1\nA,x\n", META, ",", ",", [], "Duplicate entry for gene A"),
    ("the first line wins", "g,c0\nA,x\nA,1\nB\n", META, ",", ",", [], "Invalid expression count x encountered at line 2"),
    ("an empty line", "g,c0\nA,1\n\nB,2\n", META, ",", ",", [], "Empty line in expression counts file"),
    ("a line of one carriage return", "g,c0\nA,1\n\r\nB,2\n", META, ",", ",", [], "Unexpected number of items in line of expression counts file"),
    ("an empty second line", "g,c0\n\nA,1\n", META, ",", ",", [], "Empty line in expression counts file"),
    ("an unknown escape", "g,c0\nA,1\nB\\q,2\n", META, ",", ",", [], "unknown escape sequence"),
    ("an escape at the end", "g,c0\nA,1\nB,2\\\n", META, ",", ",", [], "cannot end with escape"),
    ("a negative count", "g,c0,c1\nA,1,2\nB,3,-4\n", META, ",", ",", [], "Negative expression count encountered."),
    ("a parse error before an addCell error", "g,c0,c1\nA,1,-2\nB,3,x\n", META, ",", ",", [], "Invalid expression count x"),
    ("a cell twice in the header", "g,c0,c0\nA,1,2\n", META, ",", ",", [], "Cell name c0 already exists."),
    ("a header that fits nothing", "a,b,c,d\nA,1\n", META, ",", ",", [], "Number of tokens in header line of expression counts file"),
    ("an empty header", "\nA,1\n", META, ",", ",", [], "Error reading header line from expression counts file"),
    ("one line only", "g,c0\n", META, ",", ",", [], "Error reading the second line of file"),
    ("an empty expression file", "", META, ",", ",", [], "Error reading header line of file"),
    ("a meta data header that fits nothing", "g,c0\nA,1\n", "a,b,c,d\nc0,Brain\n", ",", ",", [], "Number of tokens in header line of cell meta data file"),
    ("a short meta data line", "g,c0\nA,1\n", "Cell,Organ\nc0,Brain\nc1\n", ",", ",", [], "Unexpected number of items in line of cell meta data file"),
    ("a cell twice in the meta data", "g,c0\nA,1\n", "Cell,Organ\nc0,Brain\nc0,Liver\n", ",", ",", [], "Duplicate cell name c0 in cell meta data file"),
    ("an empty meta data line", "g,c0\nA,1\n", "Cell,Organ\nc0,Brain\n\nc1,Liver\n", ",", ",", [], "Empty line in cell meta data file"),
    ("an empty meta data header", "g,c0\nA,1\n", "\nc0,Brain\n", ",", ",", [], "Error reading header line from cell meta data file"),
]


@pytest.mark.parametrize("case", CASES, ids=[case[0] for case in CASES])
def test_add_cells_on_the_host_path(tmp_path, case):
    _, expression, meta, expression_separators, meta_separators, additional, expected = case
    steps = [(cb.write(tmp_path / "e.csv", expression), expression_separators, cb.write(tmp_path / "m.csv", meta), meta_separators, additional)]
    error, directory, _ = cb.check_add_cells(tmp_path / "stores", steps, False)
    if expected is None:
        assert error is None
    else:
        assert error is not None and expected in error


def test_add_cells_details_on_the_host_path(tmp_path):
    expression = cb.write(tmp_path / "e.csv", "g,c2,zz,c0\nA,1,x!,2\nB,0,,0.5\n")
    meta = cb.write(tmp_path / "m.csv", META)
    e = ExpressionMatrix.create(str(tmp_path / "s"))
    import expressionmatrix2_amd.expression_matrix as facade
    saved, facade.CSV_USE_DEVICE = facade.CSV_USE_DEVICE, False
    try:
        assert e.addCells(expressionCountsFileName=expression, cellMetaDataFileName=meta, additionalCellMetaData=[("Lab", "x")]) is None
        with pytest.raises(RuntimeError, match="Could not open file"):
            e.addCells(expressionCountsFileName=expression, cellMetaDataFileName=str(tmp_path / "missing.csv"))
        with pytest.raises(RuntimeError, match="Cell name c2 already exists."):
            e.addCells(expressionCountsFileName=expression, cellMetaDataFileName=meta)
        with pytest.raises(TypeError):
            e.addCells(expressionCountsFileName=expression)
    finally:
        facade.CSV_USE_DEVICE = saved
    e.close()
    store = ib.read_store(str(tmp_path / "s"))
    assert store["cellNames"] == ["c2", "c0"] and store["geneNames"] == ["A", "B"]             # the order of the file's columns
    assert store["cellMetaData"][0] == [("CellName", "c2"), ("Lab", "x"), ("Organ", "Lung")]    # the swap puts Lab where CellName stood
    assert store["toc"] == [0, 1, 3]


META_DATA_CASES = [
    ("plain", "Cell,Organ,Tumor\nc0,Brain,Yes\nc1, Liver ,No\n", None),
    ("an empty header name skips its column, a set field is overwritten", "x,,Stage,Organ\nc1,a,b,c\nc1,d,e,f\nc0,\"g,h\",i\\nj,k\n", None),
    ("no trailing carriage return handling", "Cell,Organ\r\nc0,Brain\r\n", None),
    ("a short line", "Cell,Organ\nc0,Brain\nc1\n", "Unexpected number of meta data values in"),
    ("an unknown cell", "Cell,Organ\nc0,Brain\nzz,Liver\n", "Attempt to add meta data for undefined cell zz"),
    ("an empty file", "", "Error reading the header line from file"),
    ("an empty header line", "\nc0\n", "Invalid format of cell meta data file"),
    ("an empty line", "Cell,Organ\n\n", "Unexpected number of meta data values in"),
]


@pytest.mark.parametrize("case", META_DATA_CASES, ids=[case[0] for case in META_DATA_CASES])
def test_add_cell_meta_data(tmp_path, case):
    _, content, expected = case
    path = cb.write(tmp_path / "more.csv", content)
    stores = []
    for name in ("product", "replayed"):
        e = ExpressionMatrix.create(str(tmp_path / name))
        for cell in ("c0", "c1"):
            e.addCell([("CellName", cell), ("Organ", "none")], [("A", 1.)])
        stores.append(e)
    product, replayed = stores
    product.flush()
    before = ib.file_bytes(str(tmp_path / "product"))
    if expected is None:
        cb.replay(replayed, cb.restated_add_cell_meta_data(path, ["c0", "c1"]))
        assert product.addCellMetaData(path) is None
    else:
        with pytest.raises(cb.Failure, match=expected):
            cb.restated_add_cell_meta_data(path, ["c0", "c1"])
        with pytest.raises(RuntimeError, match=expected):
            product.addCellMetaData(path)
        product.flush()
        assert ib.file_bytes(str(tmp_path / "product")) == before            # all or nothing
    product.close()
    replayed.close()
    if expected is None:
        a, b = ib.read_store(str(tmp_path / "product")), ib.read_store(str(tmp_path / "replayed"))
        assert a == b
        if case[0] == "plain":
            assert a["cellMetaData"][1] == [("CellName", "c1"), ("Organ", "Liver"), ("Tumor", "No")]
    with pytest.raises(RuntimeError, match="Error opening"):
        ExpressionMatrix(str(tmp_path / "product")).addCellMetaData(str(tmp_path / "missing.csv"))
