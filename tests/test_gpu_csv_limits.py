"""em2_dev_csv_parse and csvSessionFinish where no feature test reaches them (the cases of tests/ingest_limit_cases.py, each proven
to reach its branch by tests/test_ingest_limit_cases_cpu.py), against the model of the entry's outputs with nothing discarded
and no tolerance (csv_binding.assert_parse), and through the facade against the replayed restatement and the host path
(csv_binding.check_add_cells):

  C1  the stage of csvFieldsKernel flushes mid-line: lines of 2000 decided counts, three waves flushing into one list; the
      flush condition at staged 490, 500 and 511 with 32 joining and at 511 with 1 and 2 joining; deferred fields between
      flushes; a triple capacity of 700 of 6000
  C2  the 64-byte step: separators, quotes that open and close, quoted separators and a carriage return at offsets 62 .. 65 and
      127 .. 129 of a line, a field over three steps, lines of exactly 63 .. 192 bytes (the extra step of a multiple of 64)
  C3  the second trips of the three grid-stride loops: more than 65 536 lines (a stage that a wave's first line began is flushed
      at the kernel's end, and in the middle of a second line of 600 counts), more than 65 536 tiles
  C4  decideField on 20 000 random numeric fields, 20 000 float midpoints and their neighbours, and the edges of the rule
  C5  NUL, VT, FF, TAB and bytes from 0x80 in a text
  C6  csvSessionFinish's key packing with 1 .. 257 lines and 1 .. 5 kept cells, an empty CSR row first, in the middle and last,
      host triples only, no triples at all

Where the issue names "0.1" as a deferred field the cases hold "16777217" (a float midpoint) or a quoted count: the rule decides
"0.1" (one digit, one exact division).  A single kept cell cannot be all "0" and hold a deferred field, so in the C6 files that
keep one cell the empty CSR row is left to the file whose counts are all "0".

Wall time on an MI355X: 9.2 s for the 23 tests of this file (model included), of which C3(b), 70 000 lines with 1.35 million
decided counts, takes 4.0 s -- nearly all of it the Python model -- and no other test more than 0.4 s.

Checked against mutated libraries (built outside the tree, selected with EM2_LIBRARY): flushStaged copying staged - 1 entries
fails every test here; the quote state not carried from step to step fails C2 (and C5, C6[256]); fieldBegin taken from a
step's first closer fails C1, C2, C3(b), C3(c), C5 and C6[255 .. 257]; a stride of gridDim.x * 4 + 4 lines fails the three C3 tests over lines;
the flush condition with >= instead of > changes no output and fails nothing."""
import os
import random

import numpy as np
import pytest

import csv_binding as cb
import ingest_binding as ib
import ingest_limit_cases as lc
from expressionmatrix2_amd import capi

pytestmark = pytest.mark.gpu


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


# ---- C1 ----
@pytest.mark.parametrize("variant", ["a", "c"])
def test_c1_wide_lines(torch, tile, variant):
    tile(lc.C1_TILE)
    text, columns, kept = lc.c1_wide(kept_every_third_out=variant == "c", deferred_every_fifth=variant == "c")
    got = cb.assert_parse(torch, text, ",", columns, kept, "C1(%s)" % variant)
    if variant == "a":
        assert got["counts"] == [3, 6000, 0]
    else:
        assert got["counts"][2] > 700 and got["counts"][1] > 3 * 2 * lc.K_STAGED


def test_c1_the_flush_condition_at_its_edge(torch, tile):
    tile(lc.C1_TILE)
    text, columns, kept, decided = lc.c1_marks()
    got = cb.assert_parse(torch, text, ",", columns, kept, "C1(b)")
    assert got["counts"] == [len(decided), sum(decided), 0]


def test_c1_a_triple_capacity_below_the_count(torch, tile):
    tile(lc.C1_TILE)
    text, columns, kept = lc.c1_wide()
    full = cb.assert_parse(torch, text, ",", columns, kept, "C1(d), full")
    short = cb.device_parse(torch, text, ",", columns, kept, capacities=(3, 700, 0))       # the guards are checked inside
    assert short["counts"] == [3, 6000, 0] and np.array_equal(short["lines"], full["lines"])
    assert len(short["triples"]) == 700 and short["triples"] <= full["triples"]            # 700 distinct slots were written


# ---- C2 ----
@pytest.mark.parametrize("tile_bytes", lc.C2_TILES)
def test_c2_the_64_byte_step(torch, tile, tile_bytes):
    tile(tile_bytes)
    text, columns, kept, where = lc.c2_text()
    cb.assert_parse(torch, text, ",", columns, kept, "C2, tile %d" % tile_bytes)
    for what, begin, end in where[::7]:                       # and each line alone behind its ordinary line: the begin moves
        alone = lc.C2_ORDINARY[begin % 3] + text[begin:text.index(b"\n", begin) + 1]
        cb.assert_parse(torch, alone, ",", columns, kept, "C2 %s, tile %d" % (what, tile_bytes))


# ---- C3 ----
def test_c3_lines_on_a_second_trip(torch, tile):
    tile(0)
    text, columns, kept = lc.c3_lines()
    got = cb.assert_parse(torch, text, ",", columns, kept, "C3(a)")
    assert got["counts"] == [lc.C3_LINES, lc.C3_LINES, 0]


def test_c3_wide_lines_on_a_second_trip(torch, tile):
    tile(0)
    text, columns, kept = lc.c3_wide_tail()
    got = cb.assert_parse(torch, text, ",", columns, kept, "C3(b)")
    assert got["counts"][1] == lc.C3_LINES - lc.C3_WIDE_LINES + lc.C3_WIDE_LINES * lc.C3_WIDE_COLUMNS


def test_c3_a_second_line_flushes_what_the_first_staged(torch, tile):
    tile(0)
    text, columns, kept = lc.c3_late_flush()
    got = cb.assert_parse(torch, text, ",", columns, kept, "C3, a mid-line flush in a wave's second line")
    assert got["counts"] == [65536 + lc.C3_LATE_LINES, 65536 + lc.C3_LATE_LINES * lc.C3_LATE_COLUMNS, 0]


@pytest.mark.parametrize("misalign", [0, 9])
def test_c3_tiles_on_a_second_trip(torch, tile, misalign):
    tile(lc.C3_TILE)
    text, columns, kept = lc.c3_tiles()
    got = cb.assert_parse(torch, text, ",", columns, kept, "C3(c), misaligned by %d" % misalign, misalign=misalign)
    assert got["counts"] == [lc.C3_TILE_LINES, lc.C3_TILE_LINES, 0]


# ---- C4 ----
@pytest.mark.parametrize("family", ["plain", "midpoints", "edges"])
def test_c4_numeric_fields(torch, tile, family):
    tile(lc.C4_TILE)
    fields = {"plain": lambda: lc.c4_plain(random.Random(1)), "midpoints": lambda: [f for f, _ in lc.c4_midpoints(random.Random(2))],
              "edges": lambda: list(lc.C4_EDGES)}[family]()
    text, columns, kept = lc.c4_text(fields)
    got = cb.assert_parse(torch, text, ",", columns, kept, "C4 " + family)
    decided = {(line, cell) for cell, line, _ in got["triples"]}
    mine = sum(1 for at in lc.c4_field_of_line(fields) if at in decided)
    print("C4 %s: %d of %d fuzzed fields decided on the device" % (family, mine, len(fields)))
    if family == "midpoints":
        assert mine == len(fields) - -(-len(fields) // 3)
    if family == "plain":
        assert mine >= 0.75 * len(fields)


# ---- C5 ----
def test_c5_bytes(torch, tile):
    for i, (text, columns, kept, tile_bytes, misalign) in enumerate(lc.c5_all()):
        tile(tile_bytes)
        cb.assert_parse(torch, text, ",", columns, kept, "C5 text %d" % i, misalign=misalign)


# ---- C6 ----
@pytest.mark.parametrize("gene_lines", lc.C6_GENE_LINES)
def test_c6_session_finish_through_the_facade(torch, tmp_path, gene_lines):
    for number, f in enumerate(lc.c6_files(gene_lines)):
        base = tmp_path / ("f%d" % number)
        os.makedirs(str(base))
        steps = [(cb.write(base / "e.csv", f["expression"]), ",", cb.write(base / "m.csv", f["meta"]), ",", [])]
        error, host_dir, none = cb.check_add_cells(base / "host", steps, False)
        assert error is None and none == [0]
        host = ib.read_store(host_dir)
        assert host["cellNames"] == f["kept"] and len(host["geneNames"]) == gene_lines
        if f["empty"] is not None:
            cell = f["kept"].index(f["empty"])
            assert host["toc"][cell] == host["toc"][cell + 1]
        for chunk_bytes in lc.C6_CHUNK_BYTES:
            error, device_dir, deferred = cb.check_add_cells(base / ("device%d" % chunk_bytes), steps, True, chunk_bytes=chunk_bytes)
            assert error is None and (deferred == [0] if f["kind"] == "zero" else deferred[0] > 0), (f["kind"], deferred)
            assert ib.read_store(device_dir) == host
