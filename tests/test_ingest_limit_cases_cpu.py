"""Every case of tests/ingest_limit_cases.py reaches the branch it is there for: asserted here from the model of
em2_dev_csv_parse (csv_binding.model_parse, decide), libc's strtof and the restatement of the ingest
(tests/native/em2_ingest_restatement.cpp) alone, without a GPU.  These are conditions, not measurements: they keep
tests/test_gpu_csv_limits.py and tests/test_gpu_ingest_limits.py from passing empty."""
import random

import numpy as np
import pytest

import csv_binding as cb
import ingest_binding as ib
import ingest_limit_cases as lc


def decided_per_line(model, lines):
    counts = [0] * lines
    for _, line, _ in model["triples"]:
        counts[line] += 1
    return counts


def emitters_of(text, begin, end, kept):
    """The closer positions, relative to the line's begin, of the kept fields the model decides with a value."""
    line, out, start = text[begin:end], [], 0
    for column, closer in enumerate(lc.closers_of(line)):
        if column < len(kept) and kept[column] != lc.NONE and cb.decide(line[start:closer])[0] == "value":
            out.append(closer)
        start = closer + 1
    return out


# ---- C1 ----
@pytest.mark.parametrize("variant", ["a", "c"])
def test_c1_wide_lines_flush_mid_line(variant):
    text, columns, kept = lc.c1_wide(kept_every_third_out=variant == "c", deferred_every_fifth=variant == "c")
    model = cb.model_parse(text, ",", columns, kept)
    assert (model["lines"][:, 3] == cb.OK).all() and len(model["lines"]) == 3
    per_line = decided_per_line(model, 3)
    if variant == "a":
        assert per_line == [2000] * 3 and not model["deferred"]
    else:
        kept_columns = sum(1 for k in kept if k != lc.NONE)
        assert len(model["deferred"]) * 5 >= kept_columns * 3 * 0.19 * 5 and min(per_line) > 2 * lc.K_STAGED
        assert sum(per_line) + len(model["deferred"]) == 3 * kept_columns
    for begin, end in cb.lines_of(text):
        flushes, _ = lc.stage_flushes(emitters_of(text, begin, end, kept))
        assert len(flushes) >= 2                              # the restart behind a flush is followed by another flush


def test_c1_marks_meet_the_stage_at_its_edge():
    text, columns, kept, decided = lc.c1_marks()
    model = cb.model_parse(text, ",", columns, kept)
    assert decided_per_line(model, len(decided)) == decided and not model["deferred"]
    assert set(decided) == {511, 512, 513, 575, 576, 577} and decided[:2] == [512, 513]
    met = set()
    for (begin, end), count in zip(cb.lines_of(text), decided):
        flushes, behind = lc.stage_flushes(emitters_of(text, begin, end, kept))
        assert len(flushes) == (1 if count > lc.K_STAGED else 0) and behind == (count - flushes[0][0] if flushes else count)
        met.update(flushes)
    assert {(490, 32), (500, 32), (511, 32), (511, 2)} <= met                # (staged, emitters of the step that flushes)


# ---- C2 ----
def test_c2_closers_at_the_ends_of_a_step():
    text, columns, kept, where = lc.c2_text()
    model = cb.model_parse(text, ",", columns, kept)
    table = {int(row[0]): row for row in model["lines"]}
    residues, lengths, parities = set(), set(), set()
    quote_carried = False
    for what, begin, end in where:
        row = table[begin]
        assert int(row[1]) == end, what
        closers = lc.closers_of(text[begin:end])
        assert len(closers) == int(row[2]) <= columns, what                    # the model sees the same fields
        residues.update(c % 64 for c in closers)
        lengths.add((end - begin) % 64)
        parities.add(begin & 1)
        line = text[begin:end]
        opened = False
        for i, byte in enumerate(line):                       # a quote open at the end of one step that hides a separator in the next
            if i and i % 64 == 0 and opened and b"," in line[i:i + 64].split(b'"')[0]:
                quote_carried = True
            opened ^= byte == 0x22
        if "from before 64" in what:
            spans = [(a + 1, b) for a, b in zip([-1] + closers, closers)]
            assert any(a < 64 and b > 192 for a, b in spans), what
    assert {0, 63} <= residues and 0 in lengths and parities == {0, 1} and quote_carried
    for length in lc.C2_LENGTHS:
        assert sum(1 for what, begin, end in where if what.startswith("%d bytes" % length) and end - begin == length) == 2
    for p in lc.C2_POSITIONS:
        assert any(end - begin == p and text[end:end + 2] == b"\r\n" for _, begin, end in where)
    line_of_begin = {int(row[0]): i for i, row in enumerate(model["lines"])}
    decided_lines = {line for _, line, _ in model["triples"]}
    for what, begin, end in where:                            # "a decided field last": the line's last column is decided
        if "a decided field last" in what:
            last = int(table[begin][2]) - 1
            assert (kept[last], line_of_begin[begin], 0x40e00000) in model["triples"] and line_of_begin[begin] in decided_lines, what
        if "an empty field last" in what:
            assert any(d[0] == line_of_begin[begin] and d[2] == d[3] == end for d in model["deferred"]), what


# ---- C3 ----
def test_c3_second_trips():
    text, columns, kept = lc.c3_lines()
    model = cb.model_parse(text, ",", columns, kept)
    assert len(model["lines"]) == lc.C3_LINES > 65536 and lc.lines_on_a_second_trip(lc.C3_LINES) == lc.C3_LINES - 65536
    assert len(model["triples"]) == lc.C3_LINES and lc.tile_count(len(text), 0, 0) < 65536
    text, columns, kept = lc.c3_wide_tail()
    lines = cb.lines_of(text)
    assert len(lines) == lc.C3_LINES > 65536
    second = lines[65536:]                                    # the wave of line l took line l - 65536 first: an "a,1" line
    assert all(end - begin > 2 * lc.C3_WIDE_COLUMNS for begin, end in second) and lc.C3_LINES - lc.C3_WIDE_LINES <= 65536
    assert all(text[begin:end] == b"a,1" for begin, end in lines[:len(second)])
    begin, end = second[0]
    assert len(emitters_of(text, begin, end, kept)) == lc.C3_WIDE_COLUMNS
    text, columns, kept = lc.c3_late_flush()
    lines = cb.lines_of(text)
    assert lc.lines_on_a_second_trip(len(lines)) == lc.C3_LATE_LINES and all(text[b:e] == b"a,1" for b, e in lines[:lc.C3_LATE_LINES])
    for begin, end in lines[65536:]:                          # one count is staged when the wave's second line begins
        flushes, behind = lc.stage_flushes(emitters_of(text, begin, end, kept), staged=1)
        assert len(flushes) == 1 and flushes[0][0] > 480 and behind == 1 + lc.C3_LATE_COLUMNS - flushes[0][0]
    text, columns, kept = lc.c3_tiles()
    assert len(text) == 1065000
    for misalign in (0, 9):
        tiles = lc.tile_count(len(text), misalign, lc.C3_TILE)
        assert tiles > 65536 and lc.tile_grid(tiles) == 65536


# ---- C4 ----
def held_to_strtof(fields):
    """-> (decided, deferred, skipped); every decided field has strtof's bits."""
    decided = deferred = skipped = 0
    for field in fields:
        kind = cb.decide(field.encode())
        if kind[0] == "value":
            trimmed = field.strip(cb.BLANKS).encode()
            bits, consumed = cb.strtof_bits(trimmed)
            assert consumed == len(trimmed) and kind[1] == bits, field
            decided += 1
        elif kind[0] == "skip":
            assert field.strip(cb.BLANKS) in ("0", "0.")
            skipped += 1
        else:
            deferred += 1
    return decided, deferred, skipped


def test_c4_plain_fields():
    fields = lc.c4_plain(random.Random(1))
    decided, deferred, skipped = held_to_strtof(fields)
    print("C4 plain: %d decided, %d deferred, %d skipped of %d" % (decided, deferred, skipped, len(fields)))
    assert len(fields) == lc.C4_COUNT and decided >= 0.75 * len(fields) and deferred > 1000


def test_c4_midpoints_are_deferred_and_their_neighbours_decided():
    fields = lc.c4_midpoints(random.Random(2))
    for field, kind in fields:
        assert cb.decide(field.encode())[0] == ("defer" if kind == "midpoint" else "value"), field
    decided, deferred, _ = held_to_strtof([field for field, _ in fields])
    assert deferred == -(-len(fields) // 3) and decided + deferred == len(fields)          # exactly one third
    assert len(set(field for field, _ in fields)) > 0.99 * len(fields)


def test_c4_edges():
    decided, deferred, skipped = held_to_strtof(lc.C4_EDGES)
    kinds = {field: cb.decide(field.encode())[0] for field in lc.C4_EDGES}
    assert kinds["0" * 30 + "12"] == "value" and kinds["0" * 31 + "12"] == "defer"           # 32 and 33 bytes
    assert kinds[" " * 5 + "0" * 29 + "77" + " " * 5] == "value"
    assert kinds["9007199254740992"] == "value" and kinds["9007199254740993"] == "defer"
    assert kinds["1e22"] == "value" and kinds["1e23"] == "defer" and kinds["1e-22"] == "value" and kinds["1e-23"] == "defer"
    assert kinds["1e0022"] == "value" and kinds["1e00022"] == "defer"
    assert kinds["1234567890123456789"] == "defer" and kinds["12345678901234567890"] == "defer"
    assert kinds["9007199254740992e22"] == "value" and kinds["1.7014118e38"] == "defer" and kinds["1.17549435e-38"] == "defer"
    assert kinds["-0.0"] == "value" and kinds["0"] == "skip" and kinds["0."] == "skip" and kinds[".0"] == "value"
    assert decided >= 30 and deferred >= 30 and skipped == 2


# ---- C5 ----
def test_c5_texts_hold_the_bytes():
    cases = lc.c5_all()
    assert len(cases) == 42
    seen = set()
    for text, columns, kept, tile, misalign in cases:
        assert 1 <= len(text) <= 400 and tile in lc.C5_TILES and 0 <= misalign <= 15
        seen.update(text)
        cb.model_parse(text, ",", columns, kept)              # the model takes every byte
    assert {0, 0x0b, 0x0c, 0x09, 0x80, 0xc3, 0xa9, 0xff} <= seen
    assert set(cases[-2][0]) == {0xff} and set(cases[-1][0]) == {0}
    misalignments = {case[4] for case in cases}
    assert len(misalignments) >= 12


# ---- C6 ----
def test_c6_files():
    positions, keeps, powers = set(), set(), set()
    for gene_lines in lc.C6_GENE_LINES:
        files = lc.c6_files(gene_lines)
        assert [len(f["expression"].split("\n")[0].split(",")) - 1 for f in files[:5]] == list(lc.C6_CELLS)
        for f in files:
            lines = f["expression"].encode().split(b"\n")[1:-1]
            names = f["expression"].split("\n")[0].split(",")[1:]
            assert len(lines) == gene_lines
            kept = [lc.NONE] + [f["kept"].index(n) if n in f["kept"] else lc.NONE for n in names]
            model = cb.model_parse(b"\n".join(lines) + b"\n", ",", len(names) + 1, kept)
            assert (model["lines"][:, 3] == cb.OK).all()
            keeps.add(len(f["kept"]))
            if f["kind"] == "zero":
                assert not model["triples"] and not model["deferred"]
                continue
            assert model["deferred"], "no deferred field"
            if f["kind"] == "deferred":
                assert all(bits == 0 for _, _, bits in model["triples"])
            if f["empty"] is not None:
                cell = f["kept"].index(f["empty"])
                assert all(c != cell for c, _, _ in model["triples"]) and all(kept[column] != cell for _, column, _, _ in model["deferred"])
                positions.add("first" if cell == 0 else "last" if cell == len(f["kept"]) - 1 else "middle")
            else:
                assert len(f["kept"]) == 1
        powers.add(gene_lines & (gene_lines - 1) == 0)
    assert positions == {"first", "middle", "last"} and {1, 2, 3, 4, 5} <= keeps and powers == {True, False}


# ---- the ingest cases ----
def restate(indptr, indices, values, genes=None, skip=None):
    return ib.restate(ib.Csr.from_arrays(indptr, indices, values, skip), lc.gene_map() if genes is None else genes)


@pytest.mark.parametrize("case", ["i1", "i2"])
def test_i1_i2_plants_and_second_trips(case):
    build, limit, rows, short, long = {"i1": (lc.i1, lc.I1_LIMIT, lc.I1_ROWS, lc.I1_SHORT, lc.I1_LONG),
                                       "i2": (lc.i2, lc.I2_LIMIT, lc.I2_ROWS, lc.I2_SHORT, lc.I2_LONG)}[case]
    indptr, indices, values, plants = build(True)
    lengths = np.diff(indptr.astype(np.int64))
    trips = lc.ingest_second_trips(lengths, None, limit)
    assert len(lengths) == rows and lengths.min() == short and lengths.max() == long
    assert trips == ((0, 0, rows - lc.GLOBAL_BLOCKS) if case == "i1" else (0, rows - lc.LDS_BLOCKS, 0)) and max(trips) >= 76
    expected = restate(indptr, indices, values)
    status = expected["status"]
    assert (status[plants["duplicate"]] == ib.DUPLICATE).all() and status.sum() == ib.DUPLICATE * len(plants["duplicate"])
    for key, length in (("short", short), ("long", long)):
        assert len(plants[key]) >= 200 and (lengths[plants[key]] == length).all() and not status[plants[key]].any()
    assert len(plants["duplicate"]) >= 200
    for row in plants["duplicate"]:
        assert all(status[n] == 0 for n in (row - 1, row + 1) if 0 <= n < rows)
    assert (expected["kept"] == lengths).all()
    indptr, indices, values, _ = build(False)                 # the second call: nothing fails, the fill runs
    assert not restate(indptr, indices, values)["status"].any()
    kinds = [lc.sums_in_parallel(values[int(indptr[r]):int(indptr[r + 1])]) for r in range(8)]
    assert True in kinds and False in kinds                   # integers and fractions mixed


def test_i3_the_wave_kernel_takes_a_second_row():
    indptr, indices, values, duplicate = lc.i3("first")
    lengths = np.diff(indptr.astype(np.int64))
    assert len(lengths) == lc.I3_ROWS and lc.ingest_second_trips(lengths, None, 0) == (lc.I3_EDGE, 0, 0)
    assert (lengths[:lc.I3_EDGE] == 512).all() and (lengths[-lc.I3_EDGE:] == 3).all() and lengths[lc.I3_EDGE:-lc.I3_EDGE].max() == 2
    assert lengths.max() <= lc.wave_limit(0)
    status = restate(indptr, indices, values)["status"]
    assert duplicate.tolist() == list(range(0, 70, 2)) and (status[duplicate] == ib.DUPLICATE).all() and status.sum() == 2 * 35
    indptr, indices, values, duplicate = lc.i3("swapped")
    status = restate(indptr, indices, values)["status"]
    assert (status[-lc.I3_EDGE:] == ib.DUPLICATE).all() and not status[:-lc.I3_EDGE].any() and len(duplicate) == lc.I3_EDGE
    indptr, indices, values, _ = lc.i3("clean")
    assert not restate(indptr, indices, values)["status"].any()


def test_i4_rows_are_what_they_are_called():
    for index_count in (lc.GENES, lc.GENES - 40):
        rows = lc.i4_rows(index_count)
        assert [status for _, _, status in rows] == [0, 3, 3, 0, 3, 3, 3, 0, 3, 0] and len(rows[8][0]) == 700
        for entries, skipped, status in rows:
            bad = [index for index, value in entries if value != 0 and index >= index_count]
            assert (status == 3) == (bool(bad) and not skipped)
        assert any(index >= index_count and value == 0 for index, value in rows[3][0])
        assert any(value < 0 for _, value in rows[4][0]) and any(index >= index_count and value < 0 for index, value in rows[5][0])
        kept_indices = [index for index, value in rows[6][0] if value != 0]
        assert len(set(kept_indices)) < len(kept_indices)
        assert rows[8][0][-1][0] == index_count and all(index < index_count for index, _ in rows[8][0][:-1])
        assert any(lc.GENES - 40 <= index < lc.GENES for entries, _, _ in lc.i4_rows(lc.GENES - 40) for index, _ in entries)


def test_i5_rows_and_moved_tocs():
    indptr, indices, values = lc.i5()
    lengths = np.diff(indptr.astype(np.int64))
    assert lengths.tolist() == list(lc.I5_LENGTHS)
    assert lc.ingest_rows_per_kernel(lengths, None, 0) == (4, 1, 1) and lc.ingest_rows_per_kernel(lengths, None, 16) == (4, 0, 4)
    expected = restate(indptr, indices, values)
    assert not expected["status"].any() and (expected["kept"] == lengths - 2).all()
    moved = lc.i5_moved_tocs(expected["toc"])
    assert len(moved) == 6 and {(b, s) for b, s, _ in moved} == {(b, s) for b in (1, 2, 3) for s in (-1, 1)}
    for _, _, toc in moved:
        assert toc[0] == 0 and toc[-1] == expected["toc"][-1] and (np.diff(toc.astype(np.int64)) >= 0).all()
        assert (toc != expected["toc"]).sum() == 1


def test_i6_rows_lie_on_both_sides_of_the_switch():
    rows = lc.i6_rows()
    for what, values, parallel in rows:
        assert lc.sums_in_parallel(values) == parallel, what
    products = {what: int(values.max()) ** 2 * len(values) for what, values, _ in rows[:7]}
    assert [products[w] for w in ("a single 2^26", "four of 2^25", "2^12 of 2^20", "2^16 of 2^18")] == [1 << 52] * 4
    assert all(products[w] > 1 << 52 for w in ("five of 2^25", "2^12 + 1 of 2^20", "2^16 + 1 of 2^18"))
    assert float(np.float32(2 ** 26 + 4)) == 2 ** 26
    indptr, indices, values, genes = lc.i6()
    lengths = np.diff(indptr.astype(np.int64))
    assert lc.ingest_rows_per_kernel(lengths, None, 0)[1:] == (2, 3)        # the LDS and the global-memory kernel meet the switch too
    expected = restate(indptr, indices, values, genes)
    assert not expected["status"].any()
    cells = expected["cells"].view(ib.CELL_DTYPE)
    assert cells["sum2"][0] == 2.0 ** 52 and cells["sum2"][1] == 2.0 ** 52 and cells["sum2"][3] == 2.0 ** 52


# ---- the fuzzer's draws ----
def test_the_draws_are_well_formed():
    rng = np.random.default_rng(3)
    for _ in range(30):
        case = lc.draw_csv_parse(rng)
        model = cb.model_parse(case["text"], case["separators"], case["columns"], case["kept"])
        assert len(case["kept"]) == case["columns"] and len(model["lines"]) >= 1
    seen = set()
    for _ in range(30):
        case = lc.draw_ingest(rng)
        csr = ib.Csr.from_arrays(case["indptr"], case["indices"], case["values"], case["skip"])
        expected = ib.restate(csr, lc.gene_map())
        seen.update(expected["status"].tolist())
    assert seen == {0, 1, 2}
