"""The inputs of tests/test_gpu_csv_limits.py and tests/test_gpu_ingest_limits.py, built here so that
tests/test_ingest_limit_cases_cpu.py can prove without a GPU that every one of them reaches the branch of csrc/em2_csv.hip or
csrc/em2_ingest.hip it is there for: a GPU run then cannot pass because an input quietly missed its target.  tools/fuzz_parity.py
draws its csv_parse and ingest legs from the generators at the end.

Plain data and small generators: neither torch nor the library is imported.  The formulas that decide which branch a case reaches
are restated here from the two files:

  csvFieldsKernel    a wave per line, 4 lines per block, min(ceil(lines / 4), 16384) blocks; 64 bytes per step, steps at
                     begin, begin + 64, ... while base <= end; decided counts staged 512 per wave (kStaged), flushed when
                     staged + popcount(emitted) > 512 and at the kernel's end
  csvCountKernel,    a block per tile, min(tiles, 65536) blocks; tiles = ceil((bytes + misalignment) / tile bytes), the tile
  csvLinesKernel     bytes rounded up to 16, 16384 by default
  ingestKernel       waveLimit = min(ldsLimit, 512); rows up to waveLimit: a wave each, min(cells, 2^20) blocks; listed rows up
                     to ldsLimit: min(listed, 4096) blocks; longer rows: min(listed, 1024) blocks
  the sums           in parallel where every kept value is a finite integer, none negative, and largest^2 * kept <= 2^52"""
import random

import numpy as np

NONE = 0xffffffff

# ---- the formulas ----
K_STAGED = 512
LINES_PER_BLOCK = 4
MAX_FIELD_BLOCKS = 16384
MAX_TILE_BLOCKS = 65536
DEFAULT_TILE_BYTES = 16384
WAVE_ROW_LIMIT = 512
DEFAULT_LDS_ROW_LIMIT = 8192
WAVE_BLOCKS, LDS_BLOCKS, GLOBAL_BLOCKS = 1 << 20, 4096, 1024


def field_grid(lines):
    return min(-(-lines // LINES_PER_BLOCK), MAX_FIELD_BLOCKS)


def lines_on_a_second_trip(lines):
    """The lines a wave of csvFieldsKernel takes after its first one."""
    return max(0, lines - field_grid(lines) * LINES_PER_BLOCK)


def tile_count(byte_count, misalign, tile_bytes):
    tile = (tile_bytes + 15) & ~15 if tile_bytes else DEFAULT_TILE_BYTES
    return (byte_count + misalign + tile - 1) // tile


def tile_grid(tiles):
    return min(tiles, MAX_TILE_BLOCKS)


def wave_limit(lds_limit):
    return min(lds_limit or DEFAULT_LDS_ROW_LIMIT, WAVE_ROW_LIMIT)


def ingest_rows_per_kernel(lengths, skip, lds_limit):
    """-> (rows of the wave kernel's grid loop, rows listed for the LDS workgroup kernel, rows listed for the global-memory one).
    The wave kernel loops over every cell; the two lists hold the rows that are not skipped and longer than the limits."""
    lengths = np.asarray(lengths, dtype=np.int64)
    live = np.ones(len(lengths), bool) if skip is None else np.asarray(skip) == 0
    lds = lds_limit or DEFAULT_LDS_ROW_LIMIT
    return len(lengths), int((live & (lengths > wave_limit(lds_limit)) & (lengths <= lds)).sum()), int((live & (lengths > lds)).sum())


def ingest_second_trips(lengths, skip, lds_limit):
    """The rows each of the three kernels serves in a second or later trip of a block."""
    wave, lds, glob = ingest_rows_per_kernel(lengths, skip, lds_limit)
    return max(0, wave - WAVE_BLOCKS), max(0, lds - LDS_BLOCKS), max(0, glob - GLOBAL_BLOCKS)


def sums_in_parallel(values):
    """The rule of ingestRow for a row's values (float32, zeros dropped first)."""
    kept = np.asarray(values, dtype=np.float32)
    kept = kept[kept != 0]
    if len(kept) == 0:
        return True
    if not np.isfinite(kept).all() or (kept < 0).any() or (kept != np.trunc(kept)).any():
        return False
    largest = int(kept.max())
    return largest * largest * len(kept) <= 1 << 52


# ---- the walk of one line, restated: closers, and what the stage does ----
def closers_of(line, separators=","):
    """The positions, relative to the line's begin, of the bytes that end a field of the line (without its line end): the
    separators outside quotes, and the line's end."""
    out, in_quote = [], False
    for i, byte in enumerate(line):
        if byte == 0x22:
            in_quote = not in_quote
        elif chr(byte) in separators and not in_quote:
            out.append(i)
    return out + [len(line)]


def stage_flushes(emitter_positions, staged=0):
    """emitter_positions: the closer positions (relative to the line's begin) of the fields that are decided with a value.
    -> (the (staged, emitters) of every step that flushes mid-line, staged behind the line)."""
    per_step = {}
    for p in emitter_positions:
        per_step[p // 64] = per_step.get(p // 64, 0) + 1
    flushes = []
    for step in sorted(per_step):
        if staged + per_step[step] > K_STAGED:
            flushes.append((staged, per_step[step]))
            staged = 0
        staged += per_step[step]
    return flushes, staged


# ---- C1: the stage flushes mid-kernel ----
C1_TILE = 256
C1_COLUMNS = 2000


DEFERRED_FIELD = "16777217"                                  # a float midpoint.  ("0.1" is decided: one digit, one exact division.)


def c1_wide(lines=3, columns=C1_COLUMNS, kept_every_third_out=False, deferred_every_fifth=False):
    """(a) / (c): `lines` lines of `columns` non-zero integers behind a name.  -> (text, expected tokens, kept)."""
    rows = []
    for r in range(lines):
        fields = []
        for i in range(columns):
            fields.append(DEFERRED_FIELD if deferred_every_fifth and i % 5 == 4 else str(1 + (7 * i + 13 * r) % 997))
        rows.append("gene%d," % r + ",".join(fields))
    kept = [NONE] + [NONE if kept_every_third_out and i % 3 == 2 else i for i in range(columns)]
    return ("\n".join(rows) + "\n").encode(), columns + 1, kept


C1B_FIELDS = 700
# (decided counts of the line, "0" fields among the first 511): the fields are one byte each behind a one-byte name, so the
# separators stand at the odd offsets, step k closes the fields 32 k .. 32 k + 31, and step 16 meets 511 minus the zeros staged.
C1B_LINES = [(512, 0), (513, 0), (511, 0), (512, 0), (513, 0), (575, 21), (576, 11), (577, 0), (575, 0), (576, 21), (577, 11),
             (575, 11), (576, 0), (577, 21)]


def c1b_line(decided, zeros):
    """One line of C1B_FIELDS one-byte fields: `zeros` of the fields 1 .. 511 are "0" (spread out), the fields 512 .. 543 are
    all non-zero where the count allows, and behind them as many non-zero ones as the count still needs."""
    fields = ["0"] * (C1B_FIELDS + 1)
    zero_at = set(1 + (i * 511) // max(zeros, 1) for i in range(zeros))
    assert len(zero_at) == zeros
    placed = 0
    for i in range(1, C1B_FIELDS + 1):
        if placed == decided:
            break
        if i <= 511 and i in zero_at:
            continue
        fields[i] = str(1 + i % 9)
        placed += 1
    assert placed == decided
    fields[0] = "g"
    return ",".join(fields)


def c1_marks():
    """(b) -> (text, expected tokens, kept, the decided counts per line)."""
    text = "".join(c1b_line(decided, zeros) + "\n" for decided, zeros in C1B_LINES).encode()
    return text, C1B_FIELDS + 1, [NONE] + list(range(C1B_FIELDS)), [decided for decided, _ in C1B_LINES]


# ---- C2: the 64-byte step of the line walk ----
C2_POSITIONS = (62, 63, 64, 65, 127, 128, 129)
C2_LENGTHS = (63, 64, 65, 127, 128, 129, 191, 192)
C2_TILES = (0, 48)
C2_COLUMNS = 100
C2_ORDINARY = (b"p,1,2\n", b"pq,1,2\n", b"pqr,10,2\n")


def c2_base(length):
    """`length` bytes of short numeric fields behind a name."""
    pattern = b"12,345,6,7089,"
    return bytearray((b"g," + pattern * (length // len(pattern) + 1))[:length])


def c2_lines():
    """-> list of (what, line bytes without the line feed)."""
    out = []
    for p in C2_POSITIONS:
        line = c2_base(210)
        line[p - 1:p + 2] = b"5,7"
        out.append(("a separator at %d" % p, bytes(line)))
        for close in (1, 2, 70):
            line = c2_base(210)
            line[p - 1] = ord(",")
            line[p] = line[p + close] = ord('"')
            if close == 2:
                line[p + 1] = ord("8")
            line[p + close + 1] = ord(",")
            out.append(("a quote at %d that closes at +%d" % (p, close), bytes(line)))
        line = c2_base(210)
        line[p - 3:p + 4] = b',"3,4",'
        out.append(("a quoted separator at %d" % p, bytes(line)))
        line = c2_base(p)
        line[p - 2:p] = b",7"
        out.append(("a carriage return at %d" % p, bytes(line) + b"\r"))
    out.append(("a field from before 64 to behind 192", b"g,12," + b"7" * 200 + b",5"))
    out.append(("a quoted field from before 64 to behind 192", b"g,12,3,\"" + b"7,8" * 70 + b"\",5"))
    for length in C2_LENGTHS:
        line = c2_base(length)
        line[length - 3:length] = b"1,7"
        out.append(("%d bytes, a decided field last" % length, bytes(line)))
        line[length - 3:length] = b"41,"
        out.append(("%d bytes, an empty field last" % length, bytes(line)))
    return out


def c2_text():
    """Every line behind an ordinary one whose length moves the begin.  -> (text, expected tokens, kept, [(what, begin, end)])."""
    text, where = b"", []
    for i, (what, line) in enumerate(c2_lines()):
        text += C2_ORDINARY[i % len(C2_ORDINARY)]
        end = len(text) + len(line)
        where.append((what, len(text), end - 1 if line.endswith(b"\r") else end))
        text += line + b"\n"
    return text, C2_COLUMNS, [NONE] + list(range(C2_COLUMNS - 1)), where


# ---- C3: second trips of the grid-stride loops ----
C3_LINES = 70000
C3_WIDE_LINES, C3_WIDE_COLUMNS = 4500, 300
C3_TILE_LINES, C3_TILE = 15000, 16


def c3_lines():
    """(a) -> (text, expected tokens, kept)."""
    return b"a,1\n" * C3_LINES, 2, [NONE, 0]


def c3_wide_tail():
    """(b): the last lines hold 300 non-zero kept columns.  The waves that take them took an "a,1" line first."""
    wide = ("w," + ",".join(str(1 + i % 9) for i in range(C3_WIDE_COLUMNS)) + "\n").encode()
    return b"a,1\n" * (C3_LINES - C3_WIDE_LINES) + wide * C3_WIDE_LINES, C3_WIDE_COLUMNS + 1, [NONE] + list(range(C3_WIDE_COLUMNS))


C3_LATE_LINES, C3_LATE_COLUMNS = 8, 600


def c3_late_flush():
    """(b) at the width of C1, beyond the issue's list: 65 536 "a,1" lines, then 8 lines of 600 non-zero kept columns.  The waves
    that take those have one count staged from their first line, and flush it mid-line."""
    wide = ("w," + ",".join(str(1 + i % 9) for i in range(C3_LATE_COLUMNS)) + "\n").encode()
    return b"a,1\n" * 65536 + wide * C3_LATE_LINES, C3_LATE_COLUMNS + 1, [NONE] + list(range(C3_LATE_COLUMNS))


def c3_tiles():
    """(c) -> (text, expected tokens, kept)."""
    return (b"abcdefgh,1" + b",0" * 30 + b"\n") * C3_TILE_LINES, 32, [NONE] + list(range(31))


# ---- C4: numeric fields ----
C4_TILE = 64
C4_COUNT = 20000


def c4_plain(rng, count=C4_COUNT):
    """1 to 19 random digits; a point at a random place (0.6); an exponent e|E, optional sign, 0 to 25 (0.3); a sign (0.2);
    blanks around the field (0.2)."""
    fields = []
    for _ in range(count):
        digits = "".join(rng.choice("0123456789") for _ in range(rng.randint(1, 19)))
        if rng.random() < 0.6:
            at = rng.randint(0, len(digits))
            digits = digits[:at] + "." + digits[at:]
        if rng.random() < 0.3:
            digits += rng.choice("eE") + rng.choice(["", "+", "-"]) + str(rng.randint(0, 25))
        if rng.random() < 0.2:
            digits = rng.choice("+-") + digits
        if rng.random() < 0.2:
            digits = rng.choice([" ", "\t", "  "]) + digits + rng.choice([" ", "\t", " \t"])
        fields.append(digits)
    return fields


def decimal_of(numerator, fraction_digits):
    """numerator / 10^fraction_digits written out, at least one digit on each side of the point."""
    digits = str(numerator).rjust(fraction_digits + 1, "0")
    return digits[:len(digits) - fraction_digits] + "." + digits[len(digits) - fraction_digits:] if fraction_digits else digits


def c4_midpoints(rng, count=C4_COUNT):
    """Floats f with 2^17 <= f < 2^24; the exact decimal of the midpoint of f and its successor (a multiple of 2^-7: at most 8
    digits before the point and 7 behind it), a third each as it is, one unit of its last digit lower, and one higher.
    -> list of (field, "midpoint" | "neighbour")."""
    out = []
    for i in range(count):
        bits = rng.randint(0x48000000, 0x4b7fffff)
        exponent, mantissa = (bits >> 23) - 127, (bits & 0x7fffff) | 0x800000
        assert 17 <= exponent <= 23
        middle_128 = (2 * mantissa + 1) << (exponent - 23 + 6)                 # the midpoint in units of 2^-7: an integer
        numerator, fraction_digits = middle_128 * 5 ** 7, 7                     # ... and in units of 10^-7
        while numerator % 10 == 0:
            numerator //= 10
            fraction_digits -= 1
        assert fraction_digits >= 1
        shift = (0, -1, 1)[i % 3]
        field = decimal_of(numerator + shift, fraction_digits)
        assert len(field.replace(".", "")) <= 15
        out.append((field, "neighbour" if shift else "midpoint"))
    return out


# By hand.  No decimal of at most 19 significant digits with |q| <= 22 that the rule decides lies near 0x1p-126, 0x1p127 or
# FLT_MAX (m <= 2^53 and |q| <= 22 bound a decided value to [1e-22, 9.007e37]), so their neighbours are here as the fields that
# must be deferred, next to the ends of the decided range itself.
C4_EDGES = [
    "1.17549435e-38", "1.17549421e-38", "1.1754944e-38", "1.1754943508222875e-38", "1.70141183e38", "1.7014118e38", "1.7014119e38",
    "1.7014118346046923e38", "3.40282347e38", "3.4028235e38", "3.4028236e38", "170141183460469231731687303715884105728",
    "9007199254740992e22", "9007199254740991e22", "9007199254740993e22", "1e-22", "0.0000000000000000000001", "0.0000000000000000000009",
    "0" * 30 + "12", "0" * 31 + "12", "0" * 16 + "9007199254740992", "1234567.890123450000000000000000", "0." + "0" * 21 + "123456789",
    "0." + "0" * 22 + "123456789", " " * 5 + "0" * 29 + "77" + " " * 5, "\t" * 10 + "0" * 28 + "7.5", "0" * 29 + "77" + " " * 10,
    "000" + "1234567890123456789", "0001234567890123456", "0.0001234567890123456789", "0000000000001234567.890123456789",
    "1234567890123456789", "12345678901234567890", "1000000000000000000", "10000000000000000000", "999999999999999999", "123456789012345678",
    "9007199254740992", "9007199254740993", "9007199254740991", "9007199254740994", "900719925474099.2", "9007199254740.993",
    "1e22", "1e23", "1e-22", "1e-23", "12345e22", "1.5e23", "15e21", "0.5e-21", "0.5e-22", "9.5e22", "95e-23", "9.5e-22", "8388608.5e0",
    "1e0022", "1e00022", "1e-0022", "1e-00022", "1e9999", "1e99999", "1e-9999", "5e0000", "5e00000", "7e+0001", "7e-0001",
    "-0.0", "+0", "0e5", ".0", "0", "0.", "-0", "00", "0.00", "-.0e-3", "+0.", "-0.", "0e0", "0.e1", "+.0", "-0e22", "0e23", "0e9999",
]


def c4_text(fields):
    """Three columns per line, the field first, in the middle and last by turns.  -> (text, expected tokens, kept)."""
    lines = []
    for i, field in enumerate(fields):
        lines.append((field + ",1,2", "1," + field + ",2", "1,2," + field)[i % 3])
    return ("\n".join(lines) + "\n").encode(), 3, [0, 1, 2]


def c4_field_of_line(fields):
    """-> list of (line, column) of the fuzzed field."""
    return [(i, i % 3) for i in range(len(fields))]


# ---- C5: bytes ----
C5_ALPHABET = [bytes([b]) for b in b"0123456789" * 3 + b",,,,,," + b"\n\n" + b"\"\r .e-+\\x"] + [
    b"\0", b"\x0b", b"\x0c", b"\t", b"\x80", b"\xc3\xa9", b"\xff"] * 2
C5_TILES = (16, 32, 80)


def c5_texts(rng, count=40, alphabet=C5_ALPHABET, longest=400):
    """-> list of (text, expected tokens, kept, tile, misalignment): the generator of test_random_texts over bytes."""
    out = []
    for _ in range(count):
        tile = rng.choice(C5_TILES)
        text = b"".join(rng.choice(alphabet) for _ in range(rng.randint(1, longest)))[:longest]
        columns = rng.randint(1, 6)
        kept = [rng.choice([NONE, i]) for i in range(columns)]
        out.append((text, columns, kept, tile, rng.randint(0, 15)))
    return out


def c5_all():
    out = c5_texts(random.Random(23))
    out.append((b"\xff" * 333, 2, [0, 1], 16, 3))
    out.append((b"\0" * 333, 2, [0, 1], 32, 11))
    return out


# ---- C6: csvSessionFinish through the facade ----
C6_GENE_LINES = (1, 2, 3, 4, 5, 255, 256, 257)
C6_CELLS = (1, 2, 3, 4, 5)
C6_CHUNK_BYTES = (1 << 30, 64)
C6_DEFERRED = (DEFERRED_FIELD, "\"8\"")                      # the device defers both, the host's strtof resolves them


def c6_file(gene_lines, cells, number, kind="mixed"):
    """One expression file and its meta data file.  `number` rotates what the issue rotates: the meta data file keeps 1, 2 or
    all of the cells; where more than one cell is kept, one kept cell's column is all "0", first, in the middle or last among
    the kept cells (a single kept cell cannot be all "0" and hold a deferred field: there the kept cell holds counts, and the
    all-"0" kind below is the single kept cell without any).  kind: "mixed" (decided and deferred counts), "deferred" (every
    non-zero field is one the device defers), "zero" (every count is "0").
    -> dict(expression, meta, kept (cell names in the order of their ids), empty (the all-"0" kept cell or None))."""
    names = ["c%d" % i for i in range(cells)]
    keep = min((1, 2, cells)[number % 3], cells)
    rotated = names[number % cells:] + names[:number % cells]
    meta_order = rotated[:keep][::-1] if number % 2 else rotated[:keep]       # not the file's column order
    kept = sorted(meta_order, key=names.index)                                # the cells get their ids in column order
    empty = None
    if len(kept) > 1:
        empty = kept[(0, len(kept) // 2, len(kept) - 1)[(number // 3) % 3]]
    rng = random.Random(1000 * gene_lines + 10 * cells + number)
    lines = ["gene," + ",".join(names)]
    for g in range(gene_lines):
        fields = []
        for name in names:
            if kind == "zero" or name == empty:
                fields.append("0")
            elif kind == "deferred":
                fields.append(rng.choice(("0", DEFERRED_FIELD, "\"8\"", "0.30000001192092896", "\"12\"")))
            else:
                fields.append(rng.choice(("0", "0", "3", "17", "2.5", "1e2", "250")))
        lines.append("G%d," % g + ",".join(fields))
    if kind != "zero":                                        # at least one deferred field, in a kept column that is not the empty one
        column = names.index([n for n in kept if n != empty][0])
        row = 1 + rng.randrange(gene_lines)
        fields = lines[row].split(",")
        fields[1 + column] = C6_DEFERRED[number % 2]
        lines[row] = ",".join(fields)
    meta = "Cell,Organ\n" + "".join("%s,organ%d\n" % (name, i) for i, name in enumerate(meta_order))
    return {"expression": "\n".join(lines) + "\n", "meta": meta, "kept": kept, "empty": empty, "kind": kind}


def c6_files(gene_lines):
    """The files of one gene line count: every cell count, and with 5 cells the two special kinds."""
    out = [c6_file(gene_lines, cells, C6_GENE_LINES.index(gene_lines) + i) for i, cells in enumerate(C6_CELLS)]
    out.append(c6_file(gene_lines, 5, C6_GENE_LINES.index(gene_lines) + 2, "deferred"))
    out.append(c6_file(gene_lines, 4, C6_GENE_LINES.index(gene_lines), "zero"))
    return out


# ---- the ingest cases ----
GENES = 9973                                                  # a prime: start + j * step (mod GENES) gives distinct indices


def gene_map(genes=GENES):
    """Not monotone, injective: the store already had some of the genes, in another order."""
    return np.random.default_rng(5).permutation(genes + 500).astype(np.uint32)[:genes]


def rows_from_lengths(lengths, rng, kinds, genes=GENES):
    """Distinct indices per row in a scattered order, no zero value.  kinds: per row 0 integers (1 .. 59), 1 fractions (magnitudes
    apart: the double sums depend on the order).  -> (indptr, indices, values), vectorised."""
    lengths = np.asarray(lengths, dtype=np.int64)
    assert lengths.max(initial=0) <= genes
    indptr = np.concatenate([[0], np.cumsum(lengths)]).astype(np.uint64)
    total = int(indptr[-1])
    row = np.repeat(np.arange(len(lengths)), lengths)
    within = np.arange(total, dtype=np.int64) - np.repeat(indptr[:-1].astype(np.int64), lengths)
    start, step = rng.integers(0, genes, len(lengths)), rng.integers(1, genes, len(lengths))
    indices = ((start[row] + within * step[row]) % genes).astype(np.uint32)
    integers = rng.integers(1, 60, total).astype(np.float32)
    fractions = (rng.random(total) * 10.0 ** rng.integers(-6, 7, total)).astype(np.float32) + np.float32(1e-3)
    values = np.where(np.asarray(kinds)[row] == 0, integers, fractions).astype(np.float32)
    return indptr, indices, values


def plant_duplicates(indptr, indices, rows, rng):
    """In each of `rows` (at least 2 entries long) one entry takes the index of another entry of the row."""
    starts, lengths = indptr[rows].astype(np.int64), (indptr[np.asarray(rows) + 1] - indptr[rows]).astype(np.int64)
    assert (lengths >= 2).all()
    first = rng.integers(0, lengths)
    second = (first + 1 + rng.integers(0, lengths - 1)) % lengths
    indices[starts + second] = indices[starts + first]


def planted_rows(count, short, long, seed, duplicates):
    """I1 / I2: row i is, by i mod 4: 0 a row of a random length that holds a duplicated gene (clean when `duplicates` is off),
    1 clean and `short`, 2 clean and of a random length, 3 clean and `long`; integers and fractions alternate.
    -> (indptr, indices, values, dict(duplicate rows, short rows, long rows))."""
    rng = np.random.default_rng(seed)
    kind = np.arange(count) % 4
    lengths = np.where(kind == 1, short, np.where(kind == 3, long, rng.integers(short, long + 1, count)))
    indptr, indices, values = rows_from_lengths(lengths, rng, (np.arange(count) // 2) % 2)
    plants = {"duplicate": np.nonzero(kind == 0)[0], "short": np.nonzero(kind == 1)[0], "long": np.nonzero(kind == 3)[0]}
    if duplicates:
        plant_duplicates(indptr, indices, plants["duplicate"], rng)
    return indptr, indices, values, plants


I1_LIMIT, I1_ROWS, I1_SHORT, I1_LONG = 16, 1100, 17, 60
I2_LIMIT, I2_ROWS, I2_SHORT, I2_LONG = 600, 4200, 513, 600


def i1(duplicates):
    return planted_rows(I1_ROWS, I1_SHORT, I1_LONG, 31, duplicates)


def i2(duplicates):
    return planted_rows(I2_ROWS, I2_SHORT, I2_LONG, 32, duplicates)


I3_ROWS, I3_EDGE = (1 << 20) + 70, 70


def i3(variant):
    """Rows 0 .. 69: 512 entries; rows 2^20 .. 2^20 + 69, the same blocks' second rows: 3 entries; all others 0 to 2.
    "first": the even rows of the first 70 hold a duplicated gene, the last 70 are clean (a stale sU32[8] or buffer tail of the
    block's first row would show in them).  "swapped": the first 70 are clean and the last 70 hold the duplicates.  "clean": no
    duplicate anywhere, so the fill runs.  -> (indptr, indices, values, duplicate rows)."""
    rng = np.random.default_rng(33)
    lengths = rng.integers(0, 3, I3_ROWS)
    lengths[:I3_EDGE] = WAVE_ROW_LIMIT
    lengths[-I3_EDGE:] = 3
    indptr, indices, values = rows_from_lengths(lengths, rng, np.arange(I3_ROWS) % 2)
    duplicate = {"first": np.arange(0, I3_EDGE, 2), "swapped": np.arange(I3_ROWS - I3_EDGE, I3_ROWS),
                 "clean": np.zeros(0, dtype=np.int64)}[variant]
    if len(duplicate):
        plant_duplicates(indptr, indices, duplicate, rng)
    return indptr, indices, values, duplicate


# I4: status 3.  -> per row (entries, skipped, expected status); the kept count is the number of values that are not zero.
def i4_rows(index_count):
    rng = np.random.default_rng(34)

    def clean(n):
        index = rng.choice(index_count, size=n, replace=False)
        return [(int(i), float(v)) for i, v in zip(index, rng.integers(1, 60, n))]
    good = clean(30)
    at_count = clean(20)
    at_count[7] = (index_count, 4.0)
    all_ones = clean(20)
    all_ones[0] = (0xffffffff, 4.0)
    on_zero = clean(20)
    on_zero[5] = (index_count + 3, 0.0)
    on_zero[11] = (0xffffffff, -0.0)
    negative = clean(20)
    negative[3] = (index_count, 2.0)
    negative[9] = (negative[9][0], -1.0)
    negative_itself = clean(20)
    negative_itself[4] = (index_count + 1, -3.0)
    duplicate = clean(20)
    duplicate[15] = (index_count + 1, 2.0)
    duplicate[2] = (duplicate[8][0], 6.0)
    skipped = clean(20)
    skipped[1] = (index_count, 2.0)
    long = clean(700)
    long[-1] = (index_count, 9.0)
    return [(good, 0, 0), (at_count, 0, 3), (all_ones, 0, 3), (on_zero, 0, 0), (negative, 0, 3), (negative_itself, 0, 3),
            (duplicate, 0, 3), (skipped, 1, 0), (long, 0, 3), (good, 0, 0)]


# I5: the fill's toc check
I5_LENGTHS = (40, 300, 700, 9000)


def i5():
    """Rows for the wave, the LDS and (9000, or everything at limit 16) the global-memory kernel, a few zeros in each.
    -> (indptr, indices, values)."""
    rng = np.random.default_rng(35)
    indptr, indices, values = rows_from_lengths(I5_LENGTHS, rng, [0, 1, 0, 1])
    values[indptr[:-1].astype(np.int64) + 5] = 0.0
    values[indptr[1:].astype(np.int64) - 2] = -0.0
    return indptr, indices, values


def i5_moved_tocs(toc):
    """Every inner boundary moved by one, down and up: toc[0] and toc[n] stay and the sequence stays non-decreasing, so every
    [toc[r], toc[r + 1]) lies inside the data buffer."""
    out = []
    for boundary in range(1, len(toc) - 1):
        for shift in (-1, 1):
            moved = np.array(toc, dtype=np.int64)
            moved[boundary] += shift
            assert moved[0] == 0 and moved[-1] == toc[-1] and (np.diff(moved) >= 0).all()
            out.append((boundary, shift, moved.astype(np.uint64)))
    return out


# I6: largest^2 * kept at 2^52
I6_GENES = 70001


def i6_rows():
    """-> list of (what, values, parallel sums expected).  2^26 + 4 is no float (the spacing there is 8): float32 rounds it to 2^26,
    so its successor 2^26 + 8 stands next to it as the first single value above the switch."""
    rng = np.random.default_rng(36)
    large = lambda n: rng.integers(2 ** 24 + 1, 2 ** 26, n).astype(np.float32)
    among = lambda special: np.concatenate([large(4), np.float32([special]), large(4)])
    four = large(400)
    nine = large(9)
    return [
        ("a single 2^26", np.float32([2 ** 26]), True),
        ("four of 2^25", np.float32([2 ** 25] * 4), True),
        ("five of 2^25", np.float32([2 ** 25] * 5), False),
        ("2^12 of 2^20", np.full(1 << 12, 2 ** 20, np.float32), True),
        ("2^12 + 1 of 2^20", np.full((1 << 12) + 1, 2 ** 20, np.float32), False),
        ("2^16 of 2^18", np.full(1 << 16, 2 ** 18, np.float32), True),
        ("2^16 + 1 of 2^18", np.full((1 << 16) + 1, 2 ** 18, np.float32), False),
        ("2^16 of 2^18 and a 3", np.concatenate([np.full((1 << 16) - 1, 2 ** 18, np.float32), np.float32([3])]), True),
        ("2^26 + 4 as a float", np.float32([2 ** 26 + 4]), True),
        ("the float above 2^26", np.float32([2 ** 26 + 8]), False),
        ("400 above 2^24", four, False), ("400 above 2^24, reversed", four[::-1].copy(), False),
        ("9 above 2^24", nine, False), ("9 above 2^24, reversed", nine[::-1].copy(), False),
        ("inf among large integers", among(np.inf), False), ("nan among large integers", among(np.nan), False),
        ("-0.0 among large integers", among(-0.0), False),
        ("-0.0 among four of 2^25", np.float32([2 ** 25, 2 ** 25, -0.0, 2 ** 25, 2 ** 25]), True),
    ]


def i6():
    """-> (indptr, indices, values, gene map): distinct indices in a scattered order for every row."""
    rng = np.random.default_rng(37)
    rows = i6_rows()
    lengths = [len(values) for _, values, _ in rows]
    indptr, indices, _ = rows_from_lengths(lengths, rng, np.zeros(len(rows), int), genes=I6_GENES)
    return indptr, indices, np.concatenate([values for _, values, _ in rows]), gene_map(I6_GENES)


# ---- the draws of tools/fuzz_parity.py ----
def draw_csv_parse(rng, seed=None):
    """rng: numpy Generator (the draw is a function of the one seed taken from it, or of `seed`).  Random structure (quotes, blanks, carriage returns, empty and wrong lines) and numeric fields (the
    generators of C4), a tile size, a misalignment and a kept subset.  -> dict(text, separators, columns, kept, tile, misalign, seed)."""
    seed = int(rng.integers(1 << 30)) if seed is None else seed
    r = random.Random(seed)
    columns = r.choice([1, 2, 3, 7, 33, 70, 300, 1200])
    separators = r.choice([",", ",", ";\t", ",;|"])
    numbers = c4_plain(r, 60) + [field for field, _ in c4_midpoints(r, 30)] + r.sample(C4_EDGES, 10)
    lines = []
    for _ in range(r.choice([1, 3, 20, 200]) if columns <= 70 else r.choice([1, 3, 9])):
        u = r.random()
        if u < 0.03:
            lines.append(r.choice(["", "\r", "x\\n,1", "\"", ",,"]))
            continue
        count = columns if u < 0.95 else max(1, columns + r.choice([-1, 1]))
        fields = []
        for _ in range(count):
            v = r.random()
            fields.append("0" if v < 0.5 else str(r.randint(1, 999)) if v < 0.8 else r.choice(numbers) if v < 0.95 else
                          r.choice(["", " ", "\"7\"", "\"%s\"" % separators[0], "x", "\"a%sb\"" % separators[-1], "\xe9", "1\0"]))
        lines.append("".join(f + r.choice(separators) for f in fields[:-1]) + fields[-1] + r.choice(["", "", "", "\r"]))
    text = "\n".join(lines) + r.choice(["\n", "\n", ""])
    kept_mode = r.choice(["all", "third", "random", "none"])
    kept = [{"all": i, "third": i if i % 3 else NONE, "random": r.choice([NONE, i]), "none": NONE}[kept_mode] for i in range(columns)]
    return dict(text=text.encode("latin-1"), separators=separators, columns=columns, kept=kept, tile=r.choice([0, 16, 48, 64, 256, 4096]),
                misalign=r.randint(0, 15), seed=seed)


def draw_ingest(rng, seed=None):
    """rng: numpy Generator (the draw is a function of the one seed taken from it, or of `seed`).  Row lengths around 512 and the LDS limit, value kinds, entry orders, duplicates, negatives, zeros
    and skip flags.  -> dict(lds_limit, indptr, indices, values, skip, seed)."""
    seed = int(rng.integers(1 << 30)) if seed is None else seed
    r = np.random.default_rng(seed)
    lds_limit = int(r.choice([0, 16, 128, 600, 1000]))
    limit = lds_limit or DEFAULT_LDS_ROW_LIMIT
    edges = [0, 1, 2, 63, 64, 65, wave_limit(lds_limit) - 1, wave_limit(lds_limit), wave_limit(lds_limit) + 1, limit - 1, limit, limit + 1]
    rows = int(r.choice([1, 5, 40, 300, 1500]))
    lengths = np.where(r.random(rows) < 0.5, r.choice(edges, rows), r.integers(0, 40, rows))
    if rows >= 300:
        lengths = np.minimum(lengths, 700)
    lengths = np.minimum(lengths, GENES)
    kind = r.choice(["integers", "fractions", "mixed", "large"])
    indptr, indices, values = rows_from_lengths(lengths, r, {"integers": np.zeros(rows, int), "fractions": np.ones(rows, int),
                                                             "mixed": r.integers(0, 2, rows), "large": np.zeros(rows, int)}[kind])
    if kind == "large":
        values = r.integers(2 ** 24 + 1, 2 ** 26, len(values)).astype(np.float32)
    order = r.choice(["scattered", "ascending", "descending"])
    if order != "scattered":
        genes = gene_map()
        for row in range(rows):
            a, b = int(indptr[row]), int(indptr[row + 1])
            by_gene = np.argsort(genes[indices[a:b]], kind="stable")
            indices[a:b] = indices[a:b][by_gene if order == "ascending" else by_gene[::-1]]
    values[r.random(len(values)) < r.choice([0.0, 0.0, 0.1, 0.5])] = 0.0
    long_enough = np.nonzero(lengths >= 2)[0]
    if len(long_enough) and r.random() < 0.4:
        plant_duplicates(indptr, indices, r.choice(long_enough, size=min(len(long_enough), 3), replace=False), r)
    if len(values) and r.random() < 0.3:
        values[r.integers(0, len(values), 2)] = np.float32([-1.0, np.nan])[r.integers(0, 2, 2)]
    skip = (r.random(rows) < 0.2).astype(np.uint8) if r.random() < 0.5 else None
    return dict(lds_limit=lds_limit, indptr=indptr, indices=indices, values=values, skip=skip, seed=seed, kind=str(kind), order=str(order))
