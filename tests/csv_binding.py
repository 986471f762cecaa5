"""ctypes binding of tests/native/em2_csv_restatement.cpp (the reference's tokenizer, addCells and addCellMetaData with its
containers and loops, as a sequence of calls or an error text) and what the CSV tests share: an independent Python tokenizer,
the exactness rule of em2_dev_csv_parse stated in Python, a Python model of that entry's outputs, the entry itself with
guarded output buffers, and the replay of a call sequence through the existing methods.  Compiled with g++ at first use.
Test infrastructure only."""
import ctypes
import functools
import os
import struct
import subprocess

import numpy as np

from expressionmatrix2_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE_DIR = os.path.join(ROOT, "tests", "native")
SOURCE = os.path.join(NATIVE_DIR, "em2_csv_restatement.cpp")
GOLDEN = os.path.join(ROOT, "tests", "golden", "csv_reference")
FILL = 0x5a
GUARD = 64
NONE = 0xffffffff
OK, EMPTY, TOKEN_COUNT, ESCAPE = 0, 1, 2, 3
BLANKS = " \t\n\v\f\r"
MAX_FIELD_BYTES = 32

c = ctypes


@functools.lru_cache(maxsize=None)
def load():
    build = os.path.join(NATIVE_DIR, "build")
    os.makedirs(build, exist_ok=True)
    path = os.path.join(build, "libem2csvrestatement.so")
    if not os.path.exists(path) or os.path.getmtime(path) < os.path.getmtime(SOURCE):
        tmp = path + ".%d.tmp" % os.getpid()
        cmd = ["g++", "-std=c++11", "-O2", "-fPIC", "-shared", "-o", tmp, SOURCE]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError("csv restatement build failed: " + r.stderr)
        os.replace(tmp, path)
    lib = ctypes.CDLL(path)
    u64p = c.POINTER(c.c_uint64)
    lib.em2r_csv_tokenize.argtypes = [c.c_char_p, c.c_char_p, c.c_uint64, c.c_int, u64p]
    lib.em2r_csv_add_cells.argtypes = [c.c_char_p, c.c_char_p, c.c_char_p, c.c_char_p, c.c_char_p, c.c_uint64, u64p]
    lib.em2r_csv_add_cell_meta_data.argtypes = [c.c_char_p, c.c_char_p, c.c_uint64, u64p]
    for f in (lib.em2r_csv_tokenize, lib.em2r_csv_add_cells, lib.em2r_csv_add_cell_meta_data):
        f.restype = c.c_void_p
    return lib


def _fields(pointer, n):
    raw = ctypes.string_at(pointer, n.value)
    assert raw == b"" or raw.endswith(b"\0")
    return [f.decode("utf-8", "surrogateescape") for f in raw.split(b"\0")[:-1]]


def _pack(strings):
    return b"".join(s.encode("utf-8", "surrogateescape") + b"\0" for s in strings)


class Failure(Exception):
    """The error text the reference would throw."""


def restated_tokenize(separators, line, trim):
    """-> list of tokens; raises Failure(text)."""
    n = c.c_uint64(0)
    raw = line.encode("utf-8", "surrogateescape") if isinstance(line, str) else line
    fields = _fields(load().em2r_csv_tokenize(separators.encode(), raw, len(raw), 1 if trim else 0, ctypes.byref(n)), n)
    if fields[:1] == ["E"]:
        raise Failure(fields[1])
    assert fields[0::2] == ["T"] * (len(fields) // 2)
    return fields[1::2]


def _calls(fields):
    """The call sequence of the restatement's output -> list of ("G", name) / ("C", pairs, counts) / ("M", cell, name, value)."""
    if fields[:1] == ["E"]:
        raise Failure(fields[1])
    calls, at = [], 0
    while at < len(fields):
        kind = fields[at]
        if kind == "G":
            calls.append(("G", fields[at + 1]))
            at += 2
        elif kind == "M":
            calls.append(("M", fields[at + 1], fields[at + 2], fields[at + 3]))
            at += 4
        else:
            assert kind == "C"
            pair_count = int(fields[at + 1])
            at += 2
            pairs = [(fields[at + 2 * i], fields[at + 2 * i + 1]) for i in range(pair_count)]
            at += 2 * pair_count
            count_count = int(fields[at])
            at += 1
            counts = [(fields[at + 2 * i], struct.unpack("<f", struct.pack("<I", int(fields[at + 2 * i + 1], 16)))[0])
                      for i in range(count_count)]
            at += 2 * count_count
            calls.append(("C", pairs, counts))
    return calls


def restated_add_cells(expression_file, expression_separators, meta_data_file, meta_data_separators, additional=()):
    n = c.c_uint64(0)
    packed = _pack([s for pair in additional for s in pair])
    return _calls(_fields(load().em2r_csv_add_cells(expression_file.encode(), expression_separators.encode(), meta_data_file.encode(),
                                                    meta_data_separators.encode(), packed, len(packed), ctypes.byref(n)), n))


def restated_add_cell_meta_data(meta_data_file, cell_names):
    n = c.c_uint64(0)
    packed = _pack(cell_names)
    return _calls(_fields(load().em2r_csv_add_cell_meta_data(meta_data_file.encode(), packed, len(packed), ctypes.byref(n)), n))


def replay(e, calls):
    """The calls through the existing methods of an ExpressionMatrix."""
    for call in calls:
        if call[0] == "G":
            e.addGene(call[1])
        elif call[0] == "C":
            e.addCell(call[1], call[2])
        else:
            e.setCellMetaData(e.cellIdFromString(call[1]), call[2], call[3])


def product_tokenize(separators, line, trim):
    """em2_csv_tokenize -> list of tokens; raises RuntimeError."""
    lib = capi.load()
    raw = line.encode("utf-8", "surrogateescape") if isinstance(line, str) else line
    count, size = c.c_uint64(0), c.c_uint64(0)
    capi.check(lib.em2_csv_tokenize(separators.encode(), raw, len(raw), 1 if trim else 0, ctypes.byref(count), ctypes.byref(size), None))
    buffer = ctypes.create_string_buffer(max(size.value, 1))
    capi.check(lib.em2_csv_tokenize(separators.encode(), raw, len(raw), 1 if trim else 0, ctypes.byref(count), ctypes.byref(size), buffer))
    tokens = buffer.raw[:size.value].split(b"\0")[:-1]
    assert len(tokens) == count.value
    return [t.decode("utf-8", "surrogateescape") for t in tokens]


# ---- an independent tokenizer: explicit loops over the rules as the issue states them ----

def python_tokenize(separators, line, trim):
    """-> list of tokens; raises Failure("cannot end with escape" / "unknown escape sequence")."""
    if line == "":
        return []
    tokens, token, in_quote, i = [], [], False, 0
    while i < len(line):
        ch = line[i]
        if ch == "\\":
            if i + 1 == len(line):
                raise Failure("cannot end with escape")
            following = line[i + 1]
            if following == "n":
                token.append("\n")
            elif following in ('"', "\\") or following in separators:
                token.append(following)
            else:
                raise Failure("unknown escape sequence")
            i += 2
            continue
        if ch in separators and not in_quote:
            tokens.append("".join(token))
            token = []
        elif ch == '"':
            in_quote = not in_quote
        else:
            token.append(ch)
        i += 1
    tokens.append("".join(token))
    if trim:
        tokens = [t.strip(BLANKS) for t in tokens]
    return tokens


def lines_of(text):
    """getline: (begin, end of the line without its line feed) for every line of the bytes."""
    out, at = [], 0
    while at < len(text):
        nl = text.find(b"\n", at)
        if nl < 0:
            out.append((at, len(text)))
            break
        out.append((at, nl))
        at = nl + 1
    return out


# ---- the exactness rule of em2_dev_csv_parse ----

def decide(field):
    """The field's text (bytes, untrimmed, as it stands between two separators) -> ("skip",), ("value", float32 bits) or
    ("defer",).  Integer arithmetic only, except the one double operation of the rule."""
    if b'"' in field:
        return ("defer",)
    text = field.strip(BLANKS.encode())
    if len(text) == 0 or len(text) > MAX_FIELD_BYTES:
        return ("defer",)
    if text in (b"0", b"0."):
        return ("skip",)
    i, negative = 0, False
    if text[i:i + 1] in (b"+", b"-"):
        negative = text[i:i + 1] == b"-"
        i += 1
    m, significant, fraction_digits, any_digit = 0, 0, 0, False
    while i < len(text) and 48 <= text[i] <= 57:
        any_digit = True
        if m or text[i] != 48:
            significant += 1
            m = m * 10 + text[i] - 48
        i += 1
    if i < len(text) and text[i] == 46:
        i += 1
        while i < len(text) and 48 <= text[i] <= 57:
            any_digit = True
            fraction_digits += 1
            if m or text[i] != 48:
                significant += 1
                m = m * 10 + text[i] - 48
            i += 1
    if not any_digit or significant > 19:
        return ("defer",)
    exponent = 0
    if i < len(text) and text[i] in (101, 69):
        i += 1
        negative_exponent = False
        if i < len(text) and text[i] in (43, 45):
            negative_exponent = text[i] == 45
            i += 1
        digits = 0
        while i < len(text) and 48 <= text[i] <= 57:
            digits += 1
            exponent = exponent * 10 + text[i] - 48
            i += 1
        if digits == 0 or digits > 4:
            return ("defer",)
        if negative_exponent:
            exponent = -exponent
    if i != len(text) or m > 2 ** 53:
        return ("defer",)
    q = exponent - fraction_digits
    if abs(q) > 22:
        return ("defer",)
    d = float(m) * float(10 ** q) if q >= 0 else float(m) / float(10 ** -q)      # exact operands, one rounded operation
    bits = struct.unpack("<Q", struct.pack("<d", d))[0]
    if bits & 0x1fffffff == 0x10000000:
        return ("defer",)
    if d != 0. and not 2. ** -126 <= d <= 2. ** 127:
        return ("defer",)
    value = np.float32(d)                                                          # round to nearest even
    if negative:
        value = -value
    return ("value", int(np.array([value], np.float32).view(np.uint32)[0]))


def strtof_bits(text):
    """libc's strtof of the bytes -> (float32 bits, bytes consumed)."""
    libc = ctypes.CDLL(None)
    libc.strtof.restype = c.c_float
    libc.strtof.argtypes = [c.c_char_p, c.POINTER(c.c_char_p)]
    buffer = ctypes.create_string_buffer(text)
    end = c.c_char_p()
    value = libc.strtof(buffer, ctypes.byref(end))
    consumed = ctypes.cast(end, c.c_void_p).value - ctypes.addressof(buffer)
    return int(np.array([value], np.float32).view(np.uint32)[0]), consumed


# ---- em2_dev_csv_parse: a model of its outputs, and the entry with guards ----

def model_parse(text, separators, expected_tokens, kept_of_column, line_base=0):
    """-> dict(lines: array [n, 6], triples: set of (cell, line, bits), deferred: set of (line, column, begin, end))."""
    table, triples, deferred = [], set(), set()
    for index, (begin, raw_end) in enumerate(lines_of(text)):
        end = raw_end - 1 if raw_end > begin and text[raw_end - 1:raw_end] == b"\r" else raw_end
        line = text[begin:end]
        if b"\\" in text[begin:raw_end]:
            table.append((begin, end, 0, ESCAPE, begin, begin))
            continue
        if raw_end == begin:
            table.append((begin, end, 0, EMPTY, begin, begin))
            continue
        fields, in_quote, start = [], False, 0
        if len(line):
            for i, byte in enumerate(line):
                ch = chr(byte)
                if ch == '"':
                    in_quote = not in_quote
                elif ch in separators and not in_quote:
                    fields.append((start, i))
                    start = i + 1
            fields.append((start, len(line)))
        first = (begin + fields[0][0], begin + fields[0][1]) if fields else (begin, begin)
        table.append((begin, end, len(fields), OK if len(fields) == expected_tokens else TOKEN_COUNT, first[0], first[1]))
        for column, (b, e) in enumerate(fields):
            if column >= expected_tokens or kept_of_column[column] == NONE:
                continue
            kind = decide(line[b:e])
            if kind[0] == "value":
                triples.add((int(kept_of_column[column]), line_base + index, kind[1]))
            elif kind[0] == "defer":
                deferred.add((line_base + index, column, begin + b, begin + e))
    return {"lines": np.array(table, np.uint32).reshape(-1, 6), "triples": triples, "deferred": deferred}


def device_parse(torch, text, separators, expected_tokens, kept_of_column, line_base=0, misalign=0, capacities=None):
    """em2_dev_csv_parse on the bytes, placed `misalign` bytes behind an aligned address; every output buffer is pre-filled
    with 0x5a and has a guard behind it.  -> the dict of model_parse, plus counts."""
    kept = np.ascontiguousarray(kept_of_column, dtype=np.uint32)
    assert len(kept) == expected_tokens
    model = model_parse(text, separators, expected_tokens, kept, line_base)
    lines, triples, deferred = capacities or (len(model["lines"]), len(model["triples"]), len(model["deferred"]))
    holder = torch.zeros(len(text) + misalign + 16, dtype=torch.uint8, device="cuda")
    if len(text):
        holder[misalign:misalign + len(text)] = torch.from_numpy(np.frombuffer(text, np.uint8).copy()).cuda()
    d_kept = torch.from_numpy(kept.view(np.uint8).copy()).cuda()
    sizes = {"lines": 24 * lines, "keys": 8 * triples, "values": 4 * triples, "deferred": 16 * deferred}
    out = {key: torch.full((size + GUARD,), FILL, dtype=torch.uint8, device="cuda") for key, size in sizes.items()}
    counts = (c.c_uint64 * 3)()
    capi.check(capi.load().em2_dev_csv_parse(
        holder.data_ptr() + misalign, len(text), separators.encode(), len(separators), expected_tokens, d_kept.data_ptr(), line_base,
        lines, out["lines"].data_ptr(), triples, out["keys"].data_ptr(), out["values"].data_ptr(), deferred, out["deferred"].data_ptr(),
        counts, None))
    torch.cuda.synchronize()
    host = {key: out[key].cpu().numpy() for key in out}
    for key, size in sizes.items():
        assert (host[key][size:] == FILL).all(), "the guard behind %s was written" % key
    counts = [int(x) for x in counts]
    result = {"counts": counts, "model": model}
    if counts[0] <= lines:
        result["lines"] = host["lines"][:24 * counts[0]].view(np.uint32).reshape(-1, 6).copy()
        n = min(counts[1], triples)
        keys = host["keys"][:8 * n].view(np.uint64)
        bits = host["values"][:4 * n].view(np.uint32)
        result["triples"] = set((int(k) >> 32, int(k) & 0xffffffff, int(b)) for k, b in zip(keys, bits))
        assert len(result["triples"]) == n, "a triple was emitted twice"
        n = min(counts[2], deferred)
        rows = host["deferred"][:16 * n].view(np.uint32).reshape(-1, 4)
        result["deferred"] = set(tuple(int(x) for x in row) for row in rows)
        assert len(result["deferred"]) == n, "a field was deferred twice"
    return result


def assert_parse(torch, text, separators, expected_tokens, kept_of_column, what="", **kw):
    """The entry against the model, all equal: line table, token counts, statuses, first-field ranges, the set of decided
    triples with their bits, the deferred list.  -> the result."""
    got = device_parse(torch, text, separators, expected_tokens, kept_of_column, **kw)
    model = got["model"]
    assert got["counts"] == [len(model["lines"]), len(model["triples"]), len(model["deferred"])], "%s: counts %r" % (what, got["counts"])
    assert np.array_equal(got["lines"], model["lines"]), "%s: the line table differs:\n%r\n%r" % (what, got["lines"], model["lines"])
    assert got["triples"] == model["triples"], "%s: the decided counts differ" % what
    assert got["deferred"] == model["deferred"], "%s: the deferred fields differ" % what
    return got


# the numbers the issue lists, and neighbours
NUMBERS = ["16777217", "16777216", "16777218", "1234567890123456789", "12345678901234567890", "9007199254740992", "9007199254740993",
           "1e22", "1e23", "1e-22", "1e-23", "123e20", "5e-324", "1e-50", ".5", "5.", "+5", "-1", "1E+5", " 7 ", "0.0", "-0", "00", "0", "0.",
           "3abc", "0x10", "inf", "nan", "1e999", "", " ", "1e", "1e+", ".", "-", "+.5e-3", "3.4028235e38", "1.17549435e-38", "0.1", "0.3",
           "2.5", "1.5e3", "33554434", "33554435", "100000000000000000000", "0.000000000000000000001", "7\t", "\"7\"", "1.0000000596046448"]


# ---- addCells through the facade against the replayed restatement ----

def write(path, content):
    with open(str(path), "wb") as f:
        f.write(content if isinstance(content, bytes) else content.encode("utf-8"))
    return str(path)


def check_add_cells(directory, steps, use_device, chunk_bytes=None):
    """steps: (expression file, expression separators, meta data file, meta data separators, additional pairs) per call.
    The calls through ExpressionMatrix.addCells into <directory>/product, the restatement's call sequences replayed through
    addGene / addCell into <directory>/replayed.  Both succeed with equal stores (object for object), or both fail at the
    same step with the same text, the product's files then byte-identical to before the failing call.
    -> (the error text or None, the product's directory, the deferred field counts per successful call)."""
    import ingest_binding as ib
    import expressionmatrix2_amd.expression_matrix as facade
    from expressionmatrix2_amd import ExpressionMatrix
    os.makedirs(str(directory), exist_ok=True)
    product_dir, replayed_dir = os.path.join(str(directory), "product"), os.path.join(str(directory), "replayed")
    product, replayed = ExpressionMatrix.create(product_dir), ExpressionMatrix.create(replayed_dir)
    saved = facade.CSV_USE_DEVICE, facade.CSV_CHUNK_BYTES
    facade.CSV_USE_DEVICE = use_device
    if chunk_bytes is not None:
        facade.CSV_CHUNK_BYTES = chunk_bytes
    error, deferred = None, []
    try:
        for expression, expression_separators, meta, meta_separators, additional in steps:
            expected = None
            try:
                replay(replayed, restated_add_cells(expression, expression_separators, meta, meta_separators, additional))
            except (Failure, RuntimeError) as failure:
                expected = str(failure)
            product.flush()
            before = ib.file_bytes(product_dir)
            try:
                product.addCells(expressionCountsFileName=expression, expressionCountsFileSeparators=expression_separators,
                                 cellMetaDataFileName=meta, cellMetaDataFileSeparators=meta_separators,
                                 additionalCellMetaData=additional)
                got = None
                deferred.append(product.lastCsvDeferredFieldCount)
            except RuntimeError as failure:
                got = str(failure)
            assert got == expected, "addCells says %r, the reference's loops say %r" % (got, expected)
            if expected is not None:
                product.flush()
                assert ib.file_bytes(product_dir) == before, "a failing addCells changed the store"
                error = expected
                break
    finally:
        facade.CSV_USE_DEVICE, facade.CSV_CHUNK_BYTES = saved
        product.close()
        replayed.close()
    if error is None:
        a, b = ib.read_store(product_dir), ib.read_store(replayed_dir)
        for key in b:
            assert a[key] == b[key], "the stores differ in %s" % key
    return error, product_dir, deferred
