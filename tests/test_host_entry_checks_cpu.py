"""The argument checks of the host-buffer searches em2_find_similar_pairs4/5/6/7 and of the device-level
em2_dev_find_similar_pairs5/6/7 through the raw C ABI: return code and the whole em2_last_error() text, and the order the
checks come in -- the algorithm's own argument errors, then "nothing to do" (no cells, an empty row range) = OK, then null
pointers, then the missing device.  None of these cases reaches the device, so the test needs none; no pointer handed over
is read (the device-level calls get host addresses for that reason)."""
import numpy as np
import pytest

from expressionmatrix2_amd import capi

OK, INVALID, NO_DEVICE, RUNTIME, UNSUPPORTED = 0, 1, 2, 5, 6

N, L, K, THR = 6, 128, 3, 0.2
SIG = np.zeros((N, 2), dtype=np.uint64)
PAIRS = np.zeros((N, K), dtype=capi.PAIR_DTYPE)
USED = np.zeros(N, dtype=np.uint32)
SLICES = np.array([10, 8], dtype=np.int32)

NO_DEVICE_TEXT = ": no HIP device is visible (this library has no CPU path)"
FSP7_ASSERTION = ("Assertion failed: no mismatch count has a similarity below the similarity threshold "
                  "(Lsh::computeMismatchCountThresholdFromSimilarityThreshold)")


def _p(a):
    return a.ctypes.data if isinstance(a, np.ndarray) else a


def _extra(extra):
    return [_p(a) for a in extra]          # (the arrays stay alive in `extra` for the length of the call)


def host(name, extra, sig=SIG, n=N, lsh=L, k=K, thr=THR, pairs=PAIRS, used=USED):
    lib = capi.load()
    rc = getattr(lib, name)(_p(sig), n, lsh, k, thr, *_extra(extra), _p(pairs), _p(used))
    return rc, lib.em2_last_error().decode()


def dev(name, extra, sig=SIG, n=N, rows=(0, N), lsh=L, k=K, thr=THR, pairs=PAIRS, used=USED):
    lib = capi.load()
    rc = getattr(lib, name)(_p(sig), n, rows[0], rows[1], lsh, k, thr, *_extra(extra), _p(pairs), _p(used), None)
    return rc, lib.em2_last_error().decode()


def fsp5(q=8, overflow=1000):
    return (q, overflow)


def fsp6(P=4, S=10, pbits=64, seed=231):
    return (P, S, pbits, seed)


def fsp7(slices=SLICES, count=None, max_check=100, log2_buckets=12):
    return (slices, (0 if slices is None else len(slices)) if count is None else count, max_check, log2_buckets)


# entry point -> the extra arguments of a valid call
HOST = {
    "em2_find_similar_pairs4": (),
    "em2_find_similar_pairs5": fsp5(),
    "em2_find_similar_pairs6": fsp6(),
    "em2_find_similar_pairs7": fsp7(),
}
DEV = {
    "em2_dev_find_similar_pairs5": fsp5(),
    "em2_dev_find_similar_pairs6": fsp6(),
    "em2_dev_find_similar_pairs7": fsp7(),
}


def _argument_errors(name):
    """(extra arguments, keyword overrides, expected code, expected text) of the entry point's own argument checks."""
    cases = [((), dict(lsh=0), INVALID, name + ": lshCount must be positive")]
    if name.endswith("5"):
        text = name + ": lshSliceLength must be in [1,32]"
        if "_dev_" not in name:
            text += " (the reference divides by zero for 0)"
        cases += [(fsp5(q=0), {}, INVALID, text), (fsp5(q=33), {}, INVALID, text)]
    if name.endswith("6"):
        cases += [
            (fsp6(pbits=200), {}, RUNTIME, "Argument permutationStoreBitCount 200 exceeds number of signature bits 128"),
            (fsp6(pbits=0), {}, INVALID, name + ": permutedBitCount must be positive"),
            (fsp6(P=65), {}, UNSUPPORTED, name + ": permutationCount above 64 is not supported"),
            (fsp6(pbits=65473), dict(lsh=70000), UNSUPPORTED, name + ": permutedBitCount above 65472 is not supported"),
            (fsp6(P=64, S=9000), dict(n=200), UNSUPPORTED,
             name + ": more than 8192 candidates per cell (min(searchCount, permutationCount*(cellCount-1))) is not supported"),
        ]
    if name.endswith("7"):
        cases += [
            (fsp7(slices=None, count=2), {}, INVALID, name + ": null sliceLengths"),
            (fsp7(np.array([8, 8], dtype=np.int32)), {}, RUNTIME, "The slice lengths are not in decreasing order."),
            (fsp7(np.array([65], dtype=np.int32)), {}, RUNTIME, "Each slice length can be at most 64 bits."),
            (fsp7(np.array([8, 0], dtype=np.int32)), {}, INVALID, name + ": slice lengths must be positive"),
            (fsp7(np.array([8, -3], dtype=np.int32)), {}, INVALID, name + ": slice lengths must be positive"),
            (fsp7(log2_buckets=41), {}, UNSUPPORTED, name + ": log2BucketCount above 40 is not supported"),
            (fsp7(), dict(k=4097), UNSUPPORTED, name + ": k above 4096 is not supported"),
            (fsp7(), dict(thr=-1.5), RUNTIME, FSP7_ASSERTION),
        ]
    return cases


@pytest.mark.parametrize("name", sorted(HOST))
def test_host_entry_argument_errors(name):
    for extra, overrides, code, text in _argument_errors(name):
        extra = extra or HOST[name]
        assert host(name, extra, **overrides) == (code, text), (extra, overrides)
        # ... and they come before everything else: no cells and null pointers do not hide them
        if "n" not in overrides:
            assert host(name, extra, **dict(overrides, n=0, sig=None, pairs=None, used=None)) == (code, text), (extra, overrides)


@pytest.mark.parametrize("name", sorted(HOST))
def test_host_entry_nothing_to_do_then_null_pointers_then_the_device(name):
    extra = HOST[name]
    null = (INVALID, name + ": null pointer")
    # no cells: OK, whatever the pointers
    assert host(name, extra, n=0)[0] == OK
    assert host(name, extra, n=0, sig=None, pairs=None, used=None)[0] == OK
    # null pointers, before the device is looked for
    assert host(name, extra, sig=None) == null
    assert host(name, extra, used=None) == null
    assert host(name, extra, pairs=None) == null
    # valid arguments; pairs may be null when k is 0
    for overrides in ({}, dict(k=0, pairs=None)):
        rc, text = host(name, extra, **overrides)
        if capi.device_count() == 0:
            assert (rc, text) == (NO_DEVICE, name + NO_DEVICE_TEXT)
        else:
            assert rc == OK, text


@pytest.mark.parametrize("name", sorted(DEV))
def test_device_entry_argument_errors(name):
    for extra, overrides, code, text in _argument_errors(name):
        extra = extra or DEV[name]
        assert dev(name, extra, **overrides) == (code, text), (extra, overrides)
        # ... before the row range, the empty range and the null pointers
        assert dev(name, extra, **dict(overrides, rows=(4, 2), sig=None, pairs=None, used=None)) == (code, text), (extra, overrides)


@pytest.mark.parametrize("name", sorted(DEV))
def test_device_entry_row_range_then_nothing_to_do_then_null_pointers(name):
    extra = DEV[name]
    bad = (INVALID, name + ": bad row range")
    null = (INVALID, name + ": null pointer")
    assert dev(name, extra, rows=(4, 2)) == bad
    assert dev(name, extra, rows=(0, N + 1)) == bad
    assert dev(name, extra, rows=(N + 1, N + 1)) == bad
    assert dev(name, extra, rows=(4, 2), sig=None, pairs=None, used=None) == bad
    # an empty range: OK, whatever the pointers
    for rows in ((0, 0), (3, 3), (N, N)):
        assert dev(name, extra, rows=rows)[0] == OK
        assert dev(name, extra, rows=rows, sig=None, pairs=None, used=None)[0] == OK
    assert dev(name, extra, n=0, rows=(0, 0), sig=None, pairs=None, used=None)[0] == OK
    assert dev(name, extra, sig=None) == null
    assert dev(name, extra, used=None) == null
    assert dev(name, extra, pairs=None) == null
    assert dev(name, extra, rows=(2, 3), pairs=None) == null
