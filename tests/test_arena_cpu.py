"""The arena planner of expressionmatrix2_amd/csrc/em2_arena.h (ArenaPlan, arenaAt), which lays out the scratch of the
drivers: tests/native/em2_arena_main.cpp, a stand-alone host program, checks it and prints the blocks it took; the layout
is checked here once more from that output."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE_DIR = os.path.join(ROOT, "tests", "native")
SOURCE = os.path.join(NATIVE_DIR, "em2_arena_main.cpp")
HEADER = os.path.join(ROOT, "expressionmatrix2_amd", "csrc", "em2_arena.h")

SIZES = [0, 1, 255, 256, 257, 2**32 + 1]


def program():
    build = os.path.join(NATIVE_DIR, "build")
    os.makedirs(build, exist_ok=True)
    path = os.path.join(build, "em2_arena_main")
    newest = max(os.path.getmtime(SOURCE), os.path.getmtime(HEADER))
    if not os.path.exists(path) or os.path.getmtime(path) < newest:
        tmp = path + ".%d.tmp" % os.getpid()
        r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-o", tmp, SOURCE], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        os.replace(tmp, path)
    return path


def test_arena_plan():
    r = subprocess.run([program()], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert re.search(r"^em2_arena: [1-9][0-9]* checks passed$", r.stdout, re.M), r.stdout
    blocks = [(int(a), int(b)) for a, b in re.findall(r"^block (\d+) at (\d+)$", r.stdout, re.M)]
    assert [size for size, _ in blocks] == SIZES
    at = 0
    for i, (size, offset) in enumerate(blocks):
        assert offset % 256 == 0
        assert offset == at and (i == 0 or offset > blocks[i - 1][1])
        at += (max(size, 1) + 255) // 256 * 256            # a block of 0 bytes takes 256
    assert blocks[1][1] - blocks[0][1] == 256
