"""The index arithmetic of DPR_ALGO_ORDERED on the CPU, under the address and undefined-behaviour sanitizers.

Every loop bound of k_ord_gather comes from the sorted keys through csrc/dpr_ordered_index.h (key encode / decode,
cell ranges, the merge walk, the neighbour test).  tests/ordered_host_check.cpp is a stand-alone program around that
header: it builds the keys, stable-sorts, walks every output cell with the kernel's merge code and compares with a
plain serial splat, bit for bit.  It is compiled with -fsanitize=address,undefined and run as a child process on
the generated clouds of tests/ordered_cases.py; nothing is loaded into this interpreter.  No GPU."""
import os
import shutil
import subprocess

import pytest

from tests import ordered_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "ordered_host_check.cpp")


def _compiler():
    for cxx in (os.environ.get("CXX"), "c++", "g++", "clang++", "/opt/rocm/lib/llvm/bin/clang++"):
        if cxx and shutil.which(cxx):
            return shutil.which(cxx)
    raise RuntimeError("no C++ compiler found for the host check of DPR_ALGO_ORDERED")


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("ordered_host") / "ordered_host_check")
    cmd = [_compiler(), "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fno-sanitize-recover=all",
           "-fsanitize=address,undefined", "-Wno-unknown-pragmas", SRC, "-o", exe]
    # the sanitizer runtimes linked into the program itself (gcc links them dynamically by default), so that it
    # starts the same whatever else the process environment loads
    for static in (["-static-libasan", "-static-libubsan"], ["-static-libsan"], []):
        if subprocess.run(cmd + static, capture_output=True).returncode == 0:
            return exe
    subprocess.check_call(cmd)  # (shows the compiler's message)
    return exe


def _cases():
    """(n_in, n_out, kind, grid, P): every kind on the awkward grid of each output dimension and on a cubic one,
    plus the edge sizes."""
    out = []
    for n_in, n_out in [(1, 1), (2, 2), (3, 2), (3, 3), (2, 3), (4, 4), (3, 4)]:
        for kind in C.KINDS:
            out.append((n_in, n_out, kind, C.NASTY_GRIDS[n_out], 5000))
            out.append((n_in, n_out, kind, 8 if n_out < 4 else 5, 5000))
        for P in (0, 1, 255, 256, 257):
            out.append((n_in, n_out, "overhang", C.NASTY_GRIDS[n_out], P))
    out.append((3, 3, "one_cell", 8, 20000))
    return out


def test_host_walk_matches_the_serial_splat_under_sanitizers(program, tmp_path):
    files = []
    for i, (n_in, n_out, kind, grid, P) in enumerate(_cases()):
        d = C.make(kind, n_in, n_out, P, 2, grid, seed=100 + i)
        path = str(tmp_path / f"case{i:03d}_{n_in}{n_out}_{kind}_{P}.bin")
        C.write_case(path, d, b=i % 2)
        files.append(path)
    env = dict(os.environ)
    env["ASAN_OPTIONS"] = "detect_leaks=1:abort_on_error=0"
    env["UBSAN_OPTIONS"] = "print_stacktrace=1:halt_on_error=1"
    r = subprocess.run([program] + files, capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, f"exit {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}"
    assert "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    assert r.stdout.count(": ok (") == len(files)
    # the walk did visit contributions (not an empty table): the 5000-point clouds reach the grid
    assert any("5000 points" in line and not line.rstrip().endswith(" 0 contributions)") for line in r.stdout.splitlines())


def test_host_program_fails_on_a_walk_out_of_order_and_on_an_unreadable_file(program, tmp_path):
    """The checker itself.  With `--reversed-lists` the program reverses every cell's list after its sort (on the host
    only), so the same merge code meets descending point indices: it must report the walk and exit 1.  Without the
    switch the same file passes.  A truncated file is refused with exit 2."""
    d = C.make("one_cell", 3, 3, 500, 1, 8, seed=7)
    good = str(tmp_path / "good.bin")
    C.write_case(good, d)
    r = subprocess.run([program, good], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and ": ok (" in r.stdout, r.stderr[-2000:]
    r = subprocess.run([program, "--reversed-lists", good], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "out of order" in r.stderr, (r.returncode, r.stderr[-2000:])
    assert "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-2000:]
    short = str(tmp_path / "short.bin")
    with open(short, "wb") as f:
        f.write(b"\x01\x00\x00\x00")
    r = subprocess.run([program, short], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2
