"""The index arithmetic of the smooth DPR_ALGO_TILED path on the CPU, under the address and undefined-behaviour
sanitizers.

csrc/dpr_smooth_tile.h writes down the rule by which the key kernels and the tile kernels of the smooth families find
the tile of a point, the LDS cell of a deposit and the grid cell of a flushed LDS cell (the kernels carry the same
arithmetic as their own text; the header says why).  tests/smooth_tile_host_check.cpp is a stand-alone program around
that header: exhaustively, without random inputs, over

  2-D (1,1) (64,16) (65,17) (63,15) (130,33)      3-D (1,1,1) (16,8,8) (17,9,9) (15,7,7) (33,17,3)

(one tile, an exact tile, one cell over, one cell under, several tiles with a ragged last one) it checks that the key
of a tile's origin is the tile, that every centre cell smooth_cell can return has a tile, that every one of a point's
3^N cells that lies in the grid is deposited into an LDS cell which the flush decodes back to exactly that grid cell
(and that no cell outside the grid is deposited), and that the flush of a tile stays inside the plane and writes no
cell twice.  It is compiled with -fsanitize=address,undefined and run as a child process; nothing is loaded into this
interpreter.  No GPU."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "smooth_tile_host_check.cpp")
GRIDS = 10


def _compiler():
    for cxx in (os.environ.get("CXX"), "c++", "g++", "clang++", "/opt/rocm/lib/llvm/bin/clang++"):
        if cxx and shutil.which(cxx):
            return shutil.which(cxx)
    raise RuntimeError("no C++ compiler found for the host check of the smooth tiles")


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("smooth_tile_host") / "smooth_tile_host_check")
    cmd = [_compiler(), "-std=c++17", "-O1", "-g", "-fno-sanitize-recover=all", "-fsanitize=address,undefined",
           "-Wno-unknown-pragmas", SRC, "-o", exe]
    # the sanitizer runtimes linked into the program itself (gcc links them dynamically by default), so that it
    # starts the same whatever else the process environment loads
    for static in (["-static-libasan", "-static-libubsan"], ["-static-libsan"], []):
        if subprocess.run(cmd + static, capture_output=True).returncode == 0:
            return exe
    subprocess.check_call(cmd)  # (shows the compiler's message)
    return exe


def _run(program, *args):
    env = dict(os.environ)
    env["ASAN_OPTIONS"] = "detect_leaks=1:abort_on_error=0"
    env["UBSAN_OPTIONS"] = "print_stacktrace=1:halt_on_error=1"
    return subprocess.run([program, *args], capture_output=True, text=True, env=env, timeout=120)


def test_every_deposit_is_flushed_to_its_cell_under_sanitizers(program):
    r = _run(program)
    assert r.returncode == 0, f"exit {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}"
    assert "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    assert r.stdout.count("): ok (") == GRIDS, r.stdout
    # the walk did deposit (not an empty loop): no grid reports 0 deposits
    assert not any(line.rstrip().endswith(" 0 deposits)") for line in r.stdout.splitlines()), r.stdout


def test_host_program_fails_when_the_origin_disagrees_with_the_key(program):
    """The checker itself.  With `--shifted-origins` every tile origin is moved one cell up on the host only, so a
    point binned by the key meets an LDS tile that does not hold all of its cells: the program must name statement 3
    and exit 1.  An unknown argument is refused with exit 2."""
    r = _run(program, "--shifted-origins")
    assert r.returncode == 1 and "statement 3" in r.stderr, (r.returncode, r.stderr[-2000:])
    assert "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-2000:]
    assert _run(program, "--no-such-switch").returncode == 2
