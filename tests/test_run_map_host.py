"""The per-run un-permute map of the tiled pullback on the CPU, under the address and undefined-behaviour sanitizers.

csrc/dpr_run_map.h holds the format k_scatter_wc_runs writes and k_unpermute_runs reads (an owner word per sorted
position with a run-start bit, one record slot per run, the runs cut at every 64th position so that a wave decodes its
64 positions alone) and both directions of it as plain functions.
tests/run_map_host_check.cpp is a stand-alone program around that header: it encodes the map of a scatter sub-chunk
from (tile of each point, cursors) as the scatter does, decodes every sorted position as the un-permute does, and
holds the result to a counting sort of its own, for sub-chunks of 2048 and of 4096 points:

  every point in one tile | every point in its own tile (as many runs as points) | no valid point | valid and
  rejected points alternating | a single valid point, first or last | a ragged last sub-chunk of 1, S - 1 and S
  points | 1000 random sub-chunks over 1 - 4096 tiles

It is compiled with -fsanitize=address,undefined and run as a child process; nothing is loaded into this interpreter.
No GPU."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "run_map_host_check.cpp")
MAPS_PER_SIZE = 2 * (7 + 2 * 3 + 1000)  # every case is encoded twice on the same cursors


def _compiler():
    for cxx in (os.environ.get("CXX"), "c++", "g++", "clang++", "/opt/rocm/lib/llvm/bin/clang++"):
        if cxx and shutil.which(cxx):
            return shutil.which(cxx)
    raise RuntimeError("no C++ compiler found for the host check of the run map")


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("run_map_host") / "run_map_host_check")
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


def test_every_position_decodes_to_its_record_under_sanitizers(program):
    r = _run(program)
    assert r.returncode == 0, f"exit {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}"
    assert "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    for s in (2048, 4096):
        assert f"S = {s}: ok ({MAPS_PER_SIZE} maps, " in r.stdout, r.stdout


def test_host_program_fails_on_a_wrong_run_start_bit(program):
    """The checker itself.  With `--flip-start-bit` one run-start bit of every map is inverted between the encoder and
    the decoder: the positions behind it decode to another run's slots, the program must name statement 2 and exit 1.
    An unknown argument is refused with exit 2."""
    r = _run(program, "--flip-start-bit")
    assert r.returncode == 1 and "statement 2" in r.stderr, (r.returncode, r.stderr[-2000:])
    assert "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-2000:]
    assert _run(program, "--no-such-switch").returncode == 2
