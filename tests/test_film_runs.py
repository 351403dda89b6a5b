"""The counts the closed-records film route takes from ballots (liverrenderer_amd/csrc/film_runs.h: the lanes of a run, how many of them are
set in one mask or in two), without a GPU: tests/host/film_runs_main.cpp compares them with a plain loop over the 64 lanes, for every lane of
one run of 64, 64 runs of one, runs that end at lane 63, member masks with holes and 6000 seeded random mask triples.  The program is compiled
under AddressSanitizer and UBSan the way tests/test_record_layout.py compiles its program (a shift by 64 or a count of leading zeros of 0 would
be undefined behaviour in the header); only that program is sanitized, nothing of it is loaded into Python."""
import json
import os
import subprocess

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "liverrenderer_amd", "csrc")
# case -> mask triples the program checks (64 lanes each)
CASES = {"one run": 3, "64 runs of one lane": 3, "a run that ends at lane 63": 126, "member mask with holes": 4, "random": 6000}


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("film_runs") / "film_runs_main")
    cc = subprocess.run(["g++", "-std=c++17", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan",
                         "-I", CSRC, "-Wall", "-Werror", os.path.join(ROOT, "tests", "host", "film_runs_main.cpp"), "-o", exe], capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr[-4000:]
    env = dict(os.environ, ASAN_OPTIONS="halt_on_error=1:detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    run = subprocess.run([exe], capture_output=True, text=True, env=env)
    print(run.stdout)
    assert "Sanitizer" not in run.stderr and "runtime error" not in run.stderr, run.stderr[-4000:]
    return run.returncode, [json.loads(l) for l in run.stdout.splitlines()]


def test_every_case_ran(lines):
    assert {l["case"]: l["triples"] for l in lines[1]} == CASES
    for l in lines[1]:
        assert l["lanes"] == 64 * l["triples"], l


def test_counts_equal_the_loop_over_the_lanes(lines):
    status, out = lines
    for l in out:
        assert l["wrong"] == 0, l
    assert status == 0
