"""(not gpu) The per-line routine of the nearest-other-class transform (csrc/nearest_line.hpp: hull build, second sweep
and tie rule, and the two lines the Y and X kernels hand to it) compiled by g++ against the host stand-in for the HIP
runtime, with AddressSanitizer and UndefinedBehaviorSanitizer, and run by tests/cpp/nearest_line_host.cc: every class
pattern of lines of 1 - 10 rows with seeded heights, the deep-stack lines of 64, 65 and 300 rows and whole small grids,
each against a brute-force loop in the same program.  A stand-alone program: nothing loaded into python is sanitized."""
import os
import re
import subprocess

from conftest import ROOT

CPP = os.path.join(ROOT, "tests", "cpp")
COMPILE = ["g++", "-O1", "-g", "-std=c++17", "-x", "c++", "-Wall", "-Wextra", "-Wno-unused-parameter",
           "-Wno-unused-function", "-Wno-unknown-pragmas", "-Ihip_shim", "-I" + os.path.join(ROOT, "include"),
           "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-fno-sanitize-recover=undefined"]


def test_line_routine_on_cpu_under_sanitizers():
    subprocess.check_call(COMPILE + ["-o", "nearest_line_host", "nearest_line_host.cc"], cwd=CPP)
    run = subprocess.run([os.path.join(CPP, "nearest_line_host")], capture_output=True, text=True, timeout=300)
    print(run.stdout)
    assert run.returncode == 0, run.stdout[-3000:] + run.stderr[-3000:]
    assert "\n0 mismatches\n" in run.stdout and "PASSED" in run.stdout
    # every pattern of 1 - 10 rows, six sets of heights each
    assert int(re.search(r"short lines: (\d+)", run.stdout).group(1)) == 6 * sum(2 ** n for n in range(1, 11))
    for rows in (64, 65, 300):
        assert "flat line of %d rows: hull depth %d\n" % (rows, rows) in run.stdout
        assert re.search(r"convex line of %d rows: hull depth \d+" % rows, run.stdout)
