"""(not gpu) csrc/host_staging.hpp -- the one helper every host-pointer entry point of the C ABI stages through -- compiled
by g++ against a fake of the HIP runtime (tests/cpp/hip_fake) and run by tests/cpp/test_host_staging.cc: the order of a
successful call, the carving of the one block, absent and empty arrays, and the failure paths that no GPU test can
reach (the allocation, each upload, the body, each download and the wait failing in turn).  Once plain and once under
AddressSanitizer + UndefinedBehaviorSanitizer.  Stand-alone programs: nothing loaded into python is sanitized."""
import os
import subprocess

import pytest

from conftest import ROOT

CPP = os.path.join(ROOT, "tests", "cpp")


def _build_and_run(target):
    subprocess.check_call(["make", "-s", "-C", CPP, target])
    run = subprocess.run([os.path.join(CPP, target)], capture_output=True, text=True, timeout=120)
    print(run.stdout)
    assert run.returncode == 0, run.stdout[-3000:] + run.stderr[-3000:]
    assert run.stdout.strip().endswith("PASSED")


def test_staging_helper_against_the_fake_runtime():
    _build_and_run("test_host_staging")


def test_staging_helper_under_sanitizers():
    path = subprocess.run(["gcc", "-print-file-name=libasan.so"], capture_output=True, text=True).stdout.strip()
    if not os.path.isabs(path) or not os.path.exists(path):
        pytest.skip("libasan not available")
    _build_and_run("test_host_staging_asan")
