"""CheckMotionsWithSelf of the C++ host layer (include/vgt_hip/motion_self_queries.hpp) through
tests/cpp/test_motion_self_host.cc, built by the rule tests/cpp/Makefile has for its test binaries.  The answers come from
here: tests/motion_self_ref.py on the scene the program builds too, written to a file as hexadecimal doubles, so that the
program compares bit for bit.  Its --no-device mode (the argument errors) also runs once under AddressSanitizer +
UndefinedBehaviorSanitizer as a stand-alone CPU program: nothing loaded into python is sanitized."""
import glob
import os
import subprocess

import numpy as np
import pytest

import kinematics_ref
import motion_self_ref as R
from conftest import ROOT

CPP = os.path.join(ROOT, "tests", "cpp")
PKG = os.path.join(ROOT, "voxelized_geometry_tools_amd")
BINARY = os.path.join(CPP, "test_motion_self_host")


def _build():
    """tests/cpp/Makefile builds the binaries it lists in BINARIES by one pattern rule (which also brings the host layer's
    library up to date); this binary is not in that list, so the list is given on the command line."""
    if not os.path.exists(os.path.join(PKG, "libvgt_hip.so")):
        subprocess.check_call(["make", "-s", "-j4", "-C", os.path.join(PKG, "csrc")])
    subprocess.check_call(["make", "-s", "-C", CPP, "BINARIES=test_motion_self_host", "test_motion_self_host"])


def scene():
    """The scene at the head of tests/cpp/test_motion_self_host.cc."""
    sdf = np.empty((8, 4, 4), dtype=np.float32)
    sdf[:] = (np.arange(8, dtype=np.float32) + 1.5)[:, None, None]
    slide = np.eye(4)
    slide[:3, 3] = [0.0, 1.5, 1.5]
    bar = np.eye(4)
    bar[:3, 3] = [0.0, 0.5, 0.0]
    P, F = kinematics_ref.PRISMATIC, kinematics_ref.FIXED
    tree = kinematics_ref.Tree([-1, -1, 1], [P, P, F], [0, 1, 0], [[1, 0, 0], [1, 0, 0], [0, 0, 0]],
                               [slide.T.reshape(16), slide.T.reshape(16), bar.T.reshape(16)], 2)
    xyzr = np.array([[0.0, 0.0, 0.0, 0.25], [0.0, 0.0, 0.0, 0.25], [0.0, 0.0, 0.0, 0.125]])
    link = np.array([0, 1, 2], dtype=np.int32)
    pairs = np.array([[0, 1], [0, 2]], dtype=np.int32)
    return sdf, tree, xyzr, link, pairs


def motions():
    """23 motions inside the field and out of it, the two sliders crossing in some; a NaN row and an infinity."""
    rng = np.random.default_rng(5)
    joint_from = 1.0 + rng.random((23, 2)) * 6.0
    joint_to = 1.0 + rng.random((23, 2)) * 6.0
    joint_from[0] = [1.25, 1.5]                            # (one sample, near the wall and near each other: cause 3)
    joint_to[3] = [9.5, 12.0]                              # (leaves the grid)
    joint_from[4, 0] = np.nan
    joint_to[5, 1] = np.inf
    joint_to[6] = joint_from[6]                            # (goes nowhere)
    joint_from[7], joint_to[7] = [2.0, 5.0], [5.0, 2.0]    # (the sliders cross: coincident centres half way)
    steps = np.array([(0, 1, 2, 3, 7, 8, 9, 16, 33)[e % 9] for e in range(23)], dtype=np.int32)
    return joint_from, joint_to, steps


def write_answers(path):
    from oracle import oracle as O
    sdf, tree, xyzr, link, pairs = scene()
    joint_from, joint_to, steps = motions()
    minimum, self_minimum = 2.0, 0.25
    limits = np.array([[0.5, 6.5], [1.0, 7.5]])
    hexed = lambda v: float(v).hex() if np.isfinite(v) else ("nan" if np.isnan(v) else ("inf" if v > 0 else "-inf"))
    lines = ["%d %s %s %s" % (len(steps), hexed(minimum), hexed(self_minimum), " ".join(hexed(v) for v in limits.ravel()))]
    for a, b, n in zip(joint_from, joint_to, steps):
        lines.append("%s %s %d" % (" ".join(hexed(v) for v in a), " ".join(hexed(v) for v in b), n))
    seen = []
    for field, listed in ((sdf, pairs), (sdf, None), (None, pairs)):
        for stop in (False, True):
            want = R.check_motions_with_self(O, field, 1.0, xyzr, link, listed, tree, joint_from, joint_to, steps, minimum,
                                             self_minimum, stop_at_collision=stop, joint_limits=limits)
            seen.append(want)
            for e in range(len(steps)):
                lines.append("%d %d %d %s %d %d %s %s %d %d %d" % (
                    want.status[e], want.first_collision[e], want.collision_cause[e], hexed(want.min_clearance[e]),
                    want.min_sample[e], want.min_sphere[e], " ".join(hexed(v) for v in want.min_gradient[e]),
                    hexed(want.self_min_clearance[e]), want.self_min_sample[e], want.self_min_pair[e], want.fk_status[e]))
    with open(path, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    return seen


def test_the_answers_cover_what_the_program_relies_on(tmp_path):
    both, both_stopped = write_answers(str(tmp_path / "answers.txt"))[:2]
    assert set(both.status.tolist()) == {R.CLEAR, R.COLLISION, R.NO_VALUE}
    assert set(both.collision_cause.tolist()) >= {0, 1, 2, 3}
    assert (both.min_sample != both_stopped.min_sample).any() and both.fk_status.any()
    assert (both.self_min_sample != both_stopped.self_min_sample).any()


def test_argument_errors_without_device():
    _build()
    out = subprocess.run([BINARY, "--no-device"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "PASSED" in out.stdout


def test_argument_checks_under_sanitizers():
    """The host layer's sources are compiled into the program (as tests/cpp/Makefile does for test_hip_host_asan); the
    device library is linked as it is and no device is touched."""
    libasan = subprocess.run(["gcc", "-print-file-name=libasan.so"], capture_output=True, text=True).stdout.strip()
    if not os.path.isabs(libasan) or not os.path.exists(libasan):
        pytest.skip("libasan not available")
    if not os.path.exists(os.path.join(PKG, "libvgt_hip.so")):
        subprocess.check_call(["make", "-s", "-j4", "-C", os.path.join(PKG, "csrc")])
    binary = BINARY + "_asan"
    sources = sorted(glob.glob(os.path.join(PKG, "csrc", "host", "hip_*.cc")))
    assert os.path.join(PKG, "csrc", "host", "hip_motion_self_queries.cc") in sources
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-pthread", "-O1", "-g",
                           "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-fno-sanitize-recover=undefined",
                           "-I" + os.path.join(ROOT, "include"), "-o", binary,
                           os.path.join(CPP, "test_motion_self_host.cc")] + sources +
                          ["-L" + PKG, "-lvgt_hip", "-Wl,-rpath," + PKG])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    out = subprocess.run([binary, "--no-device"], capture_output=True, text=True, timeout=300, env=env)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    assert "PASSED" in out.stdout


@pytest.mark.gpu
def test_motions_with_self_through_cpp_layer(tmp_path):
    _build()
    path = str(tmp_path / "answers.txt")
    write_answers(path)
    out = subprocess.run([BINARY, path], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-2000:]
    assert "PASSED" in out.stdout
