"""(not gpu) tests/motion_self_ref.py, the CPU restatement of vgt_hip_check_motions_with_self, held to the two
consequences the header states and to a reduction worked out by hand; the shared cases of tests/motion_self_cases.py held
to what they must contain, so that no GPU test passes by accident; and the argument errors of the two entry points that
need no device."""
import ctypes
import os
import re

import numpy as np
import pytest

import motion_ref
import motion_self_cases as C
import motion_self_ref as R
import self_ref
from conftest import ROOT
from voxelized_geometry_tools_amd import capi

NAMES = {"vgt_hip_check_motions_with_self": 35, "vgt_hip_check_motions_with_self_dev": 35,
         "vgt_hip_motion_self_tile_samples": 2}
HOOK = "vgt_hip_testing_set_motion_self_workgroups"


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(capi.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return capi.load()


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    if a.dtype.kind != "f":
        return np.array_equal(a, b)
    nan_a, nan_b = np.isnan(a), np.isnan(b)
    return np.array_equal(nan_a, nan_b) and np.array_equal(a[~nan_a].view(np.uint64), b[~nan_b].view(np.uint64))


def test_coverage():
    total = C.Coverage(*([0] * 7))
    for index, name in enumerate(C.names()):
        found = C.coverage(index)
        print(name, found, "statuses", np.bincount(C.case(index).want.status, minlength=3).tolist())
        total = C.Coverage(*[a + b for a, b in zip(total, found)])
        if name in ("arm-21", "body-9"):
            assert found.environment_only >= 3 and found.self_only >= 3, (name, found)
        if name == "arm-21-planted":
            c = C.case(index)
            assert (c.want.first_collision == 0).all() and found.both >= 60
    assert total.both >= 1 and total.first_collision_moved >= 1 and total.stop_moves_self_minimum >= 1
    assert total.self_no_value_alone >= 1 and total.self_threshold_occurs >= 1
    # what the issue states for the four cases at the 0.02 quantile
    counts = {name: C.coverage(C.names().index(name))[:3] for name in ("arm-21", "body-9", "body-9-odd", "arm-21-frame")}
    assert counts == {"arm-21": (4, 8, 0), "body-9": (3, 7, 0), "body-9-odd": (43, 1, 0), "arm-21-frame": (4, 8, 0)}


def test_the_cases_sit_on_both_sides_of_every_tile():
    tiles = set()
    for index in range(len(C.names())):
        c = C.case(index)
        tile = C.tile_formula(c.tree.num_links, len(c.link))
        tiles.add(tile)
        assert tile >= 1 and len(c.pairs) <= C.MOST_PAIRS
        if np.ndim(c.num_steps) == 0:                     # (uniform steps: full tiles and a rest)
            assert (c.num_steps + 1) % tile != 0 and c.num_steps + 1 > tile, (c.name, tile)
            continue
        samples = np.diff(c.first)
        # full tiles alone, a full tile and one sample more, and a tile that is not full
        assert (samples % tile == 0).any() and ((samples > tile) & (samples % tile == 1 % tile)).any(), (c.name, tile)
        assert tile == 1 or (samples % tile != 0).any(), (c.name, tile)
    assert tiles >= {1, 2, 4, 8, 16, 64}


@pytest.mark.parametrize("stop", [False, True], ids=["all", "stop"])
def test_without_the_self_part_it_is_the_reduction_of_check_motions(stop):
    for name in ("arm-21", "body-9-odd", "arm-0"):
        c = C.case(C.names().index(name))
        got = R.reduce_with_self(c.samples, None, c.first, stop)
        want = motion_ref.reduce_motions(c.samples, c.first, stop)
        for field in R.SHARED:
            assert same_bits(getattr(got, field), getattr(want, field)), (name, field)
        assert np.array_equal(got.collision_cause, (want.first_collision >= 0).astype(np.uint8))
        assert np.isnan(got.self_min_clearance).all() and (got.self_min_sample == -1).all()
        assert (got.self_min_pair == -1).all()


def test_without_the_stop_flag_the_environment_outputs_are_those_of_check_motions():
    seen = 0
    for index in range(len(C.names())):
        c = C.case(index)
        if c.samples is None:
            assert np.isnan(c.want.min_clearance).all() and np.isnan(c.want.min_gradient).all()
            assert (c.want.min_sample == -1).all() and (c.want.min_sphere == -1).all()
            continue
        want = C.environment_alone(c, False)
        for field in R.ENVIRONMENT:
            assert same_bits(getattr(c.want, field), getattr(want, field)), (c.name, field)
        seen += int((c.want.first_collision != want.first_collision).sum())
    assert seen >= 10                                     # (whatever the self part finds)


def test_a_reduction_by_hand():
    """Two motions of four and three samples.  Motion 0: the self part collides at k = 1, the environment at k = 2;
    motion 1: sample 1 is NO_VALUE in the self part alone and nothing collides."""
    nan = np.nan
    environment = motion_ref.Samples(np.array([0, 0, 1, 0, 0, 0, 0], np.uint8),
                                     np.array([3.0, 2.0, 0.5, 0.25, 1.0, nan, 1.0]),
                                     np.array([4, 5, 6, 7, 1, -1, 2], np.int32),
                                     np.arange(21, dtype=np.float64).reshape(7, 3), np.array([0, 1, 0, 2, 0, 0, 0], np.uint8))
    status = np.array([0, 1, 0, 0, 0, 2, 0], np.uint8)
    own = self_ref.SelfCollisionChecks(status, None, None, np.array([0.5, -0.0, 0.0, -1.0, 2.0, nan, 2.0]),
                                       np.array([9, 8, 7, 6, 3, -1, 4], np.int32), None, None, environment.fk_status, None)
    first = np.array([0, 4, 7])
    got = R.reduce_with_self(environment, own, first, False)
    assert got.status.tolist() == [R.COLLISION, R.NO_VALUE] and got.first_collision.tolist() == [1, -1]
    assert got.collision_cause.tolist() == [R.CAUSE_SELF, 0]
    assert got.min_sample.tolist() == [3, 0] and got.min_sphere.tolist() == [7, 1]
    assert got.min_clearance.tolist() == [0.25, 1.0] and got.min_gradient[0].tolist() == [9.0, 10.0, 11.0]
    assert got.self_min_sample.tolist() == [3, 0] and got.self_min_pair.tolist() == [6, 3]
    assert got.fk_status.tolist() == [3, 0]
    stopped = R.reduce_with_self(environment, own, first, True)
    assert stopped.first_collision.tolist() == [1, -1] and stopped.min_sample.tolist() == [1, 0]
    assert stopped.self_min_sample.tolist() == [1, 0] and stopped.self_min_pair.tolist() == [8, 3]
    assert np.signbit(stopped.self_min_clearance[0]) and stopped.fk_status.tolist() == [1, 0]   # (-0.0: its own bits)
    # -0.0 and 0.0 tie: the lowest k
    tied = own._replace(min_clearance=np.array([0.5, -0.0, 0.0, 0.0, 2.0, nan, 2.0]))
    assert R.reduce_with_self(None, tied, first, False).self_min_sample.tolist() == [1, 0]
    # both parts at one sample: cause 3
    both = environment._replace(status=np.array([0, 1, 1, 0, 0, 0, 0], np.uint8))
    assert R.reduce_with_self(both, own, first, False).collision_cause.tolist() == [3, 0]
    # the field-less form
    alone = R.reduce_with_self(None, own, first, False)
    assert alone.status.tolist() == [R.COLLISION, R.NO_VALUE] and np.isnan(alone.min_clearance).all()
    assert (alone.min_sample == -1).all() and (alone.min_sphere == -1).all() and np.isnan(alone.min_gradient).all()


def test_declared_bound_and_exported(lib):
    text = open(os.path.join(ROOT, "include", "vgt_hip.h")).read()
    testing_section = text[text.index("#ifdef VGT_HIP_TESTING"):text.index("#endif /* VGT_HIP_TESTING */")]
    for needle in ("VGT_HIP_MOTION_SELF_NO_VALUE_IS_COLLISION 4u", "VGT_HIP_MOTION_CAUSE_ENVIRONMENT 1",
                   "VGT_HIP_MOTION_CAUSE_SELF 2", "equals that call's to the bit", "whatever the self part finds",
                   "Neither part: VGT_HIP_ERR_INVALID_ARGUMENT"):
        assert needle in text, needle
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    raw = ctypes.CDLL(capi.LIB_PATH)
    testing = ctypes.CDLL(capi.TESTING_LIB_PATH)
    for name, arguments in NAMES.items():
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in capi.SIGNATURES and len(capi.SIGNATURES[name][1]) == arguments
        assert hasattr(raw, name) and hasattr(testing, name), name
    assert HOOK in testing_section and HOOK not in capi.SIGNATURES
    assert HOOK in capi.TESTING_SIGNATURES and hasattr(testing, HOOK) and not hasattr(raw, HOOK)
    assert capi.MotionSelfChecks._fields == R.MotionSelfChecks._fields
    assert (capi.MOTION_SELF_NO_VALUE_IS_COLLISION, capi.MOTION_CAUSE_ENVIRONMENT, capi.MOTION_CAUSE_SELF) == (4, 1, 2)
    for links, spheres in [(1, 0), (8, 21), (15, 9), (8, 70), (8, 257), (84, 6), (664, 0), (665, 0), (1, 1989), (1, 1990),
                           (0, 5), (-1, 5), (5, -1), (2 ** 40, 1), (1, 2 ** 40)]:
        assert capi.motion_self_tile_samples(links, spheres) == C.tile_formula(links, spheres), (links, spheres)


def test_argument_errors_and_empty_batch_without_device(lib):
    """No context and no tree exist here: non-null stand-ins are never dereferenced before the checks are through."""
    stand_in = np.zeros(64)
    p = capi._ptr(stand_in)
    status = np.full(4, 9, np.uint8)
    xyzr = np.tile([0.0, 0.0, 0.0, 0.1], (3, 1))
    link = np.zeros(3, np.int32)
    pairs = np.array([[0, 1], [1, 2]], np.int32)
    steps = np.array([2, 0, 5, 1], np.int32)
    for host, fn in ((True, lib.vgt_hip_check_motions_with_self), (False, lib.vgt_hip_check_motions_with_self_dev)):
        def call(ctx=p, sdf=p, shape=(4, 4, 4), res=0.1, xyzr=capi._ptr(xyzr), link=capi._ptr(link), s=3,
                 pairs=capi._ptr(pairs), num_pairs=2, tree=p, a=p, b=p, steps=capi._ptr(steps), uniform=0, e=4,
                 clearance=0.0, self_clearance=0.0, flags=0, st=capi._ptr(status)):
            return fn(ctx, sdf, *shape, res, None, None, xyzr, link, s, pairs, num_pairs, tree, a, b, steps, uniform, e,
                      None, None, clearance, self_clearance, flags, st, *([None] * 10))

        def refused(needle, **kw):
            rc = call(**kw)
            message = lib.vgt_hip_last_error()
            assert rc == 1 and needle in message, (kw, rc, message)

        for name in ("ctx", "tree", "st", "xyzr", "link", "pairs"):
            refused(b"null", **{name: None})
        refused(b"neither a field nor a pair", sdf=None, num_pairs=0)
        refused(b"neither a field nor a pair", sdf=None, num_pairs=0, pairs=None, shape=(0, 0, 0))
        for res in (0.0, -0.1, float("inf"), float("nan")):
            refused(b"resolution", res=res)
        refused(b"minimum_clearance must not be NaN", clearance=float("nan"))
        refused(b"self_minimum_clearance must not be NaN", self_clearance=float("nan"))
        for flags in (8, 0x80000000, 15):
            refused(b"unknown motion check flag", flags=flags)
        refused(b"negative", shape=(4, -1, 4))
        refused(b"negative", s=-1)
        refused(b"negative", e=-1)
        refused(b"negative", num_pairs=-1)
        refused(b"uniform_steps -3 is negative", steps=None, uniform=-3)
        refused(b"2^31 cells", shape=(2048, 1024, 1024))
        refused(b"2^31", e=2 ** 31)
        refused(b"2^31", s=2 ** 31)
        refused(b"2^31", num_pairs=2 ** 31)
        # nothing to do: success before the tree is looked at, with whatever is null that E == 0 does not need
        assert call(e=0) == 0
        assert call(e=0, a=None, b=None, steps=None, s=0, xyzr=None, link=None, pairs=None) == 0
        assert call(e=0, uniform=0, steps=None, flags=7) == 0
        assert call(e=0, sdf=None, shape=(0, 0, 0), res=0.0, clearance=float("nan")) == 0   # (no field: not looked at)
        assert call(e=0, num_pairs=0, pairs=None, self_clearance=float("nan")) == 0         # (no pairs: not looked at)
        if host:
            # the host form looks at its arrays and names the first offender
            bad = steps.copy()
            bad[1], bad[3] = -3, -9
            refused(b"motion 1: num_steps -3", steps=capi._ptr(bad))
            model = xyzr.copy()
            model[1, 3] = model[2, 3] = np.nan
            refused(b"sphere 1: the radius must not be negative or NaN", xyzr=capi._ptr(model))
            for rows, needle in (([[0, 1], [1, 3]], b"pair 1: sphere 3 is outside [0, 3)"),
                                 ([[-1, 1], [1, 2]], b"pair 0: sphere -1 is outside [0, 3)"),
                                 ([[0, 1], [2, 2]], b"pair 1: (2, 2) is not ascending")):
                refused(needle, pairs=capi._ptr(np.array(rows, np.int32)))
        # a tree that is not this context's (the stand-in's zeroed bytes name no context at all)
        refused(b"another context")
    assert (status == 9).all()
