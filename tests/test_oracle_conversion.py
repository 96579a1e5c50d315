"""(not gpu) The CPU oracle's final conversion at the edges: oracle.sdf_from_occupancy against the oracle-free reference of
tests/sdf_conversion_ref.py (exact squared distances of lattice / few-site / complement scenes, the virtual border), every
voxel bit for bit, at near ties, exact ties on perfect squares, the fast conversion's range edges, subnormal, underflow and
overflow resolutions.  The same reference checks the device paths in tests/test_gpu_sdf_conversion.py."""
import numpy as np
import pytest

import sdf_conversion_ref as R
from conftest import bits_equal


@pytest.fixture(scope="module")
def oracle():
    from oracle import oracle as O
    return O


def _scenes():
    return [
        R.lattice_scene("dense", (70, 45, 40), range(70), R.periodic(45, 30, 7), R.periodic(40, 24, 5)),
        R.lattice_scene("sparse", (130, 40, 33), R.periodic(130, 61, 7), R.periodic(40, 23, 4), R.periodic(33, 29, 2),
                        extra_sites=[(100, 20, 30), (3, 39, 0)]),
        R.complement_scene("holes", (90, 30, 20), [(5, 3, 7), (80, 25, 15)]),
        R.lattice_scene("long", (1030, 4, 4), [0], [0], [0]),
        R.uniform_scene("all-free", (20, 9, 7), False),
        R.uniform_scene("all-filled", (20, 9, 7), True),
    ]


SCENES = {s.name: s for s in _scenes()}


def _resolutions(scene):
    extremes = R.ordinary_resolutions() + R.range_edges() + R.extreme_resolutions()
    if not np.isfinite(scene.d2).any():
        return [r for r in extremes if r.target is None]
    out = extremes
    for lo, hi in ((2, 512), (512, 1 << 20), (1 << 20, 1 << 31)):
        out = out + R.near_ties(R.pick_d2(scene, lo, hi, 3))
    for d2 in R.pick_d2(scene, 1, 512, 2, squares=True):
        k = int(round(np.sqrt(d2)))
        out = out + [R.square_tie(k, False), R.square_tie(k, True)]
    return out


def test_reference_self_checks():
    """The constructed resolutions do what they claim (each builder asserts its own property; this pins the counts)."""
    assert len(R.extreme_resolutions()) == 10 and len(R.range_edges()) == 4
    assert R.range_edges()[0].value == 1.0e-30 and R.range_edges()[1].value > 1.0e-30
    assert R.range_edges()[2].value < 1.0e30 and R.range_edges()[3].value == 1.0e30
    for d2 in (2, 3, 500, 513, 99999, (1 << 20) + 7, 2 ** 31 - 1):
        for product in (1e-20, 0.3, 7.7, 1e30):
            for nudge in (-2, 0, 2):
                R.near_tie(d2, product, nudge)
    for k in (1, 2, 3, 12, 22, 45):
        for odd in (False, True):
            r = R.square_tie(k, odd)
            p = np.float64(k) * np.float64(r.value)
            lo, hi = np.float32(p - 2.0 ** -24), np.float32(p + 2.0 ** -24)
            assert np.float32(p) == (hi if odd else lo)  # the tie rounds to even: up for N = 3 mod 4, down for 1 mod 4
    # every near tie and square tie must be built for a d2 the scene holds, or the case would test nothing
    for scene in SCENES.values():
        rs = _resolutions(scene)
        R.check_targets(scene, rs)
        if np.isfinite(scene.d2).any():
            assert sum(r.label == "near-tie" for r in rs) >= 6, scene.name
    assert (SCENES["long"].d2 > (1 << 20)).any()
    assert (SCENES["dense"].d2 < 512).all()


@pytest.mark.parametrize("name", sorted(SCENES))
@pytest.mark.parametrize("border", [False, True])
def test_oracle_final_conversion_at_the_edges(oracle, name, border):
    scene = SCENES[name].with_border() if border else SCENES[name]
    resolutions = _resolutions(scene) if not border else [
        r for r in _resolutions(SCENES[name]) if r.target is None or scene.contains(r.target)]
    R.check_targets(scene, resolutions)
    occ = scene.occupancy()
    for res in resolutions:
        want = scene.expected(res.value)
        got, lo, hi = oracle.sdf_from_occupancy(occ, res.value, True, border)
        assert bits_equal(got, want), "%s, %r: %s" % (scene.name, res, R.first_mismatch(got, want))
        assert (lo, hi) == R.extrema(want), (scene.name, res)
