"""(gpu) The SDF's final conversion, float32(sqrt(float64(d2)) * res) negated on filled voxels, on EVERY kernel path that
computes it, at near ties, exact ties, range edges, subnormal, underflow and overflow -- every voxel bit for bit against the
oracle-free reference of tests/sdf_conversion_ref.py, the extrema by value.

The X pass converts in several places (csrc/edt_sweep_kernels.hip: an exact table in LDS for full bands whose inputs are all
< 512, a fast conversion with a wave-ballot re-do of the unsure values elsewhere, the general copy for the virtual border and
resolutions outside (1e-30, 1e30); csrc/edt_short_kernels.hip for short lines; 64-bit entries beyond 1024 rows; the testing
library's brute-force finalize), and every entry point reaches them through its own launches.  Each test names the path and
the resolution of a failing case."""
import numpy as np
import pytest

import sdf_conversion_ref as R
from voxelized_geometry_tools_amd import capi, multi_gpu

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def vctx():
    c = capi.Context(0, testing=True)
    yield c
    c.set_edt_variant(0)
    c.set_short_line_rows(-1)
    c.close()


def general_resolutions():
    return R.ordinary_resolutions() + R.range_edges() + R.extreme_resolutions()


def tie_resolutions(scene, rows=None, ranges=((2, 512), (512, 1 << 20), (1 << 20, 1 << 31)), per_range=3, squares=2):
    """Near ties for d2 the scene holds (on the given X rows) in each range, and exact ties on perfect squares < 512."""
    out = []
    for lo, hi in ranges:
        out += R.near_ties(R.pick_d2(scene, lo, hi, per_range, rows))
    for d2 in R.pick_d2(scene, 1, 512, squares, rows, squares=True):
        k = int(round(np.sqrt(d2)))
        out += [R.square_tie(k, False), R.square_tie(k, True)]
    return out


def check(path, scene, res, got, lo, hi):
    want = scene.expected(res.value)
    bad = R.first_mismatch(got, want)
    assert not bad, "%s, scene %s, %r: %s" % (path, scene.name, res, bad)
    assert (lo, hi) == R.extrema(want), "%s, scene %s, %r: extrema (%r, %r), want %r" % (
        path, scene.name, res, lo, hi, R.extrema(want))


def run_host(c, path, scene, resolutions):
    R.check_targets(scene, resolutions)
    occ = scene.occupancy()
    for res in resolutions:
        got, lo, hi = c.sdf_from_occupancy(occ, res.value, True, scene.border)
        check(path, scene, res, got, lo, hi)


# ---- scenes: X extents in 129..1024 that are not a multiple of any band size (8, 16, 32) take the sweeps ----
_Y_DENSE = R.periodic(45, 30, 7)    # (y, z distances <= 15, 12: every input of the dense scenes below 512)
_Z_DENSE = R.periodic(64, 24, 5)


def dense_scene():
    """Every X slice holds sites: every input < 512, every full band takes the table (the partial last band does not)."""
    return R.lattice_scene("dense", (299, 45, 64), range(299), _Y_DENSE, _Z_DENSE)


def sparse_scene():
    """Sites on one X slice in 61: every band has a slice without any (inputs >= 512), the fast conversion everywhere."""
    return R.lattice_scene("sparse", (517, 40, 64), R.periodic(517, 61, 7), R.periodic(40, 23, 4), R.periodic(64, 29, 5),
                           extra_sites=[(200, 20, 40), (450, 3, 10)])


def mixed_scene():
    """Table bands (X rows 0..149 all sites) and fast bands (two site slices further on) in one line."""
    return R.lattice_scene("mixed", (451, 45, 64), list(range(150)) + [300, 420], _Y_DENSE, _Z_DENSE)


def holes_scene():
    """A filled grid with three free holes: large negative values."""
    return R.complement_scene("holes", (333, 30, 64), [(5, 3, 7), (300, 25, 60), (170, 15, 33)])


# X rows of full bands that take the table, whatever the band size (multiples of 32): the dense scene's rows before its partial
# last band, the mixed scene's rows of site slices
TABLE_ROWS = {"dense": (0, 288), "mixed": (0, 128)}


@pytest.mark.parametrize("make", [dense_scene, sparse_scene, mixed_scene, holes_scene],
                         ids=["dense", "sparse", "mixed", "holes"])
def test_x_sweep_table_and_fast_paths(ctx, make):
    scene = make()
    rows = TABLE_ROWS.get(scene.name)
    ties = tie_resolutions(scene, rows)
    if rows is not None:  # ... and ties of the rows past them (the partial band; the fast bands of the mixed scene)
        ties += tie_resolutions(scene, (rows[1], scene.shape[0]), ranges=((2, 512), (512, 1 << 20)), per_range=2, squares=0)
    assert len([r for r in ties if r.label == "near-tie"]) >= 6
    path = "X sweep (%s)" % ("table + fast" if rows is not None else "fast + re-do")
    run_host(ctx, path, scene, ties + general_resolutions())


def test_x_sweep_general_path_virtual_border(ctx):
    """The virtual border takes the general copy of the X sweep whatever the resolution."""
    for make in (dense_scene, sparse_scene, holes_scene):
        scene = make().with_border()
        run_host(ctx, "X sweep (general, virtual border)", scene, R.ordinary_resolutions() + tie_resolutions(scene, per_range=2))
    # (only squares there: the untargeted extremes, and ties on squares)
    scene = R.uniform_scene("all-free", (300, 20, 64), False).with_border()
    untargeted = [r for r in general_resolutions() if r.target is None]
    run_host(ctx, "X sweep (general, virtual border)", scene, untargeted + tie_resolutions(scene, squares=4))


def test_uniform_grids_give_infinities(ctx):
    for filled in (False, True):
        scene = R.uniform_scene("all-filled" if filled else "all-free", (300, 20, 64), filled)
        run_host(ctx, "X sweep (no other class)", scene, [r for r in general_resolutions() if r.target is None])


def test_x_sweep_64bit_entries_long_lines(ctx):
    """Lines beyond 1024 rows take 64-bit stack entries; squared distances beyond 2^20 only occur there."""
    scene = R.lattice_scene("long", (1100, 16, 64), [0], [3], [10])
    ties = tie_resolutions(scene, (1024, 1100), ranges=((1 << 20, 1 << 31),), per_range=4, squares=0)
    ties += tie_resolutions(scene, ranges=((2, 512), (512, 1 << 20)), per_range=2)
    run_host(ctx, "X sweep (64-bit entries)", scene, ties + general_resolutions())
    border = scene.with_border()
    run_host(ctx, "X sweep (64-bit entries, virtual border)", border,
             R.ordinary_resolutions() + tie_resolutions(border, ranges=((2, 512), (512, 1 << 20)), per_range=2))


def short_scenes():
    out = []
    for nx in (60, 100):
        out.append(R.lattice_scene("short%d" % nx, (nx, 40, 64), R.periodic(nx, 13, 2), R.periodic(40, 17, 3),
                                   R.periodic(64, 21, 6), extra_sites=[(nx - 1, 39, 63)]))
    out.append(R.complement_scene("short-holes", (90, 24, 64), [(4, 5, 6), (80, 20, 50)]))
    return out


@pytest.mark.parametrize("rows", [64, 128, 0])
def test_short_line_kernels(vctx, rows):
    """X lines of <= 64 rows (<= 128 with few items) take the short-line kernels; 128 puts every line here on them, 0 none."""
    vctx.set_edt_variant(0)
    try:
        vctx.set_short_line_rows(rows)
        for scene in short_scenes():
            path = "X short-line limit %d, nx %d" % (rows, scene.shape[0])
            run_host(vctx, path, scene, tie_resolutions(scene, ranges=((2, 512), (512, 1 << 20))) + general_resolutions())
            border = scene.with_border()
            run_host(vctx, path + " (virtual border)", border,
                     tie_resolutions(border, ranges=((2, 512),), per_range=2) + R.extreme_resolutions()[:4])
    finally:
        vctx.set_short_line_rows(-1)


def test_brute_force_finalize_variant(vctx):
    """The testing library's cross-check pipeline (variant 1) converts with its own brute-force X pass."""
    try:
        vctx.set_edt_variant(1)
        for scene in short_scenes()[1:]:
            path = "brute finalize (variant 1), nx %d" % scene.shape[0]
            run_host(vctx, path, scene, tie_resolutions(scene, ranges=((2, 512), (512, 1 << 20))) + general_resolutions())
            border = scene.with_border()
            run_host(vctx, path + " (virtual border)", border, tie_resolutions(border, ranges=((2, 512),), per_range=2))
    finally:
        vctx.set_edt_variant(0)


# ---- the other entry points: one near tie and the extreme resolutions each ----

def entry_scene():
    return R.lattice_scene("entry", (150, 40, 66), R.periodic(150, 37, 5), R.periodic(40, 17, 3), R.periodic(66, 23, 6),
                           extra_sites=[(149, 39, 65)])


def entry_resolutions(scene):
    d2 = R.pick_d2(scene, 512, 1 << 20, 1)[0]
    return [R.near_tie(d2, 7.7, -1), R.near_tie(d2, 7.7, 1), R.subnormal_near_tie(2, 1),
            R.extreme_resolutions()[7], R.Res("range-edge", R.RANGE_LO)]


def test_z_slab_pipeline(ctx):
    import torch
    scene = entry_scene()
    occ = torch.from_numpy(scene.occupancy()).cuda()
    resolutions = entry_resolutions(scene)
    R.check_targets(scene, resolutions)
    for res in resolutions:
        sdf, lo, hi = multi_gpu.sdf_slabs_single_device(ctx, torch, occ, 3, res.value)
        check("Z-slab pipeline (3 slabs)", scene, res, sdf.cpu().numpy(), lo, hi)


def test_multi_device_entry(ctx):
    scene = entry_scene()
    resolutions = entry_resolutions(scene)
    R.check_targets(scene, resolutions)
    for border in (False, True):
        s = scene.with_border() if border else scene
        for res in resolutions:
            got, lo, hi = capi.sdf_multi([0, 0], s.occupancy(), res.value, True, border)
            check("sdf_multi([0, 0])", s, res, got, lo, hi)


def test_batch_entry(ctx):
    scenes = [entry_scene(), R.complement_scene("entry-holes", (150, 40, 66), [(3, 4, 5), (140, 30, 60)])]
    for res in entry_resolutions(scenes[0]):
        R.check_targets(scenes[0], [res])
        fields, lo, hi = ctx.sdf_batch_from_occupancy([s.occupancy() for s in scenes], res.value)
        for b, s in enumerate(scenes):
            check("sdf_batch_from_occupancy[%d]" % b, s, res, fields[b], float(lo[b]), float(hi[b]))


def test_tagged_cell_entry(ctx):
    scene = entry_scene()
    rec = np.zeros(scene.shape, dtype=capi.TAGGED_OBJECT_CELL)
    rec["occupancy"] = scene.occupancy()
    rec["object_id"][scene.filled] = 1
    cells = ctx.cells(rec, scene.shape)
    try:
        resolutions = entry_resolutions(scene)
        R.check_targets(scene, resolutions)
        for res in resolutions:
            got, lo, hi = cells.sdf(res.value)
            check("tagged cells", scene, res, got, lo, hi)
    finally:
        cells.close()


def test_small_map_ring_entry(ctx):
    """Maps up to 512 KiB run from the context's page-locked ring (40 x 40 x 64 floats = 400 KiB)."""
    scene = R.lattice_scene("ring", (40, 40, 64), R.periodic(40, 13, 2), R.periodic(40, 17, 3), R.periodic(64, 21, 6))
    assert scene.occupancy().nbytes <= 512 * 1024
    d2 = R.pick_d2(scene, 2, 512, 1)[0]
    resolutions = [R.near_tie(d2, 0.3, -1), R.near_tie(d2, 0.3, 1)] + R.extreme_resolutions()[3:8] + R.range_edges()
    run_host(ctx, "host small-map ring", scene, resolutions)
    run_host(ctx, "host small-map ring (virtual border)", scene.with_border(), resolutions[:2] + R.extreme_resolutions()[:2])


def test_device_entry(ctx):
    import torch
    scene = entry_scene()
    shape = scene.shape
    occ = torch.from_numpy(scene.occupancy()).cuda()
    nbytes = capi.sdf_workspace_bytes(shape)
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    resolutions = entry_resolutions(scene)
    R.check_targets(scene, resolutions)
    ctx.set_stream(None)
    try:
        for res in resolutions:
            sdf = torch.empty(shape, dtype=torch.float32, device="cuda")
            minmax = torch.zeros(2, dtype=torch.float32, device="cuda")
            ctx.sdf_dev(occ.data_ptr(), shape, res.value, sdf.data_ptr(), ws.data_ptr(), nbytes, minmax.data_ptr())
            torch.cuda.synchronize()
            lo, hi = (float(v) for v in minmax.cpu().numpy())
            check("sdf_dev", scene, res, sdf.cpu().numpy(), lo, hi)
    finally:
        ctx.reset_stream()
