"""(gpu) Sweep 2's per-band choice between its two copies of the band code (csrc/edt_sweep_kernels.hip: a full band of an
item with class changes drops the class-change candidates when a wave vote says no lane needs them there), against the
CPU oracle, bit for bit, extrema included.  Scenes on which bands that skip and bands that keep the candidates are
neighbours -- single voxels, plates, a sphere with a line through it, their complements, half spaces that end at band and
word edges -- on shapes whose lines are longer than the short-line kernels take: two Z segments with a partial wave, a
partial band and word, and lines of more than 1024 rows (64-bit entries).  tests/test_sweep_class_bands.py checks the
choice lane by lane on the CPU."""
import numpy as np
import pytest

from conftest import bits_equal
from voxelized_geometry_tools_amd import capi

pytestmark = pytest.mark.gpu

SHAPES = [(160, 176, 72), (150, 144, 64), (1040, 136, 8)]
RESOLUTION = 0.031


def scenes(shape):
    nx, ny, nz = shape
    cx, cy, cz = nx // 2 + 3, ny // 2 - 5, nz // 2
    out = {}
    one = np.zeros(shape, dtype=np.float32)
    one[cx, cy, cz] = 1.0
    out["one_voxel"] = one
    plate = np.zeros(shape, dtype=np.float32)
    plate[cx, :, :] = 1.0
    out["plate_x"] = plate
    plate = np.zeros(shape, dtype=np.float32)
    plate[:, cy, :] = 1.0
    out["plate_y"] = plate
    x, y, z = np.ogrid[:nx, :ny, :nz]
    sphere = ((x - cx) ** 2 + (y - cy) ** 2 + (z - cz) ** 2 <= 20 ** 2).astype(np.float32)
    sphere[:, cy, cz] = 1.0
    sphere[cx, :, cz] = 1.0
    out["sphere_and_lines"] = sphere
    for name in list(out):
        out["not_" + name] = 1.0 - out[name]
    for split in (16, 32):
        half = np.zeros(shape, dtype=np.float32)
        half[:split, :, :] = 1.0  # rows split - 1 / split of the X lines
        half[:, split:, :] = 1.0 - half[:, split:, :]  # ... and of the Y lines
        out["half_%d" % split] = half
    return out


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
    c.close()


@pytest.fixture(scope="module")
def expected():
    """(shape, scene, border) -> (field, min, max) of the oracle: computed once, shared by the tests, never written to."""
    from oracle import oracle as O
    cache = {}

    def get(shape, name, occ, border):
        key = (shape, name, border)
        if key not in cache:
            field, lo, hi = O.sdf_from_occupancy(occ, RESOLUTION, True, border)
            field.setflags(write=False)
            cache[key] = (field, lo, hi)
        return cache[key]
    return get


@pytest.mark.parametrize("shape", SHAPES)
def test_sweeps_vs_oracle(ctx, expected, shape):
    for name, occ in scenes(shape).items():
        for border in (False, True):
            want, wlo, whi = expected(shape, name, occ, border)
            got, lo, hi = ctx.sdf_from_occupancy(occ, RESOLUTION, True, border)
            assert bits_equal(got, want), (shape, name, border)
            assert (lo, hi) == (wlo, whi), (shape, name, border)


@pytest.mark.parametrize("shape", SHAPES)
def test_cross_check_pipeline_agrees(ctx, vctx, shape):
    """The testing library's independent pipeline (EDT variant 1) on the same scenes, against the default pipeline."""
    vctx.set_edt_variant(1)
    try:
        for name, occ in scenes(shape).items():
            for border in (False, True):
                got, lo, hi = ctx.sdf_from_occupancy(occ, RESOLUTION, True, border)
                other, olo, ohi = vctx.sdf_from_occupancy(occ, RESOLUTION, True, border)
                assert bits_equal(got, other), (shape, name, border)
                assert (lo, hi) == (olo, ohi), (shape, name, border)
    finally:
        vctx.set_edt_variant(0)


def test_batch_of_two_grids_on_device(ctx, expected):
    """Two different grids through vgt_hip_sdf_batch_dev: the X pass deals (grid, y, segment) items."""
    import torch
    shape = SHAPES[1]
    all_scenes = scenes(shape)
    names = ["sphere_and_lines", "not_one_voxel"]
    occ = torch.from_numpy(np.stack([all_scenes[n] for n in names])).cuda()
    sdf = torch.empty_like(occ)
    nbytes = capi.sdf_batch_workspace_bytes(2, shape)
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    mm = torch.zeros((2, 2), dtype=torch.float32, device="cuda")
    ctx.set_stream(None)
    try:
        ctx.sdf_batch_dev(occ.data_ptr(), 2, shape, RESOLUTION, sdf.data_ptr(), ws.data_ptr(), nbytes, mm.data_ptr())
        torch.cuda.synchronize()
    finally:
        ctx.reset_stream()
    fields, extrema = sdf.cpu().numpy(), mm.cpu().numpy()
    for b, name in enumerate(names):
        want, wlo, whi = expected(shape, name, all_scenes[name], False)
        assert bits_equal(fields[b], want), name
        assert (float(extrema[b, 0]), float(extrema[b, 1])) == (wlo, whi), name
