"""(gpu) The coarse-hull form of the plain X pass (csrc/edt_sweep_kernels.hip, kCoarse) against the plain kernel and the CPU
oracle, bit for bit, and the choice between the two on the device.

The testing library's switch (set_coarse_hull) runs either kernel on any scene: mode 1 takes the coarse-hull kernel wherever
it applies (lines of more than 64 rows), mode 2 never.  Grids: 97 and 130 rows (three and five subsample rows, a partial
last band), 260, and 1024 (the longest line of 32-bit entries); nz of 70 and 130 leave a last wave with repeated lanes.
Which kernel did the work is read from the number the kernel writes to its scratch head (x_pass_choice): 1 plain, 2 coarse
hull, + 4 when both were enqueued and the device chose.

Mode 0 is the product's rule: both kernels are enqueued where the launch has lines of 512 rows and two rounds of items for
its workgroups, and the share of one-class Z lines among those a sample of pass 1's workgroups counts decides on the device:
the coarse-hull kernel between 18/32 and 27/32, where it was measured to win.  With the workgroups per launch lowered to 16
(set_sweep_slots), (512, 16, 128) is the smallest such shape: 32 items.  A wall across a quarter of the Y positions (a share
of exactly 0.75 whichever lines are counted) must pick the coarse-hull kernel; salt at p = 0.5 (no line holds one class) and
a single small box in empty space (nearly every line does) the plain one.  With the product's 4096 workgroups the same
grid is a launch of one round and gets the plain kernel alone."""
import numpy as np
import pytest

from conftest import bits_equal
from voxelized_geometry_tools_amd import capi, synthetic

pytestmark = pytest.mark.gpu

GRIDS = [(97, 9, 70), (130, 5, 64), (260, 3, 130), (1024, 2, 64)]
SCENES = ["spheres", "salt_0.01", "salt_0.3", "unknown_mix_filled", "unknown_mix_free", "empty", "full", "single",
          "one_class_planes"]
BY_SCENE, COARSE, PLAIN = 0, 1, 2


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0, testing=True)
    c.set_edt_variant(0)
    yield c
    c.set_coarse_hull(BY_SCENE)
    c.set_sweep_slots(0)
    c.close()


@pytest.fixture(scope="module")
def oracle():
    from oracle import oracle as O
    return O


def scene(name, shape):
    """-> (occupancy float32, unknown_is_filled)"""
    if name == "spheres":
        return synthetic.occupancy_spheres(shape, seed=5, num_spheres=6), True
    if name.startswith("salt"):
        return synthetic.occupancy_salt(shape, seed=11, p=float(name.split("_")[1])), True
    if name.startswith("unknown_mix"):
        return synthetic.occupancy_unknown_mix(shape, seed=3), name.endswith("filled")
    if name == "one_class_planes":
        # the middle X planes hold one class, the planes on either side have sites
        occ = synthetic.occupancy_salt(shape, seed=17, p=0.3)
        occ[shape[0] // 3:2 * shape[0] // 3] = 0.0
        return occ, True
    if name == "single":
        occ = np.zeros(shape, dtype=np.float32)
        occ[-1, -1, -1] = 1.0  # (a corner: the far end of every axis)
        return occ, True
    return synthetic.occupancy_degenerate(shape, name), True


def run_on_device(ctx, occ_dev, shape, unknown_is_filled, mode):
    """-> (field on the device, (min, max), which kernel did the X pass)"""
    import torch
    ctx.set_coarse_hull(mode)
    ws_bytes = capi.sdf_workspace_bytes(shape)
    ws_dev = torch.empty(ws_bytes, dtype=torch.uint8, device=occ_dev.device)
    sdf_dev = torch.empty(shape, dtype=torch.float32, device=occ_dev.device)
    minmax_dev = torch.empty(2, dtype=torch.float32, device=occ_dev.device)
    torch.cuda.synchronize()
    ctx.sdf_dev(occ_dev.data_ptr(), shape, 0.25, sdf_dev.data_ptr(), ws_dev.data_ptr(), ws_bytes, minmax_dev.data_ptr(),
                unknown_is_filled, False)
    choice = ctx.x_pass_choice(ws_dev.data_ptr(), shape)
    lo, hi = (float(v) for v in minmax_dev.cpu().numpy())
    return sdf_dev, (lo, hi), choice


@pytest.mark.parametrize("scene_name", SCENES)
@pytest.mark.parametrize("shape", GRIDS, ids=["%dx%dx%d" % g for g in GRIDS])
def test_coarse_and_plain_bit_exact(ctx, oracle, shape, scene_name):
    import torch
    occ, unknown_is_filled = scene(scene_name, shape)
    want, wlo, whi = oracle.sdf_from_occupancy(occ, 0.25, unknown_is_filled=unknown_is_filled)
    occ_dev = torch.from_numpy(occ).to("cuda:0")
    fields = {}
    for mode, kernel in ((COARSE, 2), (PLAIN, 1)):
        sdf_dev, (lo, hi), choice = run_on_device(ctx, occ_dev, shape, unknown_is_filled, mode)
        assert choice == kernel, (shape, scene_name, mode, choice)
        fields[mode] = sdf_dev.cpu().numpy()
        assert bits_equal(fields[mode], want), (shape, scene_name, mode)
        assert (lo, hi) == (wlo, whi), (shape, scene_name, mode)
    assert np.array_equal(fields[COARSE].view(np.uint32), fields[PLAIN].view(np.uint32))


def test_small_launch_by_scene_is_one_plain_launch(ctx):
    """Where the host conditions do not hold (1024 rows, but two items), mode 0 enqueues the plain kernel alone."""
    import torch
    shape = (1024, 2, 64)
    occ_dev = torch.from_numpy(synthetic.occupancy_spheres(shape, seed=5, num_spheres=6)).to("cuda:0")
    _, _, choice = run_on_device(ctx, occ_dev, shape, True, BY_SCENE)
    assert choice == 1


BIG = (512, 16, 128)


@pytest.mark.parametrize("scene_name,kernel", [("wall", 2), ("salt_0.5", 1), ("box", 1)])
def test_device_chooses_by_scene(ctx, scene_name, kernel):
    import torch
    if scene_name == "wall":
        occ_dev = torch.zeros(BIG, dtype=torch.float32, device="cuda:0")
        occ_dev[:, 0:4, 40:60] = 1.0
        occ_dev[200:230, 0:4, :] = 0.0  # (a gap in it: sites far away along X)
        occ_dev[200:230, 0:4, 100:104] = 1.0
    elif scene_name == "box":
        occ_dev = torch.zeros(BIG, dtype=torch.float32, device="cuda:0")
        occ_dev[300:309, 7:9, 60:72] = 1.0
    else:
        generator = torch.Generator(device="cuda:0")
        generator.manual_seed(99)
        occ_dev = (torch.rand(BIG, device="cuda:0", generator=generator) < 0.5).to(torch.float32)
    ctx.set_sweep_slots(16)
    try:
        chosen, chosen_minmax, choice = run_on_device(ctx, occ_dev, BIG, True, BY_SCENE)
    finally:
        ctx.set_sweep_slots(0)
    assert choice == kernel + 4, (scene_name, choice)
    # (one round of items for the product's 4096 workgroups: the plain kernel alone)
    _, _, one_round = run_on_device(ctx, occ_dev, BIG, True, BY_SCENE)
    assert one_round == 1
    plain, plain_minmax, plain_choice = run_on_device(ctx, occ_dev, BIG, True, PLAIN)
    assert plain_choice == 1
    assert torch.equal(chosen.view(torch.int32), plain.view(torch.int32))
    assert chosen_minmax == plain_minmax
    # (and the kernel the device did not choose, forced)
    coarse, coarse_minmax, coarse_choice = run_on_device(ctx, occ_dev, BIG, True, COARSE)
    assert coarse_choice == 2
    assert torch.equal(coarse.view(torch.int32), plain.view(torch.int32))
    assert coarse_minmax == plain_minmax
