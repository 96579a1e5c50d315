"""(gpu) Sweep 2's sign words, taken in blocks of several words (csrc/edt_sweep_kernels.hip), against the CPU oracle, bit for
bit, extrema included.  Lines whose class changes sit where a mistake in the block bookkeeping would show: none at all, one
change at the first or the last row of a word -- of every word, the seams between blocks among them -- and a
change at every row -- as lines of the X pass (shapes (n, 3, 65)) and of the Y pass ((3, n, 65)), with lengths around whole
words and blocks, all above the short-line kernels' limit, 1100 rows for the kernels with 64-bit entries, with and without
the virtual border; and a batch of three grids.  tests/test_sweep_sign_blocks.py runs the same lines lane by lane on the
CPU, where every use of a sign word is checked against what sweep 1 wrote."""
import numpy as np
import pytest

from conftest import bits_equal
from voxelized_geometry_tools_amd import capi

pytestmark = pytest.mark.gpu

LENGTHS = [129, 130, 159, 160, 161, 255, 256, 257, 383, 1024, 1100]
RESOLUTION = 0.031
WORD = 32


def line_patterns(n):
    """Class patterns (0 / 1 per row) of lines of n rows."""
    rows = np.arange(n)
    out = [np.zeros(n, dtype=np.uint8), np.ones(n, dtype=np.uint8), (rows & 1).astype(np.uint8)]
    nwords = (n + WORD - 1) // WORD
    seams = set()
    for w in range(nwords):
        seams.add(w * WORD)                  # rows 32 w - 1 | 32 w: the change is at the first row of word w
        seams.add(w * WORD + WORD - 1)       # rows 32 w + 30 | 32 w + 31: at its last row
    # (every word edge is there, so every seam between two blocks is, whatever the block size and the end it is counted from)
    for s in sorted(seams):
        if 0 < s < n:
            out.append((rows >= s).astype(np.uint8))
    return out


def grid_of_lines(n, axis):
    """Occupancy whose lines along `axis` (0: X pass, 1: Y pass) run through the patterns, one per (other index, z)."""
    patterns = line_patterns(n)
    shape = (n, 3, 65) if axis == 0 else (3, n, 65)
    occ = np.zeros(shape, dtype=np.float32)
    for other in range(3):
        for z in range(65):
            # (the first plane: one class per line, so the planes differ and lines without a change have neighbours)
            line = patterns[(other * 65 + z * 7) % len(patterns)].astype(np.float32)
            if axis == 0:
                occ[:, other, z] = line
            else:
                occ[other, :, z] = line
    return occ


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


# (1100 rows: lines of the X pass only)
CASES = [(n, 0) for n in LENGTHS] + [(n, 1) for n in LENGTHS if n <= 1024]


@pytest.mark.parametrize("n,axis", CASES)
def test_lines_vs_oracle(ctx, n, axis):
    from oracle import oracle as O
    occ = grid_of_lines(n, axis)
    for border in (False, True):
        want, wlo, whi = O.sdf_from_occupancy(occ, RESOLUTION, True, border)
        got, lo, hi = ctx.sdf_from_occupancy(occ, RESOLUTION, True, border)
        assert bits_equal(got, want), (n, axis, border)
        assert (lo, hi) == (wlo, whi), (n, axis, border)


def test_batch_of_three_grids_on_device(ctx):
    """Three grids of (130, 67, 129) through vgt_hip_sdf_batch_dev: lines with a change at every word edge, an empty grid (the
    fill path of every item) and a grid with a single filled voxel (planes without any site next to planes with one)."""
    import torch
    from oracle import oracle as O
    shape = (130, 67, 129)
    x, y, z = np.ogrid[:shape[0], :shape[1], :shape[2]]
    edges = (((x // WORD) + (y // WORD) + z) & 1).astype(np.float32) * np.ones(shape, dtype=np.float32)
    empty = np.zeros(shape, dtype=np.float32)
    one = np.zeros(shape, dtype=np.float32)
    one[127, 33, 64] = 1.0
    grids = [edges, empty, one]
    occ = torch.from_numpy(np.stack(grids)).cuda()
    sdf = torch.empty_like(occ)
    nbytes = capi.sdf_batch_workspace_bytes(3, shape)
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    mm = torch.zeros((3, 2), dtype=torch.float32, device="cuda")
    ctx.set_stream(None)
    try:
        ctx.sdf_batch_dev(occ.data_ptr(), 3, shape, RESOLUTION, sdf.data_ptr(), ws.data_ptr(), nbytes, mm.data_ptr())
        torch.cuda.synchronize()
    finally:
        ctx.reset_stream()
    fields, extrema = sdf.cpu().numpy(), mm.cpu().numpy()
    for b, grid in enumerate(grids):
        want, wlo, whi = O.sdf_from_occupancy(grid, RESOLUTION, True, False)
        assert bits_equal(fields[b], want), b
        assert (float(extrema[b, 0]), float(extrema[b, 1])) == (wlo, whi), b
