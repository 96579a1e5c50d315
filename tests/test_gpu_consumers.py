"""(gpu) The SDF consumers of csrc/cell_kernels.hip -- coarse gradient, trilinear estimate, fine gradient, local-extrema
map -- against the CPU oracle on every case of tests/consumer_cases.py (non-finite and signed-zero fields, axes of one
and two cells, query points on cell centres, faces and boundaries at four resolutions and in five frames, every branch
of the fine gradient, thresholds, long chains and cycles of the extrema map): doubles bit for bit, NaN placement and
has_value equal.  tests/test_consumer_ref.py pins the oracle on the same cases.  Then the device-pointer entry points,
the optional has_value output, a caller's stream, repeatability of the extrema map, and one field larger than the
kernels' thread cap."""
import numpy as np
import pytest

import consumer_cases as C
from voxelized_geometry_tools_amd import capi

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def oracle():
    from oracle import oracle as O
    return O


def same_doubles(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    nan_a, nan_b = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(nan_a, nan_b) and \
        np.array_equal(a[~nan_a].view(np.uint64), b[~nan_b].view(np.uint64))


FIELD_IDS = ["%s-%s" % (kind, "x".join(map(str, shape))) for kind, shape in C.FIELD_AND_SHAPE]


@pytest.mark.parametrize("kind,shape", C.FIELD_AND_SHAPE, ids=FIELD_IDS)
def test_coarse_gradient_matches_oracle(ctx, oracle, kind, shape):
    for case in C.field_cases([kind], [shape]):
        for edges in (False, True):
            for frame in ("grid", "quarter_turn", "rigid"):
                rot = C.rotation(frame)
                got, has = ctx.sdf_coarse_gradient(case.field, case.resolution, edges, rot)
                want, whas = oracle.coarse_gradient(case.field, case.resolution, edges, rot)
                assert np.array_equal(has, whas), (case.name, edges, frame)
                assert same_doubles(got, want), (case.name, edges, frame)


@pytest.mark.parametrize("kind,shape", C.FIELD_AND_SHAPE, ids=FIELD_IDS)
def test_estimate_matches_oracle(ctx, oracle, kind, shape):
    for case in C.query_cases(kind, shape):
        got, has = ctx.sdf_estimate_distance(case.field, case.resolution, case.queries, case.grid_from_world)
        want, whas = oracle.estimate_distance(case.field, case.resolution, case.queries, case.grid_from_world)
        assert np.array_equal(has, whas), case.name
        assert same_doubles(got, want), case.name


FINE = C.fine_cases()


@pytest.mark.parametrize("case", FINE, ids=[c.name for c in FINE])
def test_fine_gradient_matches_oracle(ctx, oracle, case):
    """The branch sets (tests/test_consumer_ref.py lists how many queries take which branch of ComputeAxisFineGradient:
    minus-only, plus-only and two-sided on each axis, 131 to 2731 queries per set, in the grid frame, after a quarter turn
    and in a general rigid frame), a negative window, an axis thinner than the window, one thrower among good queries and
    queries outside the grid only.  A call with a thrower raises for the whole batch, as the reference throws."""
    want, whas, too_large = oracle.fine_gradient(case.field, case.resolution, case.queries, case.window,
                                                 case.grid_from_world)
    assert too_large == case.raises
    if case.raises:
        with pytest.raises(ValueError, match="Window size"):
            ctx.sdf_fine_gradient(case.field, case.resolution, case.queries, case.window, case.grid_from_world)
        return
    got, has = ctx.sdf_fine_gradient(case.field, case.resolution, case.queries, case.window, case.grid_from_world)
    assert np.array_equal(has, whas), case.name
    assert same_doubles(got, want), case.name
    if case.window < 0:
        positive, phas = ctx.sdf_fine_gradient(case.field, case.resolution, case.queries, -case.window,
                                               case.grid_from_world)
        assert np.array_equal(has, phas) and same_doubles(got, positive)


EXTREMA = C.extrema_cases()


@pytest.mark.parametrize("case", EXTREMA, ids=[c.name for c in EXTREMA])
def test_local_extrema_map_matches_oracle(ctx, oracle, case):
    got = ctx.sdf_local_extrema_map(case.field, case.resolution, case.rotation)
    want = oracle.local_extrema_map(case.field, case.resolution, case.rotation)
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), case.name


@pytest.mark.parametrize("name", C.CYCLE_CASES)
def test_local_extrema_map_repeats_its_bits(ctx, name):
    """Pointer doubling in place and the marking of cycles race by design; the result must not depend on who wins."""
    case = C.extrema_case(name)
    runs = [ctx.sdf_local_extrema_map(case.field, case.resolution, case.rotation) for _ in range(3)]
    assert np.array_equal(runs[0].view(np.uint64), runs[1].view(np.uint64))
    assert np.array_equal(runs[0].view(np.uint64), runs[2].view(np.uint64))


# ---- the device-pointer entry points ----
DEV_FIELDS = [("non_finite", (9, 8, 10)), ("signed_zero", (33, 3, 64)), ("plus_inf", (1, 6, 5)), ("signed_zero", (1, 1, 1))]


def _device(array):
    import torch
    return torch.from_numpy(np.array(array)).cuda()          # (a copy: the cases are read-only)


@pytest.mark.parametrize("kind,shape", DEV_FIELDS, ids=["%s-%s" % (k, "x".join(map(str, s))) for k, s in DEV_FIELDS])
def test_dev_entry_points_equal_the_host_ones(ctx, kind, shape):
    """vgt_hip_sdf_coarse_gradient_dev, _estimate_distance_dev and _local_extrema_map_dev on torch tensors, with and
    without the optional has_value output (NULL: the values are the same and nothing else is written)."""
    import torch
    f = C.field(kind, shape)
    cells = f.size
    sdf = _device(f)
    for res in (0.125, 0.1):
        for frame in ("grid", "rigid"):
            rot, xf = C.rotation(frame), C.grid_from_world(frame)
            # coarse gradient
            want, whas = ctx.sdf_coarse_gradient(f, res, True, rot)
            for with_has in (True, False):
                grad = torch.full((cells, 3), -7.0, dtype=torch.float64, device="cuda")
                has = torch.full((cells,), 0xAB, dtype=torch.uint8, device="cuda")
                torch.cuda.synchronize()
                ctx.sdf_coarse_gradient_dev(sdf.data_ptr(), shape, res, grad.data_ptr(),
                                            has.data_ptr() if with_has else None, True, rot)
                ctx.synchronize()
                assert same_doubles(grad.cpu().numpy().reshape(want.shape), want), (res, frame, with_has)
                assert np.array_equal(has.cpu().numpy().reshape(shape), whas.astype(np.uint8) if with_has else
                                      np.full(shape, 0xAB, np.uint8))
            # no edge gradients: the faces have no value
            want, whas = ctx.sdf_coarse_gradient(f, res, False, rot)
            grad = torch.empty((cells, 3), dtype=torch.float64, device="cuda")
            has = torch.empty((cells,), dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            ctx.sdf_coarse_gradient_dev(sdf.data_ptr(), shape, res, grad.data_ptr(), has.data_ptr(), False, rot)
            ctx.synchronize()
            assert same_doubles(grad.cpu().numpy().reshape(want.shape), want)
            assert np.array_equal(has.cpu().numpy().reshape(shape).astype(bool), whas)
            # estimate
            q = C.to_world(C.grid_queries(shape, res), frame)
            want, whas = ctx.sdf_estimate_distance(f, res, q, xf)
            queries = _device(q)
            for with_has in (True, False):
                out = torch.full((len(q),), -7.0, dtype=torch.float64, device="cuda")
                has = torch.full((len(q),), 0xAB, dtype=torch.uint8, device="cuda")
                torch.cuda.synchronize()
                ctx.sdf_estimate_distance_dev(sdf.data_ptr(), shape, res, queries.data_ptr(), len(q), out.data_ptr(),
                                              has.data_ptr() if with_has else None, xf)
                ctx.synchronize()
                assert same_doubles(out.cpu().numpy(), want), (res, frame, with_has)
                assert np.array_equal(has.cpu().numpy(), whas.astype(np.uint8) if with_has else
                                      np.full(len(q), 0xAB, np.uint8))
            # extrema map
            want = ctx.sdf_local_extrema_map(f, res, rot)
            extrema = torch.full((cells, 3), -7.0, dtype=torch.float64, device="cuda")
            torch.cuda.synchronize()
            ctx.sdf_local_extrema_map_dev(sdf.data_ptr(), shape, res, extrema.data_ptr(), rot)
            assert np.array_equal(extrema.cpu().numpy().reshape(want.shape).view(np.uint64), want.view(np.uint64))
    # no queries: nothing is launched, nothing is written
    out = torch.full((4,), -7.0, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    ctx.sdf_estimate_distance_dev(sdf.data_ptr(), shape, 0.1, None, 0, out.data_ptr())
    ctx.synchronize()
    assert (out.cpu().numpy() == -7.0).all()


def test_dev_entry_points_on_a_callers_stream(ctx, oracle):
    """Occupancy -> field (vgt_hip_sdf_dev) -> the three consumers, all enqueued on a torch stream set with
    ctx.set_stream, with no host synchronisation between producing the field and consuming it."""
    import torch
    from voxelized_geometry_tools_amd import synthetic
    shape, res = (24, 20, 28), 0.05
    occupancy = synthetic.make_occupancy(shape, "spheres", seed=4)
    cells = int(np.prod(shape))
    q = C.grid_queries(shape, res)
    stream = torch.cuda.Stream()
    ctx.set_stream(stream.cuda_stream)
    try:
        with torch.cuda.stream(stream):
            occ = _device(occupancy.astype(np.float32))
            queries = _device(q)
            sdf = torch.empty(shape, dtype=torch.float32, device="cuda")
            nbytes = capi.sdf_workspace_bytes(shape)
            ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device="cuda")
            grad = torch.empty((cells, 3), dtype=torch.float64, device="cuda")
            ghas = torch.empty((cells,), dtype=torch.uint8, device="cuda")
            dist = torch.empty((len(q),), dtype=torch.float64, device="cuda")
            dhas = torch.empty((len(q),), dtype=torch.uint8, device="cuda")
            extrema = torch.empty((cells, 3), dtype=torch.float64, device="cuda")
            ctx.sdf_dev(occ.data_ptr(), shape, res, sdf.data_ptr(), ws.data_ptr(), nbytes)
            ctx.sdf_coarse_gradient_dev(sdf.data_ptr(), shape, res, grad.data_ptr(), ghas.data_ptr(), True)
            ctx.sdf_estimate_distance_dev(sdf.data_ptr(), shape, res, queries.data_ptr(), len(q), dist.data_ptr(),
                                          dhas.data_ptr())
            ctx.sdf_local_extrema_map_dev(sdf.data_ptr(), shape, res, extrema.data_ptr())
            stream.synchronize()
            field = sdf.cpu().numpy()
            got = [t.cpu().numpy() for t in (grad, ghas, dist, dhas, extrema)]
    finally:
        ctx.reset_stream()
    want_field, _, _ = oracle.sdf_from_occupancy(occupancy, res)
    assert np.array_equal(field.view(np.uint32), want_field.view(np.uint32))
    want, whas = oracle.coarse_gradient(field, res, True)
    assert same_doubles(got[0].reshape(want.shape), want) and np.array_equal(got[1].reshape(shape).astype(bool), whas)
    want, whas = oracle.estimate_distance(field, res, q)
    assert same_doubles(got[2], want) and np.array_equal(got[3].astype(bool), whas)
    want = oracle.local_extrema_map(field, res)
    assert np.array_equal(got[4].reshape(want.shape).view(np.uint64), want.view(np.uint64))


def test_coarse_gradient_beyond_the_thread_cap(ctx, oracle):
    """The consumer kernels launch at most 65536 blocks of 256 threads (16.7 M) and stride over the rest: a
    (16384, 33, 32) field, 17.3 M cells, makes the loop go round a second time.  Edge gradients on, device pointers,
    compared with the oracle on the host: 0.3 s on an MI355X, upload and download included.  (The other kernels share
    the loop form.)"""
    import torch
    shape, res = C.STRIDE_SHAPE, 0.05
    f = C.stride_field()
    cells = f.size
    assert 65536 * 256 < cells < 2 * 65536 * 256
    sdf = _device(f)
    grad = torch.empty((cells, 3), dtype=torch.float64, device="cuda")
    has = torch.empty((cells,), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ctx.sdf_coarse_gradient_dev(sdf.data_ptr(), shape, res, grad.data_ptr(), has.data_ptr(), True)
    ctx.synchronize()
    got, got_has = grad.cpu().numpy(), has.cpu().numpy()
    del grad, has, sdf
    want, whas = oracle.coarse_gradient(f, res, True)
    assert got_has.all() and whas.all()
    assert not np.isnan(got).any()
    assert np.array_equal(got.reshape(-1).view(np.uint64), want.reshape(-1).view(np.uint64))
