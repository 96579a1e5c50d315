"""Oracle-free reference for the SDF's final conversion, float32(sqrt(float64(d2)) * resolution), negated on filled voxels
(signed_distance_field_generation.hpp:85-108), and resolutions built to make that conversion hard.

Scenes here have squared distances that numpy computes exactly without any EDT:
  * lattice scenes: the filled voxels are a product set xs x ys x zs of per-axis coordinate sets (a periodic lattice
    {x = ox mod px} x ... is one such set).  A free voxel's squared distance to the nearest site is the sum over the axes
    of the squared distance to the nearest coordinate of that axis's set;
  * a few extra isolated sites on top (brute force over the sites: free d2 = min(lattice, sites));
  * complements: a filled grid with a few free holes (brute force over the holes for the filled voxels);
  * the virtual border: min(d2, b^2), b = distance to the padding layer on the axes of extent > 1.
Every filled voxel of a lattice scene, and every hole of a complement, must have a 6-neighbour of the other class (d2 = 1):
the scene builders check it.

The resolutions are near ties (the product sqrt(d2) * res within a few float64 ulps of a float32 rounding midpoint, for a
d2 the scene contains), exact ties on perfect squares, the edges of the fast conversion's range (1e-30, 1e30), subnormal,
underflow and overflow values.  Each one comes with the d2 it targets; `check_targets` makes a case fail when its scene
does not contain that d2, so that no case can pass without testing what it was built for.

Plain numpy: no oracle, no scipy.  Used by tests/test_oracle_conversion.py (CPU) and tests/test_gpu_sdf_conversion.py."""
import math

import numpy as np

F32_MAX = float(np.finfo(np.float32).max)
# the smallest float64 that rounds to +inf as a float32: FLT_MAX + half an ulp (2^128 - 2^103; a tie, rounded to even = inf)
F32_OVERFLOW = 2.0 ** 128 - 2.0 ** 103
RANGE_LO, RANGE_HI = 1.0e-30, 1.0e30  # the fast conversion's range (edt_device.hpp); outside it the exact one runs


class Scene:
    """filled: bool [nx, ny, nz]; d2: float64 [nx, ny, nz], the exact squared voxel distance to the other class
    (inf: no voxel of the other class anywhere); border: whether d2 includes the virtual border."""

    def __init__(self, name, filled, d2, border=False):
        self.name, self.filled, self.d2, self.border = name, filled, d2, border
        self.shape = filled.shape

    def occupancy(self):
        return self.filled.astype(np.float32)

    def with_border(self):
        return Scene(self.name + "+border", self.filled, np.minimum(self.d2, border_d2(self.shape)), True)

    def expected(self, res):
        return expected_sdf(self.d2, self.filled, res)

    def contains(self, d2, rows=None):
        """Does d2 occur in the scene (optionally: on X rows [rows[0], rows[1]) only)?"""
        d = self.d2 if rows is None else self.d2[rows[0]:rows[1]]
        return bool(np.any(d == d2))


def expected_sdf(d2, filled, res):
    """float32(sqrt(float64(d2)) * res), negated on filled voxels: the reference's conversion."""
    with np.errstate(over="ignore", under="ignore"):
        dist = (np.sqrt(d2.astype(np.float64)) * np.float64(res)).astype(np.float32)
    return np.where(filled, -dist, dist).astype(np.float32)


def extrema(field):
    """(min, max) by value, as Python floats (the library's extrema compare by value: -0.0 == +0.0)."""
    return float(field.min()), float(field.max())


def axis_d2(n, coords):
    """Squared distance of every coordinate 0..n-1 of an axis to the nearest of `coords` (inside [0, n))."""
    coords = np.asarray(sorted(set(int(c) for c in coords)), dtype=np.int64)
    assert coords.size and coords.min() >= 0 and coords.max() < n, "an axis set needs a coordinate inside the grid"
    i = np.arange(n, dtype=np.int64)
    return np.min((i[:, None] - coords[None, :]) ** 2, axis=1), np.isin(i, coords)


def periodic(n, period, offset=0):
    return list(range(offset, n, period))


def _sites_d2(shape, sites):
    """min over `sites` of the squared point distance, for every voxel (brute force; a handful of sites)."""
    x, y, z = (np.arange(s, dtype=np.int64) for s in shape)
    best = np.full(shape, np.inf)
    for sx, sy, sz in sites:
        d = ((x - sx) ** 2)[:, None, None] + ((y - sy) ** 2)[None, :, None] + ((z - sz) ** 2)[None, None, :]
        best = np.minimum(best, d)
    return best


def _has_other_class_neighbour(filled):
    """Per voxel: does any of its 6 neighbours (inside the grid) belong to the other class?"""
    out = np.zeros(filled.shape, dtype=bool)
    for axis in range(3):
        n = filled.shape[axis]
        if n < 2:
            continue
        a = [slice(None)] * 3
        b = [slice(None)] * 3
        a[axis], b[axis] = slice(0, n - 1), slice(1, n)
        diff = filled[tuple(a)] != filled[tuple(b)]
        out[tuple(a)] |= diff
        out[tuple(b)] |= diff
    return out


def lattice_scene(name, shape, xs, ys, zs, extra_sites=()):
    """Filled = xs x ys x zs (per-axis coordinate lists) plus `extra_sites`; exact d2 everywhere."""
    ax, inx = axis_d2(shape[0], xs)
    ay, iny = axis_d2(shape[1], ys)
    az, inz = axis_d2(shape[2], zs)
    filled = inx[:, None, None] & iny[None, :, None] & inz[None, None, :]
    d2 = (ax[:, None, None] + ay[None, :, None] + az[None, None, :]).astype(np.float64)
    if extra_sites:
        d2 = np.minimum(d2, _sites_d2(shape, extra_sites))
        for s in extra_sites:
            filled[s] = True
    if filled.all():
        return uniform_scene(name, shape, True)
    # the nearest free voxel of a site: a neighbour (asserted, not assumed)
    assert _has_other_class_neighbour(filled)[filled].all(), name + ": a site without a free neighbour"
    d2[filled] = 1.0
    return Scene(name, filled, d2)


def complement_scene(name, shape, holes):
    """A filled grid with a few free `holes`: large negative values (the field's minimum)."""
    filled = np.ones(shape, dtype=bool)
    for h in holes:
        filled[h] = False
    d2 = _sites_d2(shape, holes)
    assert _has_other_class_neighbour(filled)[~filled].all(), name + ": a hole without a filled neighbour"
    d2[~filled] = 1.0
    return Scene(name, filled, d2)


def uniform_scene(name, shape, filled):
    """No voxel of the other class: +inf everywhere (all free) or -inf (all filled); finite with the virtual border."""
    return Scene(name, np.full(shape, bool(filled)), np.full(shape, np.inf))


def border_d2(shape):
    """b^2 per voxel, b = distance to the nearest virtual border cell (the padding layer one voxel outside the grid) over
    the axes of extent > 1 (signed_distance_field_generation.hpp:134-284); inf when every extent is 1."""
    b = np.full(shape, np.inf)
    for axis, n in enumerate(shape):
        if n <= 1:
            continue
        i = np.arange(n, dtype=np.float64)
        d = np.minimum(i + 1, n - i)
        view = [1, 1, 1]
        view[axis] = n
        b = np.minimum(b, d.reshape(view))
    return b * b


# ---- resolutions ----

class Res:
    """A resolution, the squared distance it was built for (None: none in particular) and a label for messages."""

    def __init__(self, label, value, target=None):
        self.label, self.value, self.target = label, float(value), target

    def __repr__(self):
        return "%s(res=%r%s)" % (self.label, self.value, "" if self.target is None else ", d2=%d" % self.target)


def _midpoint_above(value):
    """The float32 rounding midpoint just above the float32 nearest `value` (exact in float64)."""
    f = np.float32(value)
    return float(f) + float(np.spacing(f)) / 2.0


def low29(p):
    """The 29 bits of a float64 below the 24-bit float32 mantissa."""
    return int(np.array([p], dtype=np.float64).view(np.uint64)[0] & np.uint64((1 << 29) - 1))


def near_tie(d2, product, nudge=0):
    """res = M / sqrt(d2) for the float32 midpoint M near `product`, moved by `nudge` float64 ulps: sqrt(d2) * res then lies
    within a few ulps of M, below or above it.  Self-checked."""
    m = _midpoint_above(product)
    res = m / np.sqrt(np.float64(d2))
    for _ in range(abs(nudge)):
        res = float(np.nextafter(res, np.inf if nudge > 0 else 0.0))
    p = float(np.sqrt(np.float64(d2)) * np.float64(res))
    assert abs(p - m) <= (abs(nudge) + 4) * float(np.spacing(m)), (d2, product, nudge)
    if abs(m) >= float(np.finfo(np.float32).tiny):
        assert abs(low29(p) - (1 << 28)) <= abs(nudge) + 8, (d2, product, nudge, hex(low29(p)))
    return Res("near-tie", res, d2)


def subnormal_near_tie(d2, k=1, nudge=0):
    """Near tie at the subnormal float32 midpoint M = (k + 1/2) * 2^-149."""
    m = (k + 0.5) * 2.0 ** -149
    res = m / np.sqrt(np.float64(d2))
    for _ in range(abs(nudge)):
        res = float(np.nextafter(res, np.inf if nudge > 0 else 0.0))
    p = float(np.sqrt(np.float64(d2)) * np.float64(res))
    assert abs(p - m) <= (abs(nudge) + 4) * float(np.spacing(m)), (d2, k, nudge)
    return Res("subnormal-near-tie", res, d2)


def square_tie(k, odd_quarter):
    """d2 = k^2 with sqrt(d2) * res EXACTLY on a float32 midpoint in [1, 2): k = 2^a * m (m odd), res = (N / m) * 2^(-24-a)
    for an odd 25-bit N divisible by m, N = 1 (mod 4) (the tie rounds down to even) or 3 (mod 4) (rounds up to even)."""
    a, m = 0, k
    while m % 2 == 0:
        a, m = a + 1, m // 2
    n = (1 << 24) + 12345 * m
    n -= n % m
    while n % 4 != (3 if odd_quarter else 1):
        n += m
    assert (1 << 24) <= n < (1 << 25) and n % m == 0
    res = (n // m) * 2.0 ** (-24 - a)
    p = float(np.float64(k) * np.float64(res))
    assert p == n * 2.0 ** -24 and low29(p) == 1 << 28, (k, n)
    return Res("square-tie", res, k * k)


def range_edges():
    return [Res("range-edge", RANGE_LO), Res("range-edge", float(np.nextafter(RANGE_LO, np.inf))),
            Res("range-edge", float(np.nextafter(RANGE_HI, 0.0))), Res("range-edge", RANGE_HI)]


def extreme_resolutions():
    """Subnormal and underflowing outputs (near ties target d2 = 2, 5, 8: sums of two squares), overflow around
    FLT_MAX + ulp/2 (targets d2 = 4: sqrt exact) and beyond."""
    t = F32_OVERFLOW / 2.0
    out = [Res("subnormal", 1.0e-42), Res("underflow", 1.0e-46), Res("underflow", 5.0e-324),
           subnormal_near_tie(2, 1), subnormal_near_tie(5, 1, nudge=1), subnormal_near_tie(8, 2, nudge=-1),
           Res("overflow-below", float(np.nextafter(t, 0.0)), 4), Res("overflow-at", t, 4),
           Res("overflow-above", float(np.nextafter(t, np.inf)), 4), Res("overflow", 1.7e308)]
    p = [2.0 * r.value for r in out[6:9]]
    assert p[0] < F32_OVERFLOW == p[1] < p[2]
    with np.errstate(over="ignore"):
        assert np.float32(p[0]) == np.float32(F32_MAX) and np.isinf(np.float32(p[1])) and np.isinf(np.float32(p[2]))
    return out


def ordinary_resolutions():
    return [Res("ordinary", 1.0 / 3.0), Res("ordinary", 0.1)]


def near_ties(d2_values, products=(0.3, 7.7, 123.4)):
    """Near ties for each d2, on both sides of the midpoint, at a few magnitudes of the product."""
    out = []
    for i, d2 in enumerate(d2_values):
        product = products[i % len(products)]
        for nudge in (-1, 0, 1):
            out.append(near_tie(d2, product, nudge))
    return out


def pick_d2(scene, lo, hi, count, rows=None, squares=False):
    """Up to `count` distinct d2 in [lo, hi) that occur in the scene (on X rows [rows[0], rows[1]) if given), spread over the
    range; non-squares unless `squares`."""
    d = scene.d2 if rows is None else scene.d2[rows[0]:rows[1]]
    vals = np.unique(d[np.isfinite(d)]).astype(np.int64)
    vals = vals[(vals >= lo) & (vals < hi)]
    is_square = np.array([math.isqrt(int(v)) ** 2 == int(v) for v in vals], dtype=bool)
    vals = vals[is_square] if squares else vals[~is_square]
    if vals.size <= count:
        return [int(v) for v in vals]
    return [int(vals[i]) for i in np.linspace(0, vals.size - 1, count).round().astype(int)]


def check_targets(scene, resolutions, rows=None):
    """Every resolution built for a d2 must find that d2 in the scene (on the given X rows): a case cannot pass vacuously."""
    for r in resolutions:
        if r.target is not None:
            assert scene.contains(r.target, rows), "%s: %r targets a d2 the scene does not contain" % (scene.name, r)


def first_mismatch(got, want):
    """'' when bit-equal, else a short description of the first differing voxel."""
    g = np.ascontiguousarray(got, dtype=np.float32).view(np.uint32)
    w = np.ascontiguousarray(want, dtype=np.float32).view(np.uint32)
    bad = np.argwhere(g != w)
    if bad.size == 0:
        return ""
    i = tuple(int(v) for v in bad[0])
    return "%d voxels differ, first at %s: got %r want %r" % (len(bad), i, float(got[i]), float(want[i]))
