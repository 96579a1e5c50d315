"""Fields for the surface extraction tests, shared by the reference's own tests and the GPU tests."""
import numpy as np

# shapes where ranks and borders can go wrong: no cubes at all; the smallest grids; 64-sample word boundaries inside a
# line and at line ends; more than one block of the scans (1024 samples each)
FLAT_SHAPES = [(1, 5, 5), (5, 1, 5), (5, 5, 1)]
SHAPES = [(2, 2, 2), (3, 3, 3), (4, 5, 64), (4, 5, 65), (3, 3, 130), (17, 9, 70)]
FIELDS = ["blob", "noise", "open", "equal", "iso037", "occupancy", "nonfinite"]


def _seed(shape, salt):
    return (shape[0] * 1000003 + shape[1] * 1009 + shape[2]) * 16 + salt


def _distance(shape, centre, scale=(1.0, 1.0, 1.0)):
    axes = np.meshgrid(*[np.arange(n, dtype=np.float64) for n in shape], indexing="ij")
    return np.sqrt(sum(((a - c) * s) ** 2 for a, c, s in zip(axes, centre, scale)))


def field(kind, shape):
    """-> (values float32, iso, inside_above)."""
    rng = np.random.default_rng(_seed(shape, FIELDS.index(kind)))
    centre = [(n - 1) / 2.0 + 0.21 for n in shape]
    if kind == "blob":  # a smooth closed surface inside the grid where the grid is large enough for one
        radius = 0.37 * (min(shape) - 1) + 0.3
        return (_distance(shape, centre, [min(shape) / n for n in shape]) - radius).astype(np.float32), 0.0, False
    if kind == "noise":  # nearly every cube is active and nearly every edge crosses
        return rng.uniform(-1.0, 1.0, shape).astype(np.float32), 0.0, False
    if kind == "open":  # a slanted plane: the surface runs out of the grid
        axes = np.meshgrid(*[np.arange(n, dtype=np.float64) for n in shape], indexing="ij")
        plane = 0.31 * axes[0] + 0.23 * axes[1] + 0.11 * axes[2]
        return (plane - 0.5 * plane.max() - 0.013).astype(np.float32), 0.0, False
    if kind == "equal":  # values equal to iso exactly: they are outside, and t is 0 or 1 on their edges
        return rng.integers(-1, 2, shape).astype(np.float32), 0.0, False
    if kind == "iso037":
        values = _distance(shape, centre) * 0.25 + rng.uniform(-0.2, 0.2, shape)
        return values.astype(np.float32), float(np.float32(0.37)), False
    if kind == "occupancy":
        return rng.choice(np.array([0.0, 0.5, 1.0], dtype=np.float32), shape), 0.5, True
    if kind == "nonfinite":  # void cubes, suppressed quads
        values = rng.uniform(-1.0, 1.0, shape).astype(np.float32)
        bad = rng.random(shape) < 0.02
        values[bad] = rng.choice(np.array([np.nan, np.inf, -np.inf], dtype=np.float32), int(bad.sum()))
        if not bad.any():
            values.flat[values.size // 2] = np.nan
        return values, 0.0, False
    raise ValueError(kind)


def rotation_and_translation():
    """A world_from_grid with a rotation about a skew axis and a translation, 16 doubles column-major."""
    axis = np.array([0.3, -0.5, 0.8])
    axis /= np.linalg.norm(axis)
    angle = 0.7
    k = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    m = np.eye(4)
    m[:3, :3] = np.eye(3) + np.sin(angle) * k + (1 - np.cos(angle)) * (k @ k)
    m[:3, 3] = [1.25, -0.5, 3.0]
    return np.ascontiguousarray(m.T).reshape(16)


def solid(kind, n=24):
    """A voxelized body as a boolean (n, n, n) grid: 'sphere', 'torus' (genus 1) or 'shell' (a hollow sphere: two
    surfaces).  All of them stay clear of the grid's faces."""
    c = (n - 1) / 2.0
    x, y, z = np.meshgrid(*[np.arange(n, dtype=np.float64) - c] * 3, indexing="ij")
    r = np.sqrt(x * x + y * y + z * z)
    if kind == "sphere":
        return r <= 0.33 * n
    if kind == "torus":
        return (np.sqrt(x * x + y * y) - 0.27 * n) ** 2 + z * z <= (0.11 * n) ** 2
    if kind == "shell":
        return (r <= 0.38 * n) & (r >= 0.2 * n)
    raise ValueError(kind)


SOLIDS = {"sphere": 2, "torus": 0, "shell": 4}  # the Euler characteristic of their surfaces


def salt(n=12, share=0.3, seed=5):
    """`share` of the cells filled at random, none on the grid's faces: a closed but non-manifold surface."""
    filled = np.random.default_rng(seed).random((n, n, n)) < share
    inner = np.zeros_like(filled)
    inner[1:-1, 1:-1, 1:-1] = True
    return filled & inner


def signed_edt(filled):
    """scipy's Euclidean distance transform as a signed field in cells: negative inside, positive outside, never 0."""
    from scipy.ndimage import distance_transform_edt
    return (distance_transform_edt(~filled) - distance_transform_edt(filled)).astype(np.float32)
