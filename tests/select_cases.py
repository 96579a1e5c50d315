"""Shared inputs of the cell-selection tests (tests/test_select_ref.py, tests/test_gpu_select.py)."""
import numpy as np

# the smallest shapes at which the kernels can go wrong, and what each one exercises
SHAPES = [
    (1, 1, 1), (1, 1, 2),        # degenerate axes
    (1, 70, 1),                  # waves cross lines on every lane
    (3, 3, 3),                   # the minimal stencil
    (2, 2, 64), (2, 3, 65),      # a line equal to a wave, and one over
    (5, 7, 130),                 # waves straddle line ends at changing lanes
    (65, 3, 3),                  # a long X axis
    (96, 96, 130),               # ~1.2 M cells: more blocks than one scan thread's chunk, a ragged last block
]
SMALL_SHAPES = SHAPES[:-1]

_HALF = np.float32(0.5)
# 0.0, 0.5, 1.0, NaN, +-inf and the two neighbours of 0.5
EDGE_VALUES = np.array([0.0, 0.5, 1.0, np.nan, np.inf, -np.inf, np.nextafter(_HALF, np.float32(0)),
                        np.nextafter(_HALF, np.float32(1))], dtype=np.float32)


def random_values(shape, seed):
    rng = np.random.default_rng(seed)
    return EDGE_VALUES[rng.integers(0, len(EDGE_VALUES), size=shape)]


def random_labels(shape, seed):
    """Few distinct labels in blocks, so that some interior cells have equal neighbours and some do not."""
    rng = np.random.default_rng(seed + 1000)
    coarse = rng.integers(1, 4, size=tuple((s + 2) // 3 for s in shape)).astype(np.uint32)
    lab = np.repeat(np.repeat(np.repeat(coarse, 3, 0), 3, 1), 3, 2)
    return np.ascontiguousarray(lab[:shape[0], :shape[1], :shape[2]])


def value_sets(shape, seed=0):
    """name -> (values, labels): random edge values; an all-equal grid (the 26-rule selects nothing, a class mask
    without its class neither); a grid on which mask 15 selects everything under every rule (a 0 / 1 checkerboard with
    all labels distinct -- except that a single cell has no neighbour)."""
    n = int(np.prod(shape))
    x, y, z = np.indices(shape)
    checker = ((x + y + z) % 2).astype(np.float32)
    return {
        "random": (random_values(shape, seed), random_labels(shape, seed)),
        "uniform": (np.zeros(shape, np.float32), np.full(shape, 7, np.uint32)),
        "everything": (checker, np.arange(1, n + 1, dtype=np.uint32).reshape(shape)),
    }


def sdf_field(shape, seed):
    """A signed distance-like field with -0.0, +0.0, NaN and +-inf sprinkled in."""
    rng = np.random.default_rng(seed)
    field = rng.normal(0.0, 1.0, size=shape).astype(np.float32)
    special = np.array([-0.0, 0.0, np.nan, np.inf, -np.inf], dtype=np.float32)
    where = rng.random(shape) < 0.4
    field[where] = special[rng.integers(0, len(special), size=int(where.sum()))]
    return field
