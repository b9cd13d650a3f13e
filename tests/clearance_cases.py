"""Inputs shared by tests/test_clearance_cpu.py and tests/test_gpu_clearance.py."""
import numpy as np

X = 16
TR, CHUNK = 16, 256      # k_clear: own rows a workgroup, columns a pass (lqro_kern_clear.hip)
LATTICE_RADII = (0.5, 0.25)   # a = 1, b = 0.5: the weights are 1 and 4 exactly


def states(pos, x_dim=X):
    pos = np.asarray(pos, np.float64).reshape(-1, 3)
    x = np.zeros((pos.shape[0], x_dim))
    x[:, :3] = pos
    if x_dim == 16:
        x[:, 12:16] = 9.80665 * 0.500 / 4
    return x


def lattice(scale=1.0):
    """4 x 4 x 4 points, spacing 1.0 in x and y and 0.5 in z, times scale:
    with LATTICE_RADII every axis neighbour has s2 == scale^2 exactly."""
    g = np.arange(4, dtype=np.float64)
    p = np.stack(np.meshgrid(g * 1.0, g * 1.0, g * 0.5, indexing="ij"), axis=-1).reshape(-1, 3)
    return p * scale


def lattice_axis_neighbours():
    """Per lattice point (in lattice() order), its number of axis neighbours."""
    idx = np.stack(np.meshgrid(*[np.arange(4)] * 3, indexing="ij"), axis=-1).reshape(-1, 3)
    return ((idx > 0).sum(axis=1) + (idx < 3).sum(axis=1)).astype(np.int32)


def random_positions(n, seed, box=None):
    rng = np.random.default_rng(seed)
    side = box if box is not None else 1.6 * n ** (1.0 / 3.0)
    return (rng.random((n, 3)) - 0.5) * side


def cluster(n, seed, centre=(0.0, 0.0, 0.0), radius=0.1):
    """n points within `radius` of each other's centre box."""
    rng = np.random.default_rng(seed)
    return np.asarray(centre) + (rng.random((n, 3)) - 0.5) * radius


def same_total(a, b):
    """Two totals (dicts) equal in every field, the doubles bit for bit."""
    for k in a:
        va, vb = a[k], b[k]
        if isinstance(va, float) or isinstance(vb, float):
            if np.float64(va).view(np.uint64) != np.float64(vb).view(np.uint64):
                return False
        elif int(va) != int(vb):
            return False
    return set(a) == set(b)


def same_rows(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
