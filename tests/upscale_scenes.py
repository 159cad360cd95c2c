"""An analytic screen-space scene for the upscaler tests, evaluated at the full-size pixel centres and at the low-resolution pixel
centres, so that the two G-buffers agree the way two camera queries of one scene would (low-resolution pixel
(i, j) looks at the centre of its f x f block).

The scene, in full-pixel units (X, Y) over [0, W) x [0, H):
  - a tilted ground plane with a checker albedo of cells 1.5 full pixels wide (one colour has a channel below the 2^-8 clamp);
  - a second plane of another orientation right of X = 0.6·W, and a third, parallel to the ground but far off it, below Y = 0.7·H;
  - a background region above Y = 0.18·H (index -1, zero guides, as a camera query writes a miss);
  - thin strips, each one full pixel wide and far off every other surface along the ground's normal: slanted ones (x = x0 + y div k),
    which the low-resolution samples hit only every few rows — the pixels between two hits find their surface in the 4x4 footprint
    only (stage 1) or not at all (stage 2) —, and vertical ones that fall between the low-resolution samples (stage 2).
Colours and variances are random (no dyadic structure); a few variances are +inf ("no estimate yet").

Every surface above is flat, so a guide weight is 1 within a surface and 0 across two.  `curved_pair` (below) is the scene with
weights in between: spheres, evaluated at the full pixel centres, the block centres or the samples of a lattice."""
import numpy as np

from upscale_ref import Guides

SIZES = [(1, 1), (1, 7), (7, 1), (5, 3), (17, 9), (33, 5), (65, 33)]  # low-resolution (w, h): what tests/test_upscale_gpu.py runs
FACTORS = (2, 3, 4)


def _unit(v):
    v = np.asarray(v, np.float64)
    return v / np.sqrt((v * v).sum())


def _frame(n):
    """Two unit vectors spanning the plane of normal n."""
    u = _unit(np.cross(n, (0.0, 1.0, 0.3)))
    return u, np.cross(n, u)


def _evaluate(X, Y, W, H, rng_consts):
    """The scene at the screen positions X, Y (arrays of one shape): index, normal, point, albedo."""
    n0, n1, strips, a_even, a_odd, a_other = rng_consts
    shape = X.shape
    index = np.zeros(shape, np.int32)
    normal = np.broadcast_to(n0, shape + (3,)).copy()
    u0, v0 = _frame(n0)
    origin = np.array((0.3, -1.7, 5.1))
    point = origin + X[..., None] * 0.37 * u0 + Y[..., None] * 0.37 * v0
    cell = (np.floor(X / 1.5) + np.floor(Y / 1.5)).astype(np.int64) & 1
    albedo = np.where(cell[..., None] == 1, a_odd, a_even)
    # the second plane: another orientation, through the same screen positions
    m = X >= 0.6 * W
    u1, v1 = _frame(n1)
    index[m] = 1
    normal[m] = n1
    point[m] = (origin + X[..., None] * 0.37 * u1 + Y[..., None] * 0.37 * v1)[m]
    albedo[m] = a_other
    # the third: parallel to the ground, 40 units off it
    m = (Y >= 0.7 * H) & (X < 0.6 * W)
    index[m] = 2
    point[m] = (point + 40.0 * n0)[m]
    # the strips: parallel to the ground, each at a depth of its own
    xi, yi = np.floor(X).astype(np.int64), np.floor(Y).astype(np.int64)
    for s, (x0, k) in enumerate(strips):
        m = xi == (x0 + (yi // k if k else 0))
        index[m] = 3 + s
        normal[m] = n0
        point[m] = (origin + X[..., None] * 0.37 * u0 + Y[..., None] * 0.37 * v0 - (100.0 + 30.0 * s) * n0)[m]
        albedo[m] = a_even
    # the background
    m = Y < 0.18 * H
    index[m] = -1
    normal[m] = 0.0
    point[m] = 0.0
    albedo[m] = 0.0
    return Guides(index, normal.astype(np.float32), point.astype(np.float32), albedo.astype(np.float32))


def synthetic_pair(w, h, f, seed):
    """dict(rgb_lo, var_lo, g_lo, g_hi) for a low-resolution frame of w x h pixels under a full one of f·w x f·h."""
    rng = np.random.default_rng([seed, w, h, f])
    W, H = f * w, f * h
    n0 = _unit((0.21, -0.93, 0.31))
    n1 = _unit((-0.72, -0.15, 0.66))
    strips = [(int(rng.integers(0, max(W // 2, 1))), 4), (int(rng.integers(0, max(W // 2, 1))), 3), (int(rng.integers(0, W)), 0),
              (int(rng.integers(0, W)), 0), (int(rng.integers(0, max(W - H // 7, 1))), 7)]
    consts = (n0, n1, strips, np.array((0.83, 0.79, 0.71)), np.array((0.9, 0.001, 0.31)), np.array((0.47, 0.52, 0.12)))
    xs, ys = np.meshgrid(np.arange(W) + 0.5, np.arange(H) + 0.5)
    g_hi = _evaluate(xs, ys, W, H, consts)
    xs, ys = np.meshgrid((np.arange(w) + 0.5) * f, (np.arange(h) + 0.5) * f)
    g_lo = _evaluate(xs, ys, W, H, consts)
    irradiance = rng.uniform(0.05, 2.0, (h, w, 3))
    rgb_lo = (np.where(g_lo.index[..., None] < 0, 1.0, g_lo.albedo) * irradiance).astype(np.float32)
    var_lo = (rng.uniform(0.0, 0.2, (h, w, 3)) ** 2).astype(np.float32)
    var_lo[rng.uniform(size=(h, w)) < 0.05] = np.inf
    return dict(rgb_lo=rgb_lo, var_lo=var_lo, g_lo=g_lo, g_hi=g_hi)


# ---- a curved scene: guide weights between 0 and 1 (tests/upscale_f64.py, tests/test_upscale_f64_*.py)
_S = 0.37        # world units per full pixel
_GAP = 300.0     # world units between two surfaces' depths: every silhouette is a step far larger than any sphere


def _evaluate_curved(X, Y, W, H, consts):
    """The curved scene at the screen positions X, Y: an orthographic view along +z of spheres as height fields (analytic normals
    and points, an albedo that varies with the normal), each at a depth of its own, in front of a tilted checkered ground below the
    horizon Y = 0.45·H and of the background above it; in front of everything, spheres smaller than a low-resolution pixel and thin
    slanted strips (the features the low-resolution samples miss: stages 1 and 2)."""
    spheres, strips, a_even, a_odd = consts
    shape = X.shape
    K = len(spheres)
    # the ground, behind everything
    ng = _unit((0.1, 0.4, -1.0))
    index = np.zeros(shape, np.int32)
    normal = np.broadcast_to(ng, shape + (3,)).copy()
    zg = _GAP * (K + 2) + _S * (0.4 * Y + 0.1 * X)  # (ng is this height field's normal)
    point = np.stack([_S * X, _S * Y, zg], axis=-1)
    cell = (np.floor(X / 1.5) + np.floor(Y / 1.5)).astype(np.int64) & 1
    albedo = np.where(cell[..., None] == 1, a_odd, a_even)
    ground_point = point.copy()
    # the background above the horizon
    m = Y < 0.45 * H
    index[m] = -1
    normal[m] = 0.0
    point[m] = 0.0
    albedo[m] = 0.0
    # the spheres, far to near
    for k in range(K - 1, -1, -1):
        cx, cy, R, base = spheres[k]
        dx, dy = X - cx, Y - cy
        hz2 = R * R - dx * dx - dy * dy
        m = hz2 > 0
        hz = np.sqrt(np.where(m, hz2, 1.0))
        n = np.stack([dx, dy, -hz], axis=-1) / R
        index[m] = 1 + k
        normal[m] = n[m]
        point[m] = np.stack([_S * X, _S * Y, _GAP * (k + 1) - _S * hz], axis=-1)[m]
        albedo[m] = (np.asarray(base) * (0.55 + 0.45 * n[..., :1] * n[..., 1:2] - 0.3 * n[..., 2:3] * n[..., :1]))[m]
    # the strips: parallel to the ground, each far in front of it at a depth of its own
    xi, yi = np.floor(X).astype(np.int64), np.floor(Y).astype(np.int64)
    for s, (x0, k) in enumerate(strips):
        m = xi == (x0 + yi // k)
        index[m] = 100 + s
        normal[m] = ng
        point[m] = (ground_point - (1000.0 + 30.0 * s) * ng)[m]
        albedo[m] = a_even
    return Guides(index, normal.astype(np.float32), point.astype(np.float32), albedo.astype(np.float32))


def curved_pair(w, h, f, seed, phase=None):
    """As `synthetic_pair`, on the curved scene.  `phase` None: the low-resolution guides are the scene at the block centres;
    (px, py): at the lattice samples (f·i + px, f·j + py), where they ARE the full G-buffer's (DESIGN.md §4.20 "Lattice samples")."""
    rng = np.random.default_rng([seed, w, h, f, 77])
    W, H = f * w, f * h
    rmax = min(25.0, max(9.0, 0.6 * max(W, H)))
    spheres = [(rng.uniform(0.0, W), rng.uniform(0.0, H), R, rng.uniform(0.25, 0.95, 3))
               for R in np.linspace(rmax, 6.0, max(2, min(12, round(W * H / 600))))]
    # smaller than a low-resolution pixel, centred on a full pixel's centre so that it is seen at all
    spheres = [(int(rng.integers(0, W)) + 0.5, int(rng.integers(0, H)) + 0.5, 0.45 * f, rng.uniform(0.25, 0.95, 3))
               for _ in range(max(2, W * H // 400))] + spheres
    strips = [(int(rng.integers(0, max(W // 2, 1))), 4), (int(rng.integers(0, max(W // 2, 1))), 3), (int(rng.integers(0, max(W - H // 7, 1))), 7)]
    consts = (spheres, strips, np.array((0.83, 0.79, 0.71)), np.array((0.9, 0.001, 0.31)))
    xs, ys = np.meshgrid(np.arange(W) + 0.5, np.arange(H) + 0.5)
    g_hi = _evaluate_curved(xs, ys, W, H, consts)
    if phase is None:
        xs, ys = np.meshgrid((np.arange(w) + 0.5) * f, (np.arange(h) + 0.5) * f)
    else:
        xs, ys = np.meshgrid(f * np.arange(w) + phase[0] + 0.5, f * np.arange(h) + phase[1] + 0.5)
    g_lo = _evaluate_curved(xs, ys, W, H, consts)
    irradiance = rng.uniform(0.05, 2.0, (h, w, 3))
    rgb_lo = (np.where(g_lo.index[..., None] < 0, 1.0, g_lo.albedo) * irradiance).astype(np.float32)
    var_lo = (rng.uniform(0.0, 0.2, (h, w, 3)) ** 2).astype(np.float32)
    var_lo[rng.uniform(size=(h, w)) < 0.05] = np.inf
    return dict(rgb_lo=rgb_lo, var_lo=var_lo, g_lo=g_lo, g_hi=g_hi)
