"""Scenes for the footprint-albedo tests: the guides of tests/upscale_scenes.py — whose grounds carry a checker
of cells 1.5 full pixels wide, finer than a low-resolution pixel at every factor — with a low-resolution frame that is what
`render.lowres_camera` traces: the MEAN over each f x f block of albedo_hi x irradiance (1 x irradiance on the background), the
irradiance being smooth over the full frame.

Two things are added to the evaluators' G-buffers so that every rule of §4.24 is met at every size above 1x1:
  * a few low-resolution pixels get an index no full pixel has (a feature only the low-resolution ray saw: n = 0, the albedo comes
    back as it is);
  * the low-resolution albedo of one of them holds a negative zero, so "its bits" is tested as bits."""
import functools

import numpy as np

import upscale_scenes
from upscale_ref import Guides

SIZES = [(1, 1), (2, 1), (33, 9), (65, 33)]  # low-resolution (w, h): what tests/test_footprint_gpu.py runs
FACTORS = (2, 3, 4)
ORPHAN = 900  # the index no full pixel has


def block_mean(a, f):
    """The mean over the f x f blocks of a (H, W, 3) array, in float64."""
    H, W, C = a.shape
    return np.asarray(a, np.float64).reshape(H // f, f, W // f, f, C).mean(axis=(1, 3))


@functools.lru_cache(maxsize=None)
def pair(w, h, f, seed=1, curved=False):
    """dict(rgb_lo, var_lo, g_lo, g_hi, irradiance) for a low-resolution frame of w x h under a full one of f·w x f·h.  Cached: the
    tests share it and must not modify it."""
    s = (upscale_scenes.curved_pair if curved else upscale_scenes.synthetic_pair)(w, h, f, seed)
    g_lo, g_hi = s["g_lo"], s["g_hi"]
    rng = np.random.default_rng([seed, w, h, f, 24])
    W, H = f * w, f * h
    ys, xs = np.mgrid[0:H, 0:W]
    k = rng.uniform(0.5, 2.0, 3)
    irradiance = 1.0 + 0.6 * np.sin(xs[..., None] * (0.11 * k) + 0.3) * np.cos(ys[..., None] * (0.07 * k))  # in 0.4 .. 1.6
    m_hi = np.where(g_hi.index[..., None] < 0, 1.0, g_hi.albedo.astype(np.float64))
    rgb_lo = block_mean(m_hi * irradiance, f).astype(np.float32)
    index_lo, albedo_lo = g_lo.index.copy(), g_lo.albedo.copy()
    if w * h > 2:
        hits = np.argwhere(index_lo >= 0)
        for n, (j, i) in enumerate(hits[rng.choice(len(hits), size=min(3, len(hits)), replace=False)]):
            index_lo[j, i] = ORPHAN
            if n == 0:
                albedo_lo[j, i, 1] = -0.0
    g_lo = Guides(index_lo, g_lo.normal, g_lo.point, albedo_lo)
    for a in (rgb_lo, s["var_lo"], g_lo.index, g_lo.normal, g_lo.point, g_lo.albedo, g_hi.index, g_hi.normal, g_hi.point, g_hi.albedo):
        a.setflags(write=False)
    return dict(rgb_lo=rgb_lo, var_lo=s["var_lo"], g_lo=g_lo, g_hi=g_hi, irradiance=irradiance)
