"""The scene and cameras of the chain G-buffer tests (test_chain_cpu.py checks on the CPU that they show every case the GPU test
asserts; test_chain_gpu.py runs the kernels on them): twelve hittables — a checker ground, a mirror sphere, metals of fuzz 0.2
and 0.6, a glass ball, a hollow glass ball (an inner sphere of negative radius), a diffuse sphere, a metal and a glass triangle
and two facing mirror triangles 0.3 apart, into whose gap the outside camera looks — and two cameras: one outside, one inside the
glass ball 0.85 from its centre looking along the surface, where most rays are totally reflected."""
import numpy as np

from rayz_amd import capi, render, tracer

W, H = 64, 40  # the frame; every other shape of the tests is a part of it (the camera does not depend on the frame's size)
TMIN = 1e-3
DEPTHS = (0, 1, 4, 16)
MAX_FUZZ = 0.25


def build(which: str) -> tracer.Tracer:
    if which == "outside":
        t = tracer.Tracer.init(W, 50.0, 8.0, 0.0, (0.3, 1.7, 7.5), (0.6, 0.9, 0.0), (0, 1, 0), seed=3)
    else:
        t = tracer.Tracer.init(W, 80.0, 1.0, 0.0, (0.0, 1.0, 0.85), (-1.0, 1.15, 0.75), (0, 1, 0), seed=3)
    P = t.pool
    white, grey = P.add_solid_texture((0.9, 0.9, 0.9)), P.add_solid_texture((0.2, 0.3, 0.1))
    checker = P.add_checker_texture(0.7, white, grey)
    gold, red = P.add_solid_texture((0.8, 0.6, 0.2)), P.add_solid_texture((0.7, 0.2, 0.1))
    glass = P.add_dielectric(1.5)
    mirror = P.add_metallic(white, 0.0)
    P.add_sphere((0, -1000, 0), 1000.0, P.add_diffuse(checker))        # 0  ground
    P.add_sphere((-2.3, 1.0, 0.0), 1.0, P.add_metallic(gold, 0.0))      # 1  mirror sphere
    P.add_sphere((-0.9, 0.5, 2.6), 0.5, P.add_metallic(white, 0.2))     # 2  fuzz 0.2: followed under max_fuzz 0.25
    P.add_sphere((1.0, 0.5, 2.8), 0.5, P.add_metallic(gold, 0.6))       # 3  fuzz 0.6: not followed
    P.add_sphere((0.0, 1.0, 0.0), 1.0, glass)                           # 4  glass ball (the inside camera's)
    P.add_sphere((2.3, 1.0, 0.3), 1.0, glass)                           # 5  hollow glass ball ..
    P.add_sphere((2.3, 1.0, 0.3), -0.8, glass)                          # 6  .. its inner surface
    P.add_sphere((0.3, 0.6, -2.6), 0.6, P.add_diffuse(red))             # 7  diffuse sphere
    P.add_triangle((-4.2, 0.0, 1.0), (-3.2, 0.0, 2.4), (-3.7, 1.6, 1.7), mirror)   # 8  metal triangle
    P.add_triangle((-0.4, 0.0, 4.2), (0.9, 0.0, 4.2), (0.25, 1.2, 4.2), glass)     # 9  glass triangle (one interface)
    P.add_triangle((3.9, 0.0, -3.0), (3.9, 0.0, 3.5), (3.9, 6.0, 0.25), mirror)    # 10 facing mirrors: x = 3.9 ..
    P.add_triangle((4.2, 0.0, 3.5), (4.2, 0.0, -3.0), (4.2, 6.0, 0.25), mirror)    # 11 .. and x = 4.2
    return t


CAMERAS = ("outside", "inside")


def frame_params(t: tracer.Tracer, precision: int, traversal: int, width: int = W, height: int = H, shard=(0, 1)) -> capi.RenderParams:
    p = t.params()
    p.width, p.height, p.precision, p.traversal, p.tmin = width, height, precision, traversal, TMIN
    p.shard_index, p.shard_count = shard
    return p


def shape_pixels(width: int, height: int, shard=(0, 1), tile_rows: int = 8):
    """(px, py) of a frame part's entries in output order."""
    rows = render.shard_row_indices(height, tile_rows, shard[0], shard[1])
    py, px = np.meshgrid(rows, np.arange(width), indexing="ij")
    return px.ravel(), py.ravel()


SHAPES = {"64x40 tiled": (64, 40, (0, 1)), "50x37 untiled": (50, 37, (0, 1)), "64x40 shard 1 of 3": (64, 40, (1, 3))}


def classes(r, max_depth: int):
    """The pixel counts the GPU test asserts, of a chain_ref.chain result."""
    return {"depth >= 2": int((r["depth"] >= 2).sum()),
            "at max_depth on a specular record": int(((r["depth"] == max_depth) & r["specular_end"]).sum()),
            "a miss after a followed hit": int(((r["depth"] >= 1) & (r["index"] < 0)).sum()),
            "stopped by max_fuzz": int(r["fuzz_stop"].sum()),
            "total internal reflection": int(r["tir"].sum())}
