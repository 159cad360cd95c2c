"""The scene and cameras of the sampled G-buffer tests (test_sampled_cpu.py checks on the CPU that their frames show every case the
GPU test relies on; test_sampled_gpu.py runs the kernels on them): a checker ground whose cells fall below a pixel towards the
horizon, a diffuse sphere close to the camera, a glass sphere, a fuzzy metal sphere, one MOVING sphere, one triangle, and sky above
the horizon — seen through a lens focused far behind the near sphere (defocus disk of radius ~0.24) and through a pinhole."""
import numpy as np

from rayz_amd import capi, render, tracer

W, H = 64, 40  # the frame; the other shapes are parts of it or narrower (path ids depend on the width: a reference per width)
SPP = 5
SAMPLES = (1, 2, 5)
SEED = 7
TMIN = 1e-3
GROUND, NEAR, GLASS, METAL, MOVING, TRIANGLE = 0, 1, 2, 3, 4, 5  # hittable indices (spheres, then triangles)
CAMERAS = ("lens", "pinhole")


def build(which: str) -> tracer.Tracer:
    t = tracer.Tracer.init(W, 40.0, 9.0, 3.0 if which == "lens" else 0.0, (0.3, 1.5, 7.5), (0.4, 0.7, 0.0), (0, 1, 0), seed=3)
    P = t.pool
    white, green = P.add_solid_texture((0.9, 0.9, 0.9)), P.add_solid_texture((0.2, 0.3, 0.1))
    checker = P.add_checker_texture(2.0, white, green)
    red, gold, blue = P.add_solid_texture((0.7, 0.2, 0.1)), P.add_solid_texture((0.8, 0.6, 0.2)), P.add_solid_texture((0.1, 0.2, 0.7))
    P.add_sphere((0, -1000, 0), 1000.0, P.add_diffuse(checker))                        # 0 ground
    P.add_sphere((-0.5, 0.4, 5.0), 0.4, P.add_diffuse(red))                            # 1 near the camera: out of focus
    P.add_sphere((1.3, 0.7, 1.5), 0.7, P.add_dielectric(1.5))                          # 2 glass
    P.add_sphere((-1.9, 0.8, 0.5), 0.8, P.add_metallic(gold, 0.3))                     # 3 metal
    P.add_sphere((-0.2, 0.45, 2.6), 0.35, P.add_diffuse(blue), velocity=(1.1, 0.3, 0)) # 4 moving over the shutter
    P.add_triangle((-2.6, 0.0, 3.0), (-1.3, 0.0, 3.6), (-2.0, 1.5, 3.2), P.add_metallic(white, 0.0))  # 5 triangle
    return t


def frame_params(t: tracer.Tracer, precision: int, traversal: int, width: int = W, height: int = H, shard=(0, 1), spp: int = SPP,
                 seed: int = SEED) -> capi.RenderParams:
    p = t.params()
    p.width, p.height, p.precision, p.traversal, p.tmin = width, height, precision, traversal, TMIN
    p.shard_index, p.shard_count = shard
    p.samples_per_px, p.seed, p.max_bounces, p.chunk_spp = spp, seed, 1, 0
    return p


def shape_pixels(width: int, height: int, shard=(0, 1), tile_rows: int = 8):
    """(px, py) of a frame part's entries in output order."""
    rows = render.shard_row_indices(height, tile_rows, shard[0], shard[1])
    py, px = np.meshgrid(rows, np.arange(width), indexing="ij")
    return px.ravel(), py.ravel()


# as chain_scenes.SHAPES: tiled, untiled with lanes past the frame, a shard
SHAPES = {"64x40 tiled": (64, 40, (0, 1)), "50x37 untiled": (50, 37, (0, 1)), "64x40 shard 1 of 3": (64, 40, (1, 3))}


def classes(rec, n: int):
    """The pixel counts the tests assert, of sampled_ref.records' per-sample records, over the first n samples."""
    idx = rec["index"][:, :n]
    hit = idx >= 0
    hits = hit.sum(axis=1)
    kinds = np.array([len(set(r[r >= 0].tolist())) for r in idx])
    moving = (idx == MOVING).sum(axis=1)
    ground = idx == GROUND
    alb = rec["albedo"][:, :n, 0]
    two = np.array([len(set(a[g].tolist())) >= 2 for a, g in zip(alb, ground)])
    return {"hits = n": int((hits == n).sum()), "hits = 0": int((hits == 0).sum()), "0 < hits < n": int(((hits > 0) & (hits < n)).sum()),
            "two hittables": int((kinds >= 2).sum()), "moving sphere hit by some samples": int(((moving > 0) & (moving < n)).sum()),
            "all on the triangle": int((idx == TRIANGLE).all(axis=1).sum()), "all on glass": int((idx == GLASS).all(axis=1).sum()),
            "both checker colours": int(two.sum()), "samples with more than one lens try": int((rec["draws"][:, :n] > 5).sum())}
