"""Closed-form cases of the noise estimate, worked by hand; shared by the CPU test (against tests/noise_ref.py)
and the GPU test (against rayz_hip_noise_kat).  Every value is a small integer or a power of two, so every step is exact and the
expected numbers hold for both precisions.  One pixel per case: (name, chunk_sums (K, 1, 3), chunk_sizes, expected)."""
import numpy as np

NAN, INF = float("nan"), float("inf")


def _case(name, sums, sizes, **expect):
    return name, np.asarray(sums, dtype=np.float64).reshape(len(sizes), 1, 3), list(sizes), expect


CASES = [
    # equal chunk sums: D = 0, var = 0.  Q = 3 · 4²/2 = 24 per channel of sum 4
    _case("equal", [[4, 2, 0]] * 3, [2, 2, 2], q=[24.0, 6.0, 0.0], var=0.0, rel2=0.0, unconverged=0),
    # sizes 1 and 1, sums a and b: var = (a - b)²/4 per channel: (3-1)²/4 + (8-2)²/4 + 0 = 1 + 9 = 10
    # m2 = (2² + 5² + 1²) = 30: rel2 = 10/30 is not exact, so it is given as the f64 quotient
    _case("two_singles", [[3, 8, 1], [1, 2, 1]], [1, 1], q=[10.0, 68.0, 2.0], var=10.0, rel2=10.0 / 30.0, unconverged=1),
    # sizes 4 and 2, sums 8 and 1 in red (chunk means 2 and 0.5): Q = 64/4 + 1/2 = 16.5, M = 9, N = 6: D = 16.5 - 81/6 = 3,
    # var = 3 / ((2 - 1) · 6) = 0.5; m2 = 81/36 = 2.25; rel2 = 0.5/2.25 (the f64 quotient)
    _case("unequal_4_2", [[8, 0, 0], [1, 0, 0]], [4, 2], q=[16.5, 0.0, 0.0], var=0.5, rel2=0.5 / 2.25, unconverged=1),
    # one chunk: no estimate yet
    _case("single_chunk", [[1, 2, 3]], [16], q=[1.0 / 16, 4.0 / 16, 9.0 / 16], var=INF, rel2=INF, unconverged=1),
    # an all-zero pixel: var = 0, den = floor2, rel2 = 0: converged through the floor
    _case("all_zero", [[0, 0, 0]] * 2, [16, 16], q=[0.0, 0.0, 0.0], var=0.0, rel2=0.0, unconverged=0),
    # a NaN chunk sum: unconverged, and max_rel2 is a NaN
    _case("nan", [[1, 1, 1], [NAN, 1, 1]], [1, 1], q=[NAN, 2.0, 2.0], var=NAN, rel2=NAN, unconverged=1),
]

# A tiny negative D from rounding, clamped to 0: three equal chunk sums 0.1f of one sample each.  Three equal chunks have no spread,
# but the f32 accumulator rounds 0.1f + 0.1f + 0.1f up, so M·M/3 exceeds Q by about 1.5e-9.  The CPU test asserts that the
# unclamped D of this case IS negative, so that the clamp is what the case exercises (f32 only: in f64 the sums are 0.1, not 0.1f).
CLAMP_CASE = _case("clamp", [[0.1, 0.1, 0.1]] * 3, [1, 1, 1], var=0.0, rel2=0.0, unconverged=0)
