"""Hand cases for the footprint albedo with answers written down as Fractions and rounded ONCE to float32.

The albedos are dyadic with few bits, so every partial sum of a block is exact in f32 and the only rounding of §4.24 is the divide
s / f32(n): the answer is the rational mean of the matching pixels, rounded once — or a selection (1 for a background pixel, the
low-resolution albedo's bits where nothing matches).  The means below are worked out by hand from each case's picture, not by a
routine that walks the blocks.

A case: name, f, index_lo (h, w) int32, albedo_lo (h, w, 3) float32, index_hi (f·h, f·w), albedo_hi (f·h, f·w, 3), and the answers
`want` (h, w, 3) float32, `want_count` (h, w) uint8."""
from fractions import Fraction as Fr

import numpy as np

import upscale_cases

A = (Fr(1, 4), Fr(1, 2), Fr(1, 8))   # the checker's two colours: R 0.25 / 0.75, G 0.5, B 0.125 / 0.375
B = (Fr(3, 4), Fr(1, 2), Fr(3, 8))


def round32(x):
    """The Fraction x rounded once to the nearest float32, ties to even (normal range; 0 stays 0)."""
    x = Fr(x)
    if x == 0:
        return np.float32(0.0)
    sign, x = (-1, -x) if x < 0 else (1, x)
    e = 0
    while Fr(2) ** (e + 1) <= x:
        e += 1
    while Fr(2) ** e > x:
        e -= 1
    assert -126 <= e <= 127
    ulp = Fr(2) ** (e - 23)
    k, r = divmod(x, ulp)
    k = int(k)
    if r > ulp / 2 or (r == ulp / 2 and k & 1):
        k += 1
    v = np.float32(sign * float(k * ulp))  # (k·ulp has at most 24 significant bits: exact in f64 and in f32)
    assert Fr(float(v)) == sign * k * ulp
    return v


def _f32(rows):
    """A nested list of Fractions (or numbers) as a float32 array; each entry must be a float32 exactly."""
    a = np.array([[[float(c) for c in px] for px in row] for row in rows], np.float32)
    for row_f, row in zip(a, rows):
        for px_f, px in zip(row_f, row):
            assert all(Fr(float(v)) == Fr(c) for v, c in zip(px_f, px)), (px, "is not a float32")
    return a


def _want(rows):
    return np.array([[[round32(c) for c in px] for px in row] for row in rows], np.float32)


def _case(name, f, index_lo, albedo_lo, index_hi, albedo_hi, want, want_count):
    c = dict(name=name, f=f, index_lo=np.array(index_lo, np.int32), albedo_lo=np.ascontiguousarray(albedo_lo, dtype=np.float32),
             index_hi=np.array(index_hi, np.int32), albedo_hi=np.ascontiguousarray(albedo_hi, dtype=np.float32),
             want=np.ascontiguousarray(want, dtype=np.float32), want_count=np.array(want_count, np.uint8))
    h, w = c["index_lo"].shape
    assert c["albedo_lo"].shape == (h, w, 3) and c["index_hi"].shape == (f * h, f * w) and c["albedo_hi"].shape == (f * h, f * w, 3)
    assert c["want"].shape == (h, w, 3) and c["want_count"].shape == (h, w)
    return c


def checker(W, H):
    """A one-pixel checker of the colours A (x + y even) and B (odd), as rows of Fractions."""
    return [[A if (x + y) % 2 == 0 else B for x in range(W)] for y in range(H)]


def cases():
    out = []
    # ---- a one-pixel checker, one surface.  f = 2 and 4: every block holds as many A as B, the mean is (A + B) / 2 = (1/2, 1/2, 1/4).
    half = (Fr(1, 2), Fr(1, 2), Fr(1, 4))
    for f in (2, 4):
        w, h = 3, 2
        out.append(_case(f"checker_f{f}", f, np.zeros((h, w)), _f32([[A] * w] * h), np.zeros((f * h, f * w)), _f32(checker(f * w, f * h)),
                         _want([[half] * w] * h), np.full((h, w), f * f)))
    # f = 3: a block whose corner is A holds 5 A and 4 B, the next one 4 A and 5 B; its corner (3i, 3j) is A where i + j is even.
    # The divide by 9 rounds: R = (5/4 + 12/4) / 9 = 17/36 or (4/4 + 15/4) / 9 = 19/36; G = 1/2; B = (5/8 + 12/8) / 9 = 17/72 or 19/72.
    a5 = (Fr(17, 36), Fr(1, 2), Fr(17, 72))
    b5 = (Fr(19, 36), Fr(1, 2), Fr(19, 72))
    out.append(_case("checker_f3", 3, np.zeros((2, 3)), _f32([[A, B, A], [B, A, B]]), np.zeros((6, 9)), _f32(checker(9, 6)),
                     _want([[a5, b5, a5], [b5, a5, b5]]), np.full((2, 3), 9)))
    # ---- two surfaces in one block; only the LAST pixel in visiting order is the low-resolution pixel's.  The mean of one value is
    # that value: the divide by 1 is exact.
    last = (Fr(5, 8), Fr(3, 16), Fr(7, 8))
    other = (Fr(1, 8), Fr(1, 8), Fr(1, 8))
    out.append(_case("only_the_last_matches_f2", 2, [[7]], _f32([[other]]), [[3, 3], [3, 7]], _f32([[other, other], [other, last]]),
                     _want([[last]]), [[1]]))
    out.append(_case("only_the_last_matches_f3", 3, [[7]], _f32([[other]]), [[3, 3, 3], [3, 3, 3], [3, 3, 7]],
                     _f32([[other] * 3, [other] * 3, [other, other, last]]), _want([[last]]), [[1]]))
    # ---- all sixteen match (f = 4, 1x1).  albedo_hi[y][x] = ((1 + x + 4y) / 64, 1/2, x / 8):
    #   R: (16 + (0 + 1 + .. + 15)) / 64 = 136/64, over 16 = 17/128;  G: 1/2;  B: 4 rows x (0 + 1 + 2 + 3) / 8 = 3, over 16 = 3/16.
    hi = [[(Fr(1 + x + 4 * y, 64), Fr(1, 2), Fr(x, 8)) for x in range(4)] for y in range(4)]
    out.append(_case("all_match_f4", 4, [[0]], _f32([[A]]), np.zeros((4, 4)), _f32(hi), _want([[(Fr(17, 128), Fr(1, 2), Fr(3, 16))]]), [[16]]))
    # ---- a background pixel beside hits (f = 2, 2x1).  Left block: three background pixels and one of surface 0; right block: three
    # of surface 0 and one background.  The background pixel comes out as (1, 1, 1) whatever the albedo arrays hold (9 here) and
    # counts the block's background pixels; the hit takes the mean of ITS three:
    #   R: (1/4 + 1/2 + 3/4) / 3 = 1/2;  G: (1 + 1 + 1/4) / 3 = 3/4;  B: (1/2 + 1/4 + 1/8) / 3 = 7/24 (the divide rounds).
    junk = (Fr(9), Fr(9), Fr(9))
    p0, p1, p2 = (Fr(1, 4), Fr(1), Fr(1, 2)), (Fr(1, 2), Fr(1), Fr(1, 4)), (Fr(3, 4), Fr(1, 4), Fr(1, 8))
    out.append(_case("background_beside_hits", 2, [[-1, 0]], _f32([[junk, A]]), [[-1, 0, 0, 0], [-1, -1, -1, 0]],
                     _f32([[junk, (Fr(5), Fr(5), Fr(5)), p0, p1], [junk, junk, junk, p2]]),
                     _want([[(1, 1, 1), (Fr(1, 2), Fr(3, 4), Fr(7, 24))]]), [[3, 3]]))
    # ---- a hit whose block holds no pixel of its index (a feature only the low-resolution ray saw): the low-resolution albedo
    # comes back with its BITS — 0.3's nearest float32, a negative zero and a NaN with a payload — and the count is 0.
    lo = np.array([[[0x3E99999A, 0x80000000, 0x7FC01234]]], np.uint32).view(np.float32)
    out.append(_case("nothing_matches", 2, [[4]], lo, [[2, 2], [-1, 2]], _f32([[A, B], [junk, A]]), lo, [[0]]))
    # ---- the last row and the last column: a ramp, albedo_hi[y][x] = (x / 8, y / 8, 1/2), so every block's mean names its place.
    #   f = 2 (3x2): R = (2i + 2i + 1) / 2 / 8 = (4i + 1) / 16, G = (4j + 1) / 16.
    #   f = 3 (2x3): R = (3i + 1) / 8, G = (3j + 1) / 8 (the mean of three consecutive numbers is the middle one).
    ramp = lambda W, H: [[(Fr(x, 8), Fr(y, 8), Fr(1, 2)) for x in range(W)] for y in range(H)]  # noqa: E731
    out.append(_case("ramp_to_the_last_row_and_column_f2", 2, np.zeros((2, 3)), _f32([[A] * 3] * 2), np.zeros((4, 6)), _f32(ramp(6, 4)),
                     _want([[(Fr(4 * i + 1, 16), Fr(4 * j + 1, 16), Fr(1, 2)) for i in range(3)] for j in range(2)]), np.full((2, 3), 4)))
    out.append(_case("ramp_to_the_last_row_and_column_f3", 3, np.zeros((3, 2)), _f32([[A] * 2] * 3), np.zeros((9, 6)), _f32(ramp(6, 9)),
                     _want([[(Fr(3 * i + 1, 8), Fr(3 * j + 1, 8), Fr(1, 2)) for i in range(2)] for j in range(3)]), np.full((3, 2), 9)))
    # ---- a low-resolution frame of 1x1 at f = 2: two A and two B.
    out.append(_case("one_by_one_f2", 2, [[0]], _f32([[B]]), np.zeros((2, 2)), _f32(checker(2, 2)), _want([[half]]), [[4]]))
    return out


def capability_case():
    """★ One plane, f = 2, low resolution 4x3.  albedo_hi: the one-pixel checker A / B (block means (1/2, 1/2, 1/4) exactly);
    irradiance E = (2, 1, 1/2); rgb_lo = E x block mean, exact.  `point`: which colour the low-resolution ray happened to see."""
    f, w, h = 2, 4, 3
    E = np.float32((2.0, 1.0, 0.5))
    albedo_hi = _f32(checker(f * w, f * h))
    g_hi = upscale_cases.guides(np.zeros((f * h, f * w), np.int32), 1, albedo_hi)
    rgb_lo = np.broadcast_to(E * np.float32((0.5, 0.5, 0.25)), (h, w, 3)).copy()

    def g_lo(albedo):
        return upscale_cases.guides(np.zeros((h, w), np.int32), f, albedo)

    return dict(f=f, E=E, albedo_hi=albedo_hi, g_hi=g_hi, rgb_lo=rgb_lo, g_lo=g_lo,
                point_A=np.float32([float(c) for c in A]), point_B=np.float32([float(c) for c in B]))
