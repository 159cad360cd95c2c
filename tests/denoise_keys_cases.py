"""Exact single-level cases of the denoiser's surface-key rule (an addition to §4.11), in the style of
denoise_cases.py: frames on which every weight but the rule's is 1 — all hits on one plane (n = (0, 0, 1), P = (x, y, 0): wn = wz = 1)
or all background (g = 1), sigma_color = +inf (wc = 1), no demodulation, one level — so a pixel's output is

    out_p = Σ h_q·c_q / Σ h_q   over the taps q inside the frame with key_q == key_p,   h = k[i]·k[j],  k = (1/16, 1/4, 3/8, 1/4, 1/16),

every sum exact in f32 (dyadic colours of few bits) and the quotient rounded once.  `expect()` evaluates that in rationals;
each case's `hand` holds the closed forms of the pixels its docstring works out, which the CPU test holds `expect()` to."""
from fractions import Fraction as F

import numpy as np

from denoise_cases import INF, K, round_f32

PARAMS = dict(levels=1, normal_power_log2=6, flags=0, sigma_color=INF, sigma_plane=0.25)


class KeyCase:
    def __init__(self, name, why, rgb, index, keys, hand):
        self.name, self.why = name, why
        h, w = index.shape
        self.rgb = np.repeat(np.asarray(rgb, np.float32)[..., None], 3, axis=2)
        self.index = np.asarray(index, np.int32)
        self.keys = np.asarray(keys, np.uint32)
        self.normal = np.zeros((h, w, 3), np.float32)
        self.normal[..., 2] = self.index >= 0
        self.point = np.zeros((h, w, 3), np.float32)
        gx, gy = np.meshgrid(np.arange(w), np.arange(h))
        self.point[..., 0], self.point[..., 1] = gx * (self.index >= 0), gy * (self.index >= 0)
        self.hand = hand  # {(y, x): Fraction}: the docstring's closed forms

    def expect(self, keyed=True):
        """{(y, x): Fraction} for every pixel; keyed False: the same frame without the rule."""
        h, w = self.index.shape
        out = {}
        for y in range(h):
            for x in range(w):
                W = S = F(0)
                for j in range(-2, 3):
                    for i in range(-2, 3):
                        qy, qx = y + j, x + i
                        if not (0 <= qy < h and 0 <= qx < w) or (self.index[qy, qx] < 0) != (self.index[y, x] < 0):
                            continue
                        if keyed and self.keys[qy, qx] != self.keys[y, x]:
                            continue
                        W += K[i] * K[j]
                        S += K[i] * K[j] * F(float(self.rgb[qy, qx, 0]))
                out[(y, x)] = S / W
        return out

    def check(self, got, what=""):
        for (y, x), v in self.expect().items():
            want = round_f32(v)
            for c in range(3):
                assert got[y, x, c].view(np.uint32) == want.view(np.uint32), \
                    f"{self.name} {what}: pixel {(y, x)} channel {c}: got {got[y, x, c]!r}, want {want!r} ({self.why})"


def one_among_25():
    """5x5 hits, colour 1 everywhere but 64 at I = (0, 1), the one pixel with key 7 (the others: key 0).  Every pixel's taps all have
    colour 1 once I is skipped: out = 1 exactly; I sees only itself: out = 64.  Without the rule the centre Z = (2, 2) would get
    (1 - 1/64 + 64/64) / 1 = 127/64 (I is its tap i = -1, j = -2: h = 1/4·1/16)."""
    rgb = np.ones((5, 5))
    rgb[0, 1] = 64
    keys = np.zeros((5, 5), np.uint32)
    keys[0, 1] = 7
    hand = {(2, 2): F(1), (0, 1): F(64), (0, 0): F(1), (4, 4): F(1)}
    return KeyCase("one-key-among-25", one_among_25.__doc__, rgb, np.arange(25).reshape(5, 5), keys, hand)


def sign_bit_and_nan_patterns():
    """Keys are compared as 32-bit integers, not as the floats whose slot they ride in: 1x5 hits with keys 0x00000000, 0x80000000 (the
    bits of -0.0, which EQUALS +0.0 as a float), 0x7FC00000, 0x7FC00000 (the bits of a NaN, which differs from ITSELF as a float),
    0x7FC00001 and colours 1, 2, 4, 8, 16.  Pixels 0, 1 and 4 are alone with their keys: 1, 2, 16.  Pixels 2 and 3 share one:
    out_2 = (3/8·4 + 1/4·8) / (5/8) = 28/5, out_3 = (1/4·4 + 3/8·8) / (5/8) = 32/5."""
    keys = np.array([[0x00000000, 0x80000000, 0x7FC00000, 0x7FC00000, 0x7FC00001]], np.uint32)
    hand = {(0, 0): F(1), (0, 1): F(2), (0, 2): F(28, 5), (0, 3): F(32, 5), (0, 4): F(16)}
    return KeyCase("keys-are-integers", sign_bit_and_nan_patterns.__doc__, [[1, 2, 4, 8, 16]], np.arange(5).reshape(1, 5), keys, hand)


def background_taps():
    """1x5 background pixels (g = 1 between them) with colours 1, 6, 100, 6, 1 and keys 0, 0, 5, 0, 0: the rule comes before the
    background rule.  Pixel 2 is alone: 100.  Pixel 0: taps 0 and 1: (3/8·1 + 1/4·6) / (5/8) = 3.  Pixel 1: taps 0, 1 and 3:
    (1/4·1 + 3/8·6 + 1/16·6) / (11/16) = 46/11.  Without the rule pixel 0 would get (3/8 + 6/4 + 100/16) / (11/16) = 130/11."""
    keys = np.array([[0, 0, 5, 0, 0]], np.uint32)
    hand = {(0, 0): F(3), (0, 1): F(46, 11), (0, 2): F(100), (0, 3): F(46, 11), (0, 4): F(3)}
    return KeyCase("background-taps", background_taps.__doc__, [[1, 6, 100, 6, 1]], np.full((1, 5), -1), keys, hand)


def background_and_hits_share_a_key():
    """A key does not replace the background rule: 1x4, pixels 0 and 1 hits, 2 and 3 background, ONE key (9) for all, colours 1, 2, 4, 8.
    out_0 = (3/8·1 + 1/4·2) / (5/8) = 7/5, out_1 = (1/4·1 + 3/8·2) / (5/8) = 8/5, out_2 = (3/8·4 + 1/4·8) / (5/8) = 28/5,
    out_3 = (1/4·4 + 3/8·8) / (5/8) = 32/5."""
    hand = {(0, 0): F(7, 5), (0, 1): F(8, 5), (0, 2): F(28, 5), (0, 3): F(32, 5)}
    return KeyCase("one-key-two-kinds", background_and_hits_share_a_key.__doc__, [[1, 2, 4, 8]], np.array([[0, 1, -1, -1]]),
                   np.full((1, 4), 9, np.uint32), hand)


def cases():
    return [one_among_25(), sign_bit_and_nan_patterns(), background_taps(), background_and_hits_share_a_key()]
