"""Adaptive passes worked by hand: one run of six pixels whose every answer is an exact binary fraction.

Chunks of 2, 2, 4, 8, 16, 32 samples (boundaries 2, 4, 8, 16, 32, 64: every N is a power of two, so acc · (1/N) is exact); passes
end after 2, 3, 4, 5 and 6 chunks; min_chunks 3, rel_error 0.3 (tau2 = 0.09), mean_floor 0.02.  Only red carries a signal, so
var = D_r / ((K − 1) N) and m2 = (M_r / N)².  Per pixel, the red chunk sums and the evaluation at each boundary it is evaluated at:

 0  first eligible boundary   1, 3, 4 | 80, 80, 80
      K=2: Q = 1/2 + 9/2 = 5, M = 4, N = 4: D = 5 − 4 = 1, var = 1/4, m2 = 1, rel2 = 0.25 > 0.09 (and 2 < min_chunks)
      K=3: Q = 5 + 16/4 = 9, M = 8, N = 8: D = 9 − 8 = 1, var = 1/16, m2 = 1, rel2 = 0.0625 <= 0.09: freezes at 3 on 8/8 = 1.
      The 80s are never folded: acc stays 8, Q stays 9.
 1  would pass at K=2        2, 2, 8 | ..
      K=2: Q = 2 + 2 = 4, M = 4, N = 4: D = 0, rel2 = 0 — converged, but 2 < min_chunks: it must wait
      K=3: Q = 4 + 64/4 = 20, M = 12, N = 8: D = 20 − 18 = 2, var = 2/16, m2 = 2.25, rel2 = 0.0555.. <= 0.09: freezes at 3 on 12/8 =
      1.5 (had it frozen at 2 it would show 1.0)
 2  never freezes            0, 4, 0, 16, 0, 64
      rel2 = 1, 1.5, 0.2, 0.55, 0.1047.. at K = 2 .. 6 (K=6: Q = 168, M = 84, N = 64, D = 57.75, var = 57.75/320, m2 = 7056/4096):
      all > 0.09.  It ends on the full mean 84/64 = 1.3125.
 3  NaN                      nan, 1, 1, 1, 1, 1     every rel2 is a NaN, NaN <= tau2 is false: never freezes; the frame's red is a NaN
 4  black                    0 ..                   D = 0, m2 = 0 < floor2: rel2 = 0/floor2 = 0: freezes at 3 on 0
 5  frozen != full mean      2, 2, 4 | 8, 16, 96    as pixel 1 with D = 0 at K = 3 too (Q = 8, M = 8, N = 8): freezes at 3 on 1.0,
                                                    while the mean of all 64 samples is 128/64 = 2.0

Lists: pass 0 and pass 1 trace all six; passes 2, 3, 4 trace [2, 3]; [2, 3] are left."""
import numpy as np

NAN = float("nan")
SIZES = [2, 2, 4, 8, 16, 32]
PASS_ENDS = [2, 3, 4, 5, 6]
PARAMS = {"min_chunks": 3, "rel_error": 0.3, "mean_floor": 0.02}
RED = [[1, 3, 4, 80, 80, 80],
       [2, 2, 8, 80, 80, 80],
       [0, 4, 0, 16, 0, 64],
       [NAN, 1, 1, 1, 1, 1],
       [0, 0, 0, 0, 0, 0],
       [2, 2, 4, 8, 16, 96]]
SUMS = np.zeros((6, 6, 3))          # (chunk, pixel, channel)
SUMS[:, :, 0] = np.asarray(RED).T

WANT_FROZEN_AT = [3, 3, 0, 0, 3, 3]
WANT_COUNTS = [8, 8, 64, 64, 8, 8]
WANT_RED = [1.0, 1.5, 1.3125, NAN, 0.0, 1.0]
WANT_ACC_RED = [8.0, 12.0, 84.0, NAN, 0.0, 8.0]
WANT_Q_RED = [9.0, 20.0, 168.0, NAN, 0.0, 8.0]
WANT_LISTS = [[0, 1, 2, 3, 4, 5], [0, 1, 2, 3, 4, 5], [2, 3], [2, 3], [2, 3], [2, 3]]
FULL_MEAN_RED_5 = 2.0
