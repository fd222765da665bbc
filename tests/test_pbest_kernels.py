"""Stage-level fp64 tests of the v1 P(best) / EIG HIP kernels (GPU).

Every kernel of the oldest family, coda_amd/ops/hip/pbest.hip
(pbest_kernel, pbest_row_kernel, pbest_phase1 / pbest_phase2 and their
wide twins, eig_phase1 / eig_phase2, eig_hyp_kernel) is driven on its
own through the `ops._ext` bindings and compared with the fp64
reference of ITS contract (tests/pbest_ref.py). Inputs are built on the
CPU and moved to the device; no other kernel sits upstream of the one
under test. Phase-2 kernels get a CPU-built slog2: the fp64 reference
rounded to fp32, PLUS the reference partial of a second, virtual shard
of VIRTUAL_H models that the kernel never sees, so a kernel that
coupled against its local term instead of the global one would be off
by that shard.

What is compared. Normalised P(best): absolute error over the row, and
relative error on the big entries (reference >= 1 / (16 H); the CPU
module asserts that they hold >= 99 % of every row and that no
competitive row with H >= 3 has an entry above 0.9). Unnormalised
masses and totals: relative error (masses on the big entries); these
see what normalisation hides, such as the half weights at grid points
0 and 255. slog2: absolute error over every grid point AND over the
bulk of the row, the points where every model's reference cdf is
>= 2^-10 (pbest_ref.slog2_bulk, decided on the reference alone). The
whole-row figure is set by the deep lower tail (slog2 near -1e5 at
H = 1000), where the exclusive scan cancels and which pass B's +-115.4
clamp erases; the bulk figure is the sharp one. h_after: absolute.

Tolerances. None is calibrated on kernel output: each is the
reference's own fp32-vs-fp64 spread on the test's inputs (the fp32 twin
rounds every operation to fp32 in the kernel's order and is emulated in
fp64; tests/test_pbest_ref.py recomputes every figure on the CPU and
asserts it stays within HOST_BAND of the value recorded here) times
MARGIN = 16, the project's margin for fused kernels. A recorded spread
of 0 counts as one fp32 ulp (E_ULP).

Recorded spreads (fp32 twin vs fp64; tol = 16 x each):

  pbest_kernel (family, R, H)         abs      rel-big
  ----------------------------------------------------------------------
  ('wide', 2, 1)                    0.0e+00  0.0e+00
  ('wide', 4, 2)                    4.1e-08  4.1e-08
  ('wide', 5, 63)                   7.8e-08  1.4e-06
  ('wide', 7, 64)                   9.7e-08  5.7e-07
  ('wide', 2, 65)                   7.4e-09  1.9e-07
  ('wide', 4, 128)                  8.6e-08  4.8e-07
  ('wide', 5, 129)                  7.3e-08  8.6e-07
  ('wide', 7, 257)                  1.1e-07  2.3e-06
  ('moderate', 4, 1)                0.0e+00  0.0e+00
  ('moderate', 5, 2)                5.7e-08  1.2e-07
  ('moderate', 7, 63)               7.0e-08  3.1e-07
  ('moderate', 2, 64)               9.8e-08  3.4e-07
  ('moderate', 4, 65)               5.4e-08  4.5e-07
  ('moderate', 5, 128)              3.9e-08  1.0e-06
  ('moderate', 7, 129)              4.3e-08  6.8e-07
  ('moderate', 2, 257)              2.1e-08  4.5e-07
  ('singular_a', 5, 1)              6.0e-08  6.0e-08
  ('singular_a', 7, 2)              8.3e-08  2.8e-07
  ('singular_a', 2, 63)             3.3e-08  5.5e-07
  ('singular_a', 4, 64)             1.4e-08  4.9e-07
  ('singular_a', 5, 65)             3.7e-08  5.1e-07
  ('singular_a', 7, 128)            2.7e-08  1.1e-06
  ('singular_a', 2, 129)            1.3e-08  6.1e-07
  ('singular_a', 4, 257)            9.9e-10  2.1e-07
  ('singular_ab', 7, 1)             6.0e-08  6.0e-08
  ('singular_ab', 2, 2)             5.2e-08  1.1e-07
  ('singular_ab', 4, 63)            1.7e-07  3.1e-06
  ('singular_ab', 5, 64)            1.4e-07  3.3e-06
  ('singular_ab', 7, 65)            2.0e-07  3.2e-06
  ('singular_ab', 2, 128)           2.6e-08  5.8e-07
  ('singular_ab', 4, 129)           3.7e-08  9.4e-07
  ('singular_ab', 5, 257)           2.1e-08  6.8e-07
  ('competitive', 2, 1)             0.0e+00  0.0e+00
  ('competitive', 4, 2)             5.8e-07  1.6e-06
  ('competitive', 5, 63)            1.2e-07  1.2e-05
  ('competitive', 7, 64)            1.2e-07  8.3e-06
  ('competitive', 2, 65)            1.1e-07  5.8e-06
  ('competitive', 4, 128)           8.9e-08  2.1e-06
  ('competitive', 5, 129)           1.2e-07  3.2e-06
  ('competitive', 7, 257)           8.7e-08  2.7e-06
  ('moderate', 2, 2048)             6.6e-08  1.1e-06
  ('competitive', 2, 2048)          1.7e-07  3.3e-06

  pbest_row_kernel (family, H)        abs      rel-big
  ----------------------------------------------------------------------
  ('wide', 1)                       0.0e+00  0.0e+00
  ('wide', 2)                       3.2e-08  3.2e-08
  ('wide', 3)                       5.8e-09  5.8e-09
  ('wide', 4)                       2.4e-08  1.4e-07
  ('wide', 5)                       4.0e-08  1.9e-07
  ('wide', 7)                       3.2e-08  8.7e-08
  ('wide', 64)                      1.6e-08  1.7e-07
  ('wide', 257)                     5.5e-08  7.2e-07
  ('wide', 1000)                    5.0e-08  9.2e-07
  ('moderate', 1)                   0.0e+00  0.0e+00
  ('moderate', 2)                   3.8e-08  3.9e-08
  ('moderate', 3)                   7.5e-08  9.1e-08
  ('moderate', 4)                   2.7e-08  7.4e-08
  ('moderate', 5)                   7.3e-08  7.3e-08
  ('moderate', 7)                   3.8e-08  1.2e-07
  ('moderate', 64)                  1.6e-08  5.6e-07
  ('moderate', 257)                 2.5e-08  3.7e-07
  ('moderate', 1000)                1.1e-08  6.7e-07
  ('singular_a', 1)                 0.0e+00  0.0e+00
  ('singular_a', 2)                 1.1e-07  2.0e-07
  ('singular_a', 3)                 2.4e-08  5.7e-08
  ('singular_a', 4)                 2.0e-08  1.2e-07
  ('singular_a', 5)                 1.5e-08  8.3e-08
  ('singular_a', 7)                 1.4e-08  1.2e-07
  ('singular_a', 64)                1.3e-08  4.3e-07
  ('singular_a', 257)               6.1e-10  2.4e-07
  ('singular_a', 1000)              3.0e-10  3.9e-07
  ('singular_ab', 1)                1.2e-16  1.2e-16
  ('singular_ab', 2)                8.9e-08  1.4e-07
  ('singular_ab', 3)                9.2e-08  2.6e-07
  ('singular_ab', 4)                5.9e-08  1.3e-07
  ('singular_ab', 5)                2.6e-08  1.1e-07
  ('singular_ab', 7)                4.1e-08  3.1e-07
  ('singular_ab', 64)               1.6e-07  3.2e-06
  ('singular_ab', 257)              1.3e-08  5.5e-07
  ('singular_ab', 1000)             4.4e-09  6.4e-07
  ('competitive', 1)                0.0e+00  0.0e+00
  ('competitive', 2)                6.7e-08  7.0e-08
  ('competitive', 3)                8.0e-08  2.2e-06
  ('competitive', 4)                2.8e-07  1.3e-06
  ('competitive', 5)                9.5e-07  3.7e-06
  ('competitive', 7)                9.5e-08  2.8e-06
  ('competitive', 64)               1.5e-08  3.5e-06
  ('competitive', 257)              3.2e-08  1.6e-06
  ('competitive', 1000)             6.3e-08  3.0e-06

  phase1/2 (family, R, H)             slog2    bulk     mass     total
  ----------------------------------------------------------------------
  ('wide', 2, 1)                    4.3e-03  5.5e-07  4.9e-08  4.9e-08
  ('wide', 5, 3)                    4.7e-03  8.7e-07  1.1e-07  5.1e-08
  ('wide', 2, 65)                   1.3e-02  3.2e-06  1.5e-07  1.1e-08
  ('wide', 5, 257)                  4.0e-02  9.8e-06  3.2e-07  1.4e-07
  ('moderate', 5, 1)                1.4e-04  8.6e-07  5.2e-08  5.2e-08
  ('moderate', 2, 3)                3.9e-03  1.4e-06  8.3e-08  7.7e-08
  ('moderate', 5, 65)               3.1e-02  3.7e-06  1.4e-07  5.1e-08
  ('moderate', 2, 257)              4.2e-02  1.0e-05  1.7e-07  2.7e-08
  ('singular_a', 2, 1)              1.8e-06  3.5e-07  3.1e-08  3.1e-08
  ('singular_a', 5, 3)              1.3e-05  8.1e-07  3.0e-07  7.7e-08
  ('singular_a', 2, 65)             2.0e-05  5.5e-06  4.4e-07  2.9e-08
  ('singular_a', 5, 257)            8.0e-04  2.2e-05  1.9e-07  1.1e-07
  ('singular_ab', 5, 1)             1.8e-06  5.7e-07  3.3e-07  3.3e-07
  ('singular_ab', 2, 3)             1.3e-05  1.0e-06  3.7e-07  7.7e-08
  ('singular_ab', 5, 65)            2.0e-05  1.0e-05  3.0e-06  7.9e-07
  ('singular_ab', 2, 257)           8.0e-04  3.4e-05  8.4e-07  2.2e-07
  ('competitive', 2, 1)             4.1e-03  1.9e-05  8.0e-07  8.0e-07
  ('competitive', 5, 3)             8.8e-03  7.3e-06  1.9e-06  1.2e-06
  ('competitive', 2, 65)            7.9e-02  7.1e-04  6.0e-06  3.5e-07
  ('competitive', 5, 257)           2.1e-01  1.1e-03  2.0e-06  3.6e-07
  ('end0', 2, 1)                    1.8e-06  4.5e-07  1.1e-06  1.1e-06
  ('end255', 2, 1)                  2.1e-06  1.7e-06  7.2e-08  7.2e-08

  phase1/2_wide (family, R, H, hc)    slog2    bulk     mass     total
  ----------------------------------------------------------------------
  ('wide', 2, 130, 64)              5.7e-03  2.8e-06  1.5e-07  1.6e-07
  ('moderate', 5, 130, 64)          1.5e-02  4.5e-06  2.0e-07  3.4e-07
  ('singular_a', 2, 128, 64)        1.1e-04  7.2e-06  2.8e-07  9.6e-08
  ('singular_ab', 5, 128, 64)       1.1e-04  1.2e-05  8.3e-07  4.1e-07
  ('competitive', 2, 65, 64)        6.6e-02  3.6e-04  8.8e-06  1.2e-06
  ('wide', 5, 65, 64)               1.1e-02  2.8e-06  1.6e-07  1.3e-06
  ('moderate', 2, 70, 512)          1.4e-02  6.2e-06  1.9e-07  6.2e-08
  ('singular_a', 5, 70, 512)        1.8e-04  6.7e-06  4.4e-07  8.1e-08
  ('singular_ab', 2, 257, 100)      1.1e-04  1.5e-05  8.1e-07  2.2e-07
  ('competitive', 5, 257, 100)      1.1e-01  6.6e-04  1.9e-06  2.4e-07

  eig (H, C, B, w)                    slog2    bulk     mass     total    h_after
  ----------------------------------------------------------------------
  (1, 3, 7, 1.0)                    5.5e-05  6.0e-07  8.2e-08  8.2e-08  0.0e+00
  (1, 3, 7, 0.5)                    7.0e-05  6.9e-07  8.6e-08  8.6e-08  0.0e+00
  (5, 3, 7, 1.0)                    1.6e-03  2.6e-06  1.8e-07  1.6e-07  1.6e-07
  (5, 3, 7, 0.5)                    8.4e-04  1.9e-06  1.8e-07  1.1e-07  2.5e-07
  (65, 2, 5, 1.0)                   5.1e-03  9.1e-06  1.8e-07  1.2e-07  5.3e-07
  (65, 2, 5, 0.5)                   1.3e-03  8.2e-06  1.6e-07  8.0e-08  4.8e-07
  (129, 3, 3, 1.0)                  2.6e-02  1.9e-05  1.9e-07  1.1e-07  2.7e-07
  (129, 3, 3, 0.5)                  2.6e-02  1.6e-05  1.8e-07  5.0e-08  2.0e-07

  _pbest_wide_hip ('competitive', 3, 2100): abs 1.8e-07  rel-big 3.2e-06
  eig_chunk clamp case (5, 2, 3): h_after 9.3e-08
  eig_chunk dense contraction (65, 2, 5, 1.0): eig 4.4e-07

The faults these tolerances must catch (a dropped last model, a
trapezoid counted at lane 0, a full end weight, a window reading its
neighbour's models, a window coupled against its own partial, an
inverted v-select, update_weight on both sides or on none, a row using
its neighbour's class) each move the reference by at least 10
tolerances: tests/test_pbest_ref.py::TestToleranceFloors.
"""
from __future__ import annotations

import functools
from typing import NamedTuple

import pytest
import torch

from tests import pbest_ref as PB
from tests import table_ref as TR
from tests.test_pair_kernels import HOST_BAND  # noqa: F401 (CPU checks)

pytestmark = pytest.mark.gpu

SEED = 0
MARGIN = 16.0
E_ULP = 2.0 ** -23
VIRTUAL_H = 3                     # models of the virtual second shard
FAMS = PB.FAMILIES

# pbest_from_beta, generic kernel: every (family, H) and every (R, H)
_GR, _GH = (2, 4, 5, 7), (1, 2, 63, 64, 65, 128, 129, 257)
PBEST_CASES = [(f, _GR[(i + j) % 4], H) for i, f in enumerate(FAMS)
               for j, H in enumerate(_GH)]
# the fused dispatch's LDS ceiling: 4 rows x 2048 models x 20 B = 160 KiB
CEILING_CASES = [("moderate", 2, 2048), ("competitive", 2, 2048)]
# pbest_from_beta at R = 1 (pbest_row_kernel): empty windows (H < 4), a
# window start past H (H = 5: windows of 2 start at 0, 2, 4, 6), uneven
ROW_H = (1, 2, 3, 4, 5, 7, 64, 257, 1000)
ROW_CASES = [(f, H) for f in FAMS for H in ROW_H]
# pbest_phase1 / pbest_phase2: (family, R, H), and the two end-weight rows
_PH = (1, 3, 65, 257)
PHASE_CASES = [(f, (2, 5)[(i + j) % 2], H) for i, f in enumerate(FAMS)
               for j, H in enumerate(_PH)] \
    + [("end0", 2, 1), ("end255", 2, 1)]
# pbest_phase1_wide / pbest_phase2_wide: (family, R, H, hc) - an uneven
# tail window, an exact multiple, a one-model tail, hc > H, three windows
_WS = ((130, 64), (128, 64), (65, 64), (70, 512), (257, 100))
WIDE_CASES = [(FAMS[(2 * i + j) % len(FAMS)], R, H, hc)
              for i, (H, hc) in enumerate(_WS)
              for j, R in enumerate((2, 5))]
WIDE_E2E = ("competitive", 3, 2100)
# eig_phase1 / eig_phase2 / eig_chunk: (H, C, B, update_weight); B * C is
# never a multiple of the 4 rows per block
_ES = ((1, 3, 7), (5, 3, 7), (65, 2, 5), (129, 3, 3))
EIG_CASES = [(*s, w) for s in _ES for w in (1.0, 0.5)]

# ---------------------------------------------------------------------
# recorded fp32-twin spreads (rounded up to two digits)
# ---------------------------------------------------------------------
E_PBEST = {
    ('wide', 2, 1): (0.0, 0.0),
    ('wide', 4, 2): (4.1e-08, 4.1e-08),
    ('wide', 5, 63): (7.8e-08, 1.4e-06),
    ('wide', 7, 64): (9.7e-08, 5.7e-07),
    ('wide', 2, 65): (7.4e-09, 1.9e-07),
    ('wide', 4, 128): (8.6e-08, 4.8e-07),
    ('wide', 5, 129): (7.3e-08, 8.6e-07),
    ('wide', 7, 257): (1.1e-07, 2.3e-06),
    ('moderate', 4, 1): (0.0, 0.0),
    ('moderate', 5, 2): (5.7e-08, 1.2e-07),
    ('moderate', 7, 63): (7e-08, 3.1e-07),
    ('moderate', 2, 64): (9.8e-08, 3.4e-07),
    ('moderate', 4, 65): (5.4e-08, 4.5e-07),
    ('moderate', 5, 128): (3.9e-08, 1e-06),
    ('moderate', 7, 129): (4.3e-08, 6.8e-07),
    ('moderate', 2, 257): (2.1e-08, 4.5e-07),
    ('singular_a', 5, 1): (6e-08, 6e-08),
    ('singular_a', 7, 2): (8.3e-08, 2.8e-07),
    ('singular_a', 2, 63): (3.3e-08, 5.5e-07),
    ('singular_a', 4, 64): (1.4e-08, 4.9e-07),
    ('singular_a', 5, 65): (3.7e-08, 5.1e-07),
    ('singular_a', 7, 128): (2.7e-08, 1.1e-06),
    ('singular_a', 2, 129): (1.3e-08, 6.1e-07),
    ('singular_a', 4, 257): (9.9e-10, 2.1e-07),
    ('singular_ab', 7, 1): (6e-08, 6e-08),
    ('singular_ab', 2, 2): (5.2e-08, 1.1e-07),
    ('singular_ab', 4, 63): (1.7e-07, 3.1e-06),
    ('singular_ab', 5, 64): (1.4e-07, 3.3e-06),
    ('singular_ab', 7, 65): (2e-07, 3.2e-06),
    ('singular_ab', 2, 128): (2.6e-08, 5.8e-07),
    ('singular_ab', 4, 129): (3.7e-08, 9.4e-07),
    ('singular_ab', 5, 257): (2.1e-08, 6.8e-07),
    ('competitive', 2, 1): (0.0, 0.0),
    ('competitive', 4, 2): (5.8e-07, 1.6e-06),
    ('competitive', 5, 63): (1.2e-07, 1.2e-05),
    ('competitive', 7, 64): (1.2e-07, 8.3e-06),
    ('competitive', 2, 65): (1.1e-07, 5.8e-06),
    ('competitive', 4, 128): (8.9e-08, 2.1e-06),
    ('competitive', 5, 129): (1.2e-07, 3.2e-06),
    ('competitive', 7, 257): (8.7e-08, 2.7e-06),
    ('moderate', 2, 2048): (6.6e-08, 1.1e-06),
    ('competitive', 2, 2048): (1.7e-07, 3.3e-06),
}
E_ROW = {
    ('wide', 1): (0.0, 0.0),
    ('wide', 2): (3.2e-08, 3.2e-08),
    ('wide', 3): (5.8e-09, 5.8e-09),
    ('wide', 4): (2.4e-08, 1.4e-07),
    ('wide', 5): (4e-08, 1.9e-07),
    ('wide', 7): (3.2e-08, 8.7e-08),
    ('wide', 64): (1.6e-08, 1.7e-07),
    ('wide', 257): (5.5e-08, 7.2e-07),
    ('wide', 1000): (5e-08, 9.2e-07),
    ('moderate', 1): (0.0, 0.0),
    ('moderate', 2): (3.8e-08, 3.9e-08),
    ('moderate', 3): (7.5e-08, 9.1e-08),
    ('moderate', 4): (2.7e-08, 7.4e-08),
    ('moderate', 5): (7.3e-08, 7.3e-08),
    ('moderate', 7): (3.8e-08, 1.2e-07),
    ('moderate', 64): (1.6e-08, 5.6e-07),
    ('moderate', 257): (2.5e-08, 3.7e-07),
    ('moderate', 1000): (1.1e-08, 6.7e-07),
    ('singular_a', 1): (0.0, 0.0),
    ('singular_a', 2): (1.1e-07, 2e-07),
    ('singular_a', 3): (2.4e-08, 5.7e-08),
    ('singular_a', 4): (2e-08, 1.2e-07),
    ('singular_a', 5): (1.5e-08, 8.3e-08),
    ('singular_a', 7): (1.4e-08, 1.2e-07),
    ('singular_a', 64): (1.3e-08, 4.3e-07),
    ('singular_a', 257): (6.1e-10, 2.4e-07),
    ('singular_a', 1000): (3e-10, 3.9e-07),
    ('singular_ab', 1): (1.2e-16, 1.2e-16),
    ('singular_ab', 2): (8.9e-08, 1.4e-07),
    ('singular_ab', 3): (9.2e-08, 2.6e-07),
    ('singular_ab', 4): (5.9e-08, 1.3e-07),
    ('singular_ab', 5): (2.6e-08, 1.1e-07),
    ('singular_ab', 7): (4.1e-08, 3.1e-07),
    ('singular_ab', 64): (1.6e-07, 3.2e-06),
    ('singular_ab', 257): (1.3e-08, 5.5e-07),
    ('singular_ab', 1000): (4.4e-09, 6.4e-07),
    ('competitive', 1): (0.0, 0.0),
    ('competitive', 2): (6.7e-08, 7e-08),
    ('competitive', 3): (8e-08, 2.2e-06),
    ('competitive', 4): (2.8e-07, 1.3e-06),
    ('competitive', 5): (9.5e-07, 3.7e-06),
    ('competitive', 7): (9.5e-08, 2.8e-06),
    ('competitive', 64): (1.5e-08, 3.5e-06),
    ('competitive', 257): (3.2e-08, 1.6e-06),
    ('competitive', 1000): (6.3e-08, 3e-06),
}
E_PHASE = {
    ('wide', 2, 1): (0.0043, 5.5e-07, 4.9e-08, 4.9e-08),
    ('wide', 5, 3): (0.0047, 8.7e-07, 1.1e-07, 5.1e-08),
    ('wide', 2, 65): (0.013, 3.2e-06, 1.5e-07, 1.1e-08),
    ('wide', 5, 257): (0.04, 9.8e-06, 3.2e-07, 1.4e-07),
    ('moderate', 5, 1): (0.00014, 8.6e-07, 5.2e-08, 5.2e-08),
    ('moderate', 2, 3): (0.0039, 1.4e-06, 8.3e-08, 7.7e-08),
    ('moderate', 5, 65): (0.031, 3.7e-06, 1.4e-07, 5.1e-08),
    ('moderate', 2, 257): (0.042, 1e-05, 1.7e-07, 2.7e-08),
    ('singular_a', 2, 1): (1.8e-06, 3.5e-07, 3.1e-08, 3.1e-08),
    ('singular_a', 5, 3): (1.3e-05, 8.1e-07, 3e-07, 7.7e-08),
    ('singular_a', 2, 65): (2e-05, 5.5e-06, 4.4e-07, 2.9e-08),
    ('singular_a', 5, 257): (0.0008, 2.2e-05, 1.9e-07, 1.1e-07),
    ('singular_ab', 5, 1): (1.8e-06, 5.7e-07, 3.3e-07, 3.3e-07),
    ('singular_ab', 2, 3): (1.3e-05, 1e-06, 3.7e-07, 7.7e-08),
    ('singular_ab', 5, 65): (2e-05, 1e-05, 3e-06, 7.9e-07),
    ('singular_ab', 2, 257): (0.0008, 3.4e-05, 8.4e-07, 2.2e-07),
    ('competitive', 2, 1): (0.0041, 1.9e-05, 8e-07, 8e-07),
    ('competitive', 5, 3): (0.0088, 7.3e-06, 1.9e-06, 1.2e-06),
    ('competitive', 2, 65): (0.079, 0.00071, 6e-06, 3.5e-07),
    ('competitive', 5, 257): (0.21, 0.0011, 2e-06, 3.6e-07),
    ('end0', 2, 1): (1.8e-06, 4.5e-07, 1.1e-06, 1.1e-06),
    ('end255', 2, 1): (2.1e-06, 1.7e-06, 7.2e-08, 7.2e-08),
}
E_WIDE = {
    ('wide', 2, 130, 64): (0.0057, 2.8e-06, 1.5e-07, 1.6e-07),
    ('moderate', 5, 130, 64): (0.015, 4.5e-06, 2e-07, 3.4e-07),
    ('singular_a', 2, 128, 64): (0.00011, 7.2e-06, 2.8e-07, 9.6e-08),
    ('singular_ab', 5, 128, 64): (0.00011, 1.2e-05, 8.3e-07, 4.1e-07),
    ('competitive', 2, 65, 64): (0.066, 0.00036, 8.8e-06, 1.2e-06),
    ('wide', 5, 65, 64): (0.011, 2.8e-06, 1.6e-07, 1.3e-06),
    ('moderate', 2, 70, 512): (0.014, 6.2e-06, 1.9e-07, 6.2e-08),
    ('singular_a', 5, 70, 512): (0.00018, 6.7e-06, 4.4e-07, 8.1e-08),
    ('singular_ab', 2, 257, 100): (0.00011, 1.5e-05, 8.1e-07, 2.2e-07),
    ('competitive', 5, 257, 100): (0.11, 0.00066, 1.9e-06, 2.4e-07),
}
E_EIG = {
    (1, 3, 7, 1.0): (5.5e-05, 6e-07, 8.2e-08, 8.2e-08, 0.0),
    (1, 3, 7, 0.5): (7e-05, 6.9e-07, 8.6e-08, 8.6e-08, 0.0),
    (5, 3, 7, 1.0): (0.0016, 2.6e-06, 1.8e-07, 1.6e-07, 1.6e-07),
    (5, 3, 7, 0.5): (0.00084, 1.9e-06, 1.8e-07, 1.1e-07, 2.5e-07),
    (65, 2, 5, 1.0): (0.0051, 9.1e-06, 1.8e-07, 1.2e-07, 5.3e-07),
    (65, 2, 5, 0.5): (0.0013, 8.2e-06, 1.6e-07, 8e-08, 4.8e-07),
    (129, 3, 3, 1.0): (0.026, 1.9e-05, 1.9e-07, 1.1e-07, 2.7e-07),
    (129, 3, 3, 0.5): (0.026, 1.6e-05, 1.8e-07, 5e-08, 2e-07),
}
E_WIDE_E2E = (1.8e-07, 3.2e-06)
E_EIG_CLAMP = 9.3e-08
E_EIG_DENSE = 4.4e-07


def tol(rec: float) -> float:
    return MARGIN * (rec if rec > 0 else E_ULP)


# ---------------------------------------------------------------------
# CPU-side inputs, references and measurements (shared with
# test_pbest_ref.py)
# ---------------------------------------------------------------------

def betas(fam, R, H):
    return PB.make_betas(fam, R, H, seed=SEED)


@functools.lru_cache(maxsize=None)
def pbest_ref(fam, R, H):
    return PB.ref_pbest(*betas(fam, R, H))


def measure_e_pbest(fam, R, H):
    twin = PB.ref_pbest(*betas(fam, R, H), f32=True)
    assert bool(torch.isfinite(twin).all())
    return PB.pbest_errs(twin, pbest_ref(fam, R, H))


@functools.lru_cache(maxsize=None)
def row_ref(fam, H):
    return PB.ref_pbest_row(*betas(fam, 1, H))


def measure_e_row(fam, H):
    twin = PB.ref_pbest_row(*betas(fam, 1, H), f32=True)
    assert bool(torch.isfinite(twin).all())
    return PB.pbest_errs(twin, row_ref(fam, H))


class PhaseRef(NamedTuple):
    slog2: torch.Tensor         # (R, P) fp64 local partial
    bulk: torch.Tensor          # (R, P) bool
    slog2_in: torch.Tensor      # (R, P) fp32 global term (with virtual)
    masses: torch.Tensor        # (R, H) fp64 for slog2_in
    total: torch.Tensor         # (R,)


def _global_slog2(local, av, bv):
    return (local + PB.ref_slog2(av, bv)).float()


def phase_betas(fam, R, H):
    """(a, b, av, bv): the kernel's H models and the VIRTUAL_H models of
    the virtual second shard, drawn as ONE row of H + VIRTUAL_H models
    (a competitive row's shards share its common mean). The end-weight
    rows have no second shard: any other model's cdf is 0 at point 0
    and would clamp that point's integrand away, half weight and all."""
    if fam in PB.END_RANGES:
        a, b = betas(fam, R, H)
        return a, b, a[:, :0], b[:, :0]
    a, b = betas(fam, R, H + VIRTUAL_H)
    return (a[:, :H].contiguous(), b[:, :H].contiguous(),
            a[:, H:].contiguous(), b[:, H:].contiguous())


@functools.lru_cache(maxsize=None)
def phase_ref(fam, R, H) -> PhaseRef:
    a, b, av, bv = phase_betas(fam, R, H)
    s = PB.ref_slog2(a, b)
    g = _global_slog2(s, av, bv)
    m, t = PB.ref_masses(a, b, g)
    return PhaseRef(s, PB.slog2_bulk(a, b), g, m, t)


def measure_e_phase(fam, R, H):
    a, b = phase_betas(fam, R, H)[:2]
    ref = phase_ref(fam, R, H)
    s32 = PB.ref_slog2(a, b, f32=True)
    m32, t32 = PB.ref_masses(a, b, ref.slog2_in, f32=True)
    assert bool(torch.isfinite(m32).all())
    return (*PB.slog2_errs(s32, ref.slog2, ref.bulk),
            *PB.mass_errs(m32, t32, ref.masses, ref.total))


class WideRef(NamedTuple):
    parts: torch.Tensor         # (KH, R, P) fp64 per-window partials
    bulk: torch.Tensor          # (KH, R, P) bool
    slog2_in: torch.Tensor      # (R, P) fp32 sum of the partials
    masses: torch.Tensor        # (R, H)
    tot_part: torch.Tensor      # (KH, R)


@functools.lru_cache(maxsize=None)
def wide_ref(fam, R, H, hc) -> WideRef:
    a, b = betas(fam, R, H)
    parts = PB.ref_slog2_windows(a, b, hc)
    bulk = torch.stack([PB.slog2_bulk(a[:, h0:h1], b[:, h0:h1])
                        for h0, h1 in PB.windows(H, hc)])
    g = parts.sum(0).float()
    m, t = PB.ref_masses_windows(a, b, g, hc)
    return WideRef(parts, bulk, g, m, t)


def measure_e_wide(fam, R, H, hc):
    a, b = betas(fam, R, H)
    ref = wide_ref(fam, R, H, hc)
    p32 = PB.ref_slog2_windows(a, b, hc, f32=True)
    m32, t32 = PB.ref_masses_windows(a, b, ref.slog2_in, hc, f32=True)
    assert bool(torch.isfinite(m32).all())
    return (*PB.slog2_errs(p32, ref.parts, ref.bulk),
            *PB.mass_errs(m32, t32, ref.masses, ref.tot_part))


@functools.lru_cache(maxsize=None)
def wide_e2e_ref():
    return PB.ref_pbest(*betas(*WIDE_E2E))


def measure_e_wide_e2e():
    twin = PB.ref_pbest_windows(*betas(*WIDE_E2E), 512, f32=True)
    assert bool(torch.isfinite(twin).all())
    return PB.pbest_errs(twin, wide_e2e_ref())


def eig_inputs(case):
    if case == "clamp":
        return PB.make_hyp_clamp_inputs(), 1.0
    H, C, B, w = case
    return PB.make_hyp_inputs(H, C, B, seed=SEED), w


class EigRef(NamedTuple):
    a: torch.Tensor             # (B*C, H) fp32 staged rows
    b: torch.Tensor
    phase: PhaseRef
    h_after: torch.Tensor       # (B, C) fp64


@functools.lru_cache(maxsize=None)
def eig_ref(case) -> EigRef:
    i, w = eig_inputs(case)
    H, C = i.alpha_cc.shape
    a, b = PB.ref_hyp_betas(i.alpha_cc, i.beta_cc, i.cls, w)
    # virtual shard: VIRTUAL_H more models with their own classes
    v = PB.make_hyp_inputs(VIRTUAL_H, C, i.cls.shape[0], seed=SEED + 77)
    av, bv = PB.ref_hyp_betas(v.alpha_cc, v.beta_cc, v.cls, w)
    s = PB.ref_slog2(a, b)
    g = _global_slog2(s, av, bv)
    m, t = PB.ref_masses(a, b, g)
    h = PB.ref_h_after(i.alpha_cc, i.beta_cc, i.cls, w, i.pi_hat,
                       i.pbest_before, i.mixture0)
    return EigRef(a, b, PhaseRef(s, PB.slog2_bulk(a, b), g, m, t), h)


def measure_e_eig(case):
    i, w = eig_inputs(case)
    ref = eig_ref(case)
    s32 = PB.ref_slog2(ref.a, ref.b, f32=True)
    m32, t32 = PB.ref_masses(ref.a, ref.b, ref.phase.slog2_in, f32=True)
    h32 = PB.ref_h_after(i.alpha_cc, i.beta_cc, i.cls, w, i.pi_hat,
                         i.pbest_before, i.mixture0, f32=True)
    assert bool(torch.isfinite(m32).all() and torch.isfinite(h32).all())
    return (*PB.slog2_errs(s32, ref.phase.slog2, ref.phase.bulk),
            *PB.mass_errs(m32, t32, ref.phase.masses, ref.phase.total),
            float((h32 - ref.h_after).abs().max()))


DENSE_CASE = (65, 2, 5, 1.0)


def dense_h_before() -> float:
    return 3.25


def dense_ref():
    i, _ = eig_inputs(DENSE_CASE)
    return dense_h_before() - (i.pi_hat_xi.double()
                               * eig_ref(DENSE_CASE).h_after).sum(-1)


def measure_e_dense() -> float:
    """The binding's contraction h_before - sum_c pi_hat_xi h_after in
    fp32 on the fp32 twin's h_after."""
    i, w = eig_inputs(DENSE_CASE)
    h32 = PB.ref_h_after(i.alpha_cc, i.beta_cc, i.cls, w, i.pi_hat,
                         i.pbest_before, i.mixture0, f32=True)
    prod = PB._r32(i.pi_hat_xi.double() * h32)
    twin = PB._r32(dense_h_before() - PB.PR._sum32(prod, 4))
    return float((twin - dense_ref()).abs().max())


# ---------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------

@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ext():
    import coda_amd.ops as ops
    assert ops.hip_available(), \
        "HIP extension must be built on GPU boxes (python build_hip.py)"
    return ops._ext


def _report(label, errs, recs, names):
    print(f"{label}: " + " ".join(
        f"{n} {e:.3g} (tol {tol(r):.3g}, twin {r:.3g})"
        for n, e, r in zip(names, errs, recs)))
    for n, e, r in zip(names, errs, recs):
        assert e <= tol(r), (label, n, e, tol(r))


_PB_NAMES = ("abs", "rel-big")
_PHASE1_NAMES = ("slog2", "bulk slog2")
_PHASE2_NAMES = ("mass rel", "total rel")


class TestPbestFromBeta:
    @pytest.mark.parametrize("fam,R,H", PBEST_CASES + CEILING_CASES)
    def test_generic_vs_fp64(self, ext, dev, fam, R, H):
        """pbest_kernel (R >= 2): rows that do not fill the last block,
        H across the 64-lane store / normaliser strides, and the
        160 KiB LDS ceiling at H = 2048."""
        a, b = betas(fam, R, H)
        ref = pbest_ref(fam, R, H)
        got = ext.pbest_from_beta(a.to(dev), b.to(dev), 256).cpu()
        assert got.shape == (R, H) and bool(torch.isfinite(got).all())
        _report(f"pbest_from_beta {(fam, R, H)}", PB.pbest_errs(got, ref),
                E_PBEST[(fam, R, H)], _PB_NAMES)

    @pytest.mark.parametrize("fam,H", ROW_CASES)
    def test_row_kernel_vs_fp64(self, ext, dev, fam, H):
        """pbest_row_kernel (R = 1): four windows of ceil(H / 4)."""
        a, b = betas(fam, 1, H)
        got = ext.pbest_from_beta(a.to(dev), b.to(dev), 256).cpu()
        assert got.shape == (1, H) and bool(torch.isfinite(got).all())
        _report(f"pbest_row {(fam, H)}",
                PB.pbest_errs(got, row_ref(fam, H)), E_ROW[(fam, H)],
                _PB_NAMES)


class TestPhaseKernels:
    @pytest.mark.parametrize("fam,R,H", PHASE_CASES)
    def test_phase1_vs_fp64(self, ext, dev, fam, R, H):
        a, b = phase_betas(fam, R, H)[:2]
        ref = phase_ref(fam, R, H)
        got = ext.pbest_phase1(a.to(dev), b.to(dev)).cpu()
        assert got.shape == (R, TR.P) and bool(torch.isfinite(got).all())
        _report(f"pbest_phase1 {(fam, R, H)}",
                PB.slog2_errs(got, ref.slog2, ref.bulk),
                E_PHASE[(fam, R, H)][:2], _PHASE1_NAMES)

    @pytest.mark.parametrize("fam,R,H", PHASE_CASES)
    def test_phase2_vs_fp64(self, ext, dev, fam, R, H):
        """Unnormalised masses and totals for a CPU-built global slog2
        (local reference partial + the virtual shard's)."""
        a, b = phase_betas(fam, R, H)[:2]
        ref = phase_ref(fam, R, H)
        pb, tot = ext.pbest_phase2(a.to(dev), b.to(dev),
                                   ref.slog2_in.to(dev))
        pb, tot = pb.cpu(), tot.cpu()
        assert pb.shape == (R, H) and tot.shape == (R,)
        assert bool(torch.isfinite(pb).all())
        _report(f"pbest_phase2 {(fam, R, H)}",
                PB.mass_errs(pb, tot, ref.masses, ref.total),
                E_PHASE[(fam, R, H)][2:], _PHASE2_NAMES)


class TestWideKernels:
    @pytest.mark.parametrize("fam,R,H,hc", WIDE_CASES)
    def test_phase1_wide_vs_fp64(self, ext, dev, fam, R, H, hc):
        a, b = betas(fam, R, H)
        ref = wide_ref(fam, R, H, hc)
        got = ext.pbest_phase1_wide(a.to(dev), b.to(dev), hc).cpu()
        assert got.shape == ref.parts.shape
        assert bool(torch.isfinite(got).all())
        _report(f"pbest_phase1_wide {(fam, R, H, hc)}",
                PB.slog2_errs(got, ref.parts, ref.bulk),
                E_WIDE[(fam, R, H, hc)][:2], _PHASE1_NAMES)

    @pytest.mark.parametrize("fam,R,H,hc", WIDE_CASES)
    def test_phase2_wide_vs_fp64(self, ext, dev, fam, R, H, hc):
        a, b = betas(fam, R, H)
        ref = wide_ref(fam, R, H, hc)
        pb, tot = ext.pbest_phase2_wide(a.to(dev), b.to(dev),
                                        ref.slog2_in.to(dev), hc)
        pb, tot = pb.cpu(), tot.cpu()
        assert pb.shape == (R, H) and tot.shape == ref.tot_part.shape
        assert bool(torch.isfinite(pb).all())
        _report(f"pbest_phase2_wide {(fam, R, H, hc)}",
                PB.mass_errs(pb, tot, ref.masses, ref.tot_part),
                E_WIDE[(fam, R, H, hc)][2:], _PHASE2_NAMES)

    def test_wide_end_to_end(self, dev):
        """ops._pbest_wide_hip at H = 2100, five windows of 512."""
        import coda_amd.ops as ops
        a, b = betas(*WIDE_E2E)
        got = ops._pbest_wide_hip(a.to(dev), b.to(dev), 512).cpu()
        assert bool(torch.isfinite(got).all())
        _report(f"_pbest_wide_hip {WIDE_E2E}",
                PB.pbest_errs(got, wide_e2e_ref()), E_WIDE_E2E, _PB_NAMES)


def _hyp_dev(i, dev):
    return (i.alpha_cc.to(dev), i.beta_cc.to(dev),
            i.cls.to(torch.int32).to(dev))


def _h_after_via_eig_chunk(ext, dev, i, w):
    """(B, C) h_after alone: each candidate replicated C times with
    one-hot pi_hat_xi rows and h_before = 0 makes the binding return
    -h_after[b, c] exactly (1 * x plus zeros)."""
    H, C = i.alpha_cc.shape
    B = i.cls.shape[0]
    cls = i.cls.repeat_interleave(C, 0).to(torch.int32).to(dev)
    onehot = torch.eye(C).repeat(B, 1).to(dev)
    out = ext.eig_chunk(i.alpha_cc.to(dev), i.beta_cc.to(dev), cls,
                        i.pbest_before.to(dev), i.pi_hat.to(dev), onehot,
                        i.mixture0.to(dev), 0.0, float(w), 256)
    return -out.cpu().reshape(B, C)


class TestEigKernels:
    @pytest.mark.parametrize("case", EIG_CASES)
    def test_eig_phase1_vs_fp64(self, ext, dev, case):
        i, w = eig_inputs(case)
        ref = eig_ref(case).phase
        got = ext.eig_phase1(*_hyp_dev(i, dev), w).cpu()
        assert got.shape == ref.slog2.shape
        assert bool(torch.isfinite(got).all())
        _report(f"eig_phase1 {case}",
                PB.slog2_errs(got, ref.slog2, ref.bulk),
                E_EIG[case][:2], _PHASE1_NAMES)

    @pytest.mark.parametrize("case", EIG_CASES)
    def test_eig_phase2_vs_fp64(self, ext, dev, case):
        i, w = eig_inputs(case)
        ref = eig_ref(case).phase
        pb, tot = ext.eig_phase2(*_hyp_dev(i, dev), ref.slog2_in.to(dev), w)
        pb, tot = pb.cpu(), tot.cpu()
        assert pb.shape == ref.masses.shape and tot.shape == ref.total.shape
        assert bool(torch.isfinite(pb).all())
        _report(f"eig_phase2 {case}",
                PB.mass_errs(pb, tot, ref.masses, ref.total),
                E_EIG[case][2:4], _PHASE2_NAMES)

    @pytest.mark.parametrize("case", EIG_CASES + ["clamp"])
    def test_eig_chunk_h_after_vs_fp64(self, ext, dev, case):
        """eig_hyp_kernel's h_after[b, c] on its own."""
        i, w = eig_inputs(case)
        got = _h_after_via_eig_chunk(ext, dev, i, w)
        assert bool(torch.isfinite(got).all())
        err = float((got.double() - eig_ref(case).h_after).abs().max())
        rec = E_EIG_CLAMP if case == "clamp" else E_EIG[case][4]
        _report(f"eig_chunk {case}", (err,), (rec,), ("h_after",))

    def test_eig_chunk_dense_contraction(self, ext, dev):
        """The binding's final h_before - sum_c pi_hat_xi h_after with
        dense pi_hat_xi rows."""
        i, w = eig_inputs(DENSE_CASE)
        got = ext.eig_chunk(*_hyp_dev(i, dev), i.pbest_before.to(dev),
                            i.pi_hat.to(dev), i.pi_hat_xi.to(dev),
                            i.mixture0.to(dev), dense_h_before(), w,
                            256).cpu()
        err = float((got.double() - dense_ref()).abs().max())
        _report("eig_chunk dense", (err,), (E_EIG_DENSE,), ("eig",))


class TestHostRejections:
    """Argument checks that fail in a TORCH_CHECK before any launch."""

    @staticmethod
    def _rows(dev, R=3, H=5):
        return (torch.full((R, H), 2.0, device=dev),
                torch.full((R, H), 3.0, device=dev),
                torch.zeros(R, 256, device=dev))

    def test_phase_bindings_check_alpha_beta(self, ext, dev):
        a, b, s = self._rows(dev)
        for bad_b in (b[:, :4].contiguous(), b[:2].contiguous(),
                      b.reshape(-1)):
            with pytest.raises(RuntimeError, match=r"\(R, H\)"):
                ext.pbest_phase1(a, bad_b)
            with pytest.raises(RuntimeError, match=r"\(R, H\)"):
                ext.pbest_phase2(a, bad_b, s)
            with pytest.raises(RuntimeError, match=r"\(R, H\)"):
                ext.pbest_phase1_wide(a, bad_b, 4)
            with pytest.raises(RuntimeError, match=r"\(R, H\)"):
                ext.pbest_phase2_wide(a, bad_b, s, 4)
        with pytest.raises(RuntimeError, match=r"\(R, H\)"):
            ext.pbest_phase1(a.reshape(-1), b.reshape(-1))

    @pytest.mark.parametrize("bad", [
        lambda s: s[:2].contiguous(), lambda s: s[:, :128].contiguous(),
        lambda s: s.reshape(-1), lambda s: s.t().contiguous().t(),
        lambda s: s.cpu(), lambda s: s.double()])
    def test_slog2_checked(self, ext, dev, bad):
        a, b, s = self._rows(dev)
        with pytest.raises(RuntimeError, match="slog2"):
            ext.pbest_phase2(a, b, bad(s))
        with pytest.raises(RuntimeError, match="slog2"):
            ext.pbest_phase2_wide(a, b, bad(s), 4)
        H, C, B = 5, 3, 1
        acc = torch.full((H, C), 2.0, device=dev)
        cls = torch.zeros(B, H, dtype=torch.int32, device=dev)
        with pytest.raises(RuntimeError, match="slog2"):
            ext.eig_phase2(acc, acc, cls, bad(s), 1.0)

    @pytest.mark.parametrize("bad,msg", [
        (lambda c: c.long(), "int32"),
        (lambda c: c.t().contiguous().t(), "contiguous"),
        (lambda c: c[:, :4].contiguous(), r"\(B, H\)"),
        (lambda c: c.reshape(-1), r"\(B, H\)"),
        (lambda c: c.cpu(), "ROCm device"),
    ])
    def test_chunk_classes_checked(self, ext, dev, bad, msg):
        H, C, B = 5, 3, 2
        acc = torch.full((H, C), 2.0, device=dev)
        cls = torch.zeros(B, H, dtype=torch.int32, device=dev)
        s = torch.zeros(B * C, 256, device=dev)
        pbb = torch.full((C, H), 0.2, device=dev)
        pi = torch.full((C,), 1 / 3, device=dev)
        xi = torch.full((B, C), 1 / 3, device=dev)
        mix = torch.full((H,), 0.2, device=dev)
        with pytest.raises(RuntimeError, match=msg):
            ext.eig_phase1(acc, acc, bad(cls), 1.0)
        with pytest.raises(RuntimeError, match=msg):
            ext.eig_phase2(acc, acc, bad(cls), s, 1.0)
        with pytest.raises(RuntimeError, match=msg):
            ext.eig_chunk(acc, acc, bad(cls), pbb, pi, xi, mix, 0.0, 1.0,
                          256)
        with pytest.raises(RuntimeError, match=r"\(H, C\)"):
            ext.eig_phase1(acc, acc[:, :2].contiguous(), cls, 1.0)

    def test_window_size_checked(self, ext, dev):
        a, b, s = self._rows(dev)
        with pytest.raises(RuntimeError, match="hc must be"):
            ext.pbest_phase1_wide(a, b, 0)
        with pytest.raises(RuntimeError, match="hc must be"):
            ext.pbest_phase2_wide(a, b, s, 0)

    @pytest.mark.parametrize("name,bad,msg", [
        ("pbb", lambda t: t[:, :4].contiguous(), r"pbest_before must be"),
        ("pbb", lambda t: t[:2].contiguous(), r"pbest_before must be"),
        ("pi", lambda t: t[:2].contiguous(), r"pi_hat must be"),
        ("mix", lambda t: t[:4].contiguous(), r"mixture0 must be"),
        ("xi", lambda t: t[:1].contiguous(), r"pi_hat_xi must be"),
        ("xi", lambda t: t[:, :2].contiguous(), r"pi_hat_xi must be"),
    ])
    def test_eig_chunk_operands_checked(self, ext, dev, name, bad, msg):
        """Everything eig_hyp_kernel and the final contraction index."""
        H, C, B = 5, 3, 2
        acc = torch.full((H, C), 2.0, device=dev)
        t = {"cls": torch.zeros(B, H, dtype=torch.int32, device=dev),
             "pbb": torch.full((C, H), 0.2, device=dev),
             "pi": torch.full((C,), 1 / 3, device=dev),
             "xi": torch.full((B, C), 1 / 3, device=dev),
             "mix": torch.full((H,), 0.2, device=dev)}
        t[name] = bad(t[name])
        with pytest.raises(RuntimeError, match=msg):
            ext.eig_chunk(acc, acc, t["cls"], t["pbb"], t["pi"], t["xi"],
                          t["mix"], 0.0, 1.0, 256)

    def test_phase2_lds_ceiling_checked(self, ext, dev):
        """One model past the 160 KiB ceiling is refused by phase 2 as
        by phase 1, before any launch."""
        H = 2049
        a = torch.full((1, H), 2.0, device=dev)
        s = torch.zeros(1, 256, device=dev)
        with pytest.raises(RuntimeError, match="too large for LDS"):
            ext.pbest_phase1(a, a)
        with pytest.raises(RuntimeError, match="too large for LDS"):
            ext.pbest_phase2(a, a, s)
        acc = torch.full((H, 1), 2.0, device=dev)
        cls = torch.zeros(1, H, dtype=torch.int32, device=dev)
        with pytest.raises(RuntimeError, match="too large for LDS"):
            ext.eig_phase1(acc, acc, cls, 1.0)
        with pytest.raises(RuntimeError, match="too large for LDS"):
            ext.eig_phase2(acc, acc, cls, s, 1.0)
