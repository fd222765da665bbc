"""Stage-level fp64 tests of the table engine's HIP kernels (GPU).

Every v2 kernel of coda_amd/ops/hip/table.hip (es_build with its
block-per-row companion, es_build_gathered, eig_assemble_k, eig_totals,
eig_entropy, beta_row_tables, table_commit_row / table_commit_cols) is
driven on its own through the `ops._ext` bindings and compared with the
fp64 reference of ITS contract (tests/table_ref.py). Inputs are built on
the CPU and moved to the device; no other kernel sits upstream of the
one under test.

Tolerances. None is calibrated on kernel output: each is the
reference's own fp32-vs-fp64 spread on the test's inputs (the fp32 twin
rounds every operation to fp32 in a fixed order and is emulated in
fp64; tests/test_table_ref.py recomputes every figure on the CPU and
asserts it stays within HOST_BAND of the value recorded here) times
MARGIN = 16, the project's margin for fused kernels (reduction order,
and the hardware's 1-ulp log2/exp2 against libm; see
tests/test_pair_kernels.py).

  es_build on synthetic tables (table_ref.make_es_inputs: every ES value a
  normal fp32 number, one model more or less moves a row by >= 1.08e-2, and
  dall skewed by 2^-4 off the sum of delta so that the branch a row took
  shows in its value: 4.4e-2). Branch census = rows per (direct-short,
  complement-short, direct-long, complement-long); long rows belong to the
  block-per-row kernel.

  es_build (H, C)   rel spread  16*spread  branch census
  --------------------------------------------------------------------------
  (70, 3)           2.0e-06     3.2e-05    (24, 3, 0, 0)
  (71, 3)           1.9e-06     3.0e-05    (5, 1, 0, 0)
  (1024, 2)         1.5e-05     2.4e-04    (5, 3, 0, 0)
  (1026, 2)         1.2e-05     1.9e-04    (4, 4, 2, 0)
  (1100, 3)         1.2e-05     1.9e-04    (30, 4, 11, 3)

  es_build_gathered Hg  rel spread  16*spread
  -------------------------------------------
  1                     7.5e-07     1.2e-05
  5                     7.7e-07     1.2e-05
  70                    1.7e-06     2.7e-05
  257                   4.3e-06     6.9e-05

  assemble (H, C, B)  fp32 M: spread  tol      bf16 M: spread  tol
  ----------------------------------------------------------------
  (1, 3, 7)           0.0e+00         1.9e-06  0.0e+00         1.9e-06
  (2, 3, 7)           6.5e-08         1.9e-06  9.4e-08         1.9e-06
  (63, 3, 7)          3.0e-07         4.8e-06  4.5e-07         7.2e-06
  (64, 3, 7)          5.2e-07         8.3e-06  4.6e-07         7.4e-06
  (65, 3, 7)          5.1e-07         8.2e-06  4.5e-07         7.2e-06
  (128, 3, 7)         5.2e-07         8.3e-06  6.4e-07         1.0e-05
  (129, 3, 7)         5.0e-07         8.0e-06  6.7e-07         1.1e-05
  (130, 3, 7)         4.9e-07         7.8e-06  5.3e-07         8.5e-06
  (192, 3, 7)         6.4e-07         1.0e-05  5.1e-07         8.2e-06
  (193, 3, 7)         4.0e-07         6.4e-06  5.5e-07         8.8e-06
  (256, 3, 7)         7.7e-07         1.2e-05  7.6e-07         1.2e-05
  (257, 3, 7)         7.3e-07         1.2e-05  6.0e-07         9.6e-06
  (321, 3, 7)         7.2e-07         1.2e-05  9.9e-07         1.6e-05
  (129, 2, 7)         3.9e-07         6.2e-06  4.9e-07         7.8e-06
  clamp (5, 2, 3)     7.2e-08         1.9e-06  9.9e-08         1.9e-06
  (absolute, on h_after; tol = 16 * max(spread, 2^-23): see E_ULP)

  beta_row_tables: spreads of lc (absolute) and eg (relative, reference >=
  1e-30) over every grid point, and over the bulk of each curve (reference
  cdf >= 2^-10). The whole-curve figures are set by the deep lower tail
  (lc near -90): the kernel's exclusive scan is inclusive - local, which
  cancels where the pdf climbs by orders of magnitude per lane; the twin
  does the same. The bulk figures are the sharp ones. tol = 16 x each.

  (range, H, w)                   lc       eg       bulk lc  bulk eg
  --------------------------------------------------------------------
  ('wide', 1, 1.0)                1.3e-03  8.9e-04  6.6e-07  5.3e-06
  ('wide', 1, 2.0)                1.2e-04  7.5e-05  7.7e-07  6.7e-06
  ('wide', 2, 1.0)                9.6e-06  4.9e-06  5.5e-07  3.7e-06
  ('wide', 2, 2.0)                1.8e-05  5.8e-06  5.1e-07  5.7e-06
  ('wide', 3, 1.0)                2.1e-03  1.5e-03  9.0e-07  6.5e-06
  ('wide', 3, 2.0)                3.7e-03  2.6e-03  6.3e-07  7.2e-06
  ('wide', 67, 1.0)               4.4e-03  3.1e-03  1.0e-06  8.9e-06
  ('wide', 67, 2.0)               3.9e-03  2.7e-03  1.2e-06  9.4e-06
  ('moderate', 1, 1.0)            2.4e-04  1.7e-04  7.4e-07  5.2e-06
  ('moderate', 1, 2.0)            3.1e-04  2.1e-04  6.3e-07  6.0e-06
  ('moderate', 2, 1.0)            3.9e-03  2.7e-03  5.6e-07  6.0e-06
  ('moderate', 2, 2.0)            1.5e-03  9.8e-04  6.1e-07  4.7e-06
  ('moderate', 3, 1.0)            2.3e-04  1.6e-04  7.1e-07  6.0e-06
  ('moderate', 3, 2.0)            8.5e-04  5.9e-04  6.5e-07  4.6e-06
  ('moderate', 67, 1.0)           4.0e-03  2.8e-03  2.0e-06  6.8e-06
  ('moderate', 67, 2.0)           4.3e-03  3.0e-03  9.0e-07  7.5e-06
  ('concentrated', 1, 1.0)        1.6e-04  1.1e-04  4.2e-06  2.5e-05
  ('concentrated', 1, 2.0)        3.1e-04  2.2e-04  1.3e-05  1.5e-05
  ('concentrated', 2, 1.0)        6.8e-04  4.7e-04  2.7e-05  2.0e-05
  ('concentrated', 2, 2.0)        6.8e-04  4.8e-04  2.8e-05  1.6e-05
  ('concentrated', 3, 1.0)        4.0e-03  2.8e-03  1.1e-05  1.5e-05
  ('concentrated', 3, 2.0)        4.1e-03  2.8e-03  1.4e-05  1.8e-05
  ('concentrated', 67, 1.0)       9.8e-03  6.8e-03  5.8e-05  5.2e-05
  ('concentrated', 67, 2.0)       9.8e-03  6.9e-03  5.7e-05  5.6e-05
  ('singular0', 1, 1.0)           1.8e-06  1.2e-06  6.9e-07  1.2e-06
  ('singular0', 1, 2.0)           1.8e-06  2.7e-06  4.6e-07  1.7e-06
  ('singular0', 2, 1.0)           1.8e-06  2.2e-06  9.3e-07  2.2e-06
  ('singular0', 2, 2.0)           1.8e-06  1.5e-06  5.6e-07  1.5e-06
  ('singular0', 3, 1.0)           1.8e-06  3.5e-06  1.1e-06  2.6e-06
  ('singular0', 3, 2.0)           2.2e-06  3.6e-06  6.6e-07  1.7e-06
  ('singular0', 67, 1.0)          1.8e-06  7.4e-06  1.2e-06  7.4e-06
  ('singular0', 67, 2.0)          3.9e-06  6.8e-06  7.3e-07  6.8e-06

  commit (H, C, y)  eg rel   delta    s_base   dall     (spreads over the whole
                                                        row; tol = 16 x)
  ------------------------------------------------------------------------
  (5, 4, 0)         1.5e-04  2.5e-04  1.5e-04  3.5e-04
  (5, 4, 3)         7.4e-05  9.7e-05  3.8e-05  2.5e-05
  (5, 4, 2)         7.5e-04  1.3e-03  5.9e-05  8.8e-04
  (33, 300, 0)      1.7e-05  2.7e-05  1.8e-04  4.3e-05
  (33, 300, 299)    2.5e-05  4.6e-05  2.6e-04  6.4e-05
  (33, 300, 137)    1.8e-05  5.0e-05  1.8e-04  1.7e-04

Other bounds are reasoned, not measured: eig_totals alone is an fp32
sum of H non-negative inputs, off by at most H * 2^-24 relative in any
order; b_col is an fp32 sum of C positive terms minus one of them, off
by at most (C + 1) * 2^-24 of the row sum; a_col is a copy (exact); the
bf16/fp16 mirrors are conversions of the kernel's own fp32 values
(bitwise); egw is held to one bf16 ulp of the fp64 value.

The faults these tolerances must catch (a model dropped from a bucket,
the complement threshold, a dropped quarter of a long row, a v-select
bit, missing shard totals, swapped curve variants, a trapezoid counted
at lane 0, a commit to the wrong row) each move the reference by at
least 10 tolerances: tests/test_table_ref.py::TestToleranceFloors.
"""
from __future__ import annotations

import functools

import pytest
import torch

from tests import table_ref as TR
from tests.test_pair_kernels import HOST_BAND  # noqa: F401 (CPU checks)

pytestmark = pytest.mark.gpu

SEED = 0
MARGIN = 16.0

# es_build: (H, C) -> class-0 bucket sizes, one candidate row each
ES_CASES = {
    (70, 3): (0, 1, 2, 3, 34, 35, 36, 69, 70),
    (71, 3): (35, 36),
    (1024, 2): (0, 512, 513, 1024),
    (1026, 2): (0, 512, 513, 514, 1026),
    (1100, 3): (0, 1, 2, 3, 511, 512, 513, 549, 550, 551, 552, 587, 588,
                589, 1099, 1100),
}
# recorded max relative fp32-twin error of ES (rounded up)
E_ES = {
    (70, 3): 2e-06,
    (71, 3): 1.9e-06,
    (1024, 2): 1.5e-05,
    (1026, 2): 1.2e-05,
    (1100, 3): 1.2e-05,
}
# rows per branch (direct-short, complement-short, direct-long,
# complement-long), from the reference
ES_CENSUS = {
    (70, 3): (24, 3, 0, 0),
    (71, 3): (5, 1, 0, 0),
    (1024, 2): (5, 3, 0, 0),
    (1026, 2): (4, 4, 2, 0),
    (1100, 3): (30, 4, 11, 3),
}

# es_build_gathered: Hg -> bucket sizes (C = 3)
_G_SIZES = (0, 1, 2, 3, 4, 5, 7, 8, 9)
GATHERED_CASES = {Hg: tuple(n for n in _G_SIZES if n < Hg) + (Hg,)
                  for Hg in (1, 5, 70, 257)}
GATHERED_C = 3
E_GATHERED = {
    1: 7.5e-07,
    5: 7.7e-07,
    70: 1.7e-06,
    257: 4.3e-06,
}

# eig_assemble_k / eig_totals / eig_entropy: (H, C, B), consensus 0.6
ASSEMBLE_CASES = [(H, 3, 7) for H in (1, 2, 63, 64, 65, 128, 129, 130,
                                      192, 193, 256, 257, 321)] \
    + [(129, 2, 7)]
# recorded max |h_after fp32 twin - fp64|, per M dtype
E_ASSEMBLE = {
    ((1, 3, 7), 'fp32'): 0.0,
    ((1, 3, 7), 'bf16'): 0.0,
    ((2, 3, 7), 'fp32'): 6.5e-08,
    ((2, 3, 7), 'bf16'): 9.4e-08,
    ((63, 3, 7), 'fp32'): 3e-07,
    ((63, 3, 7), 'bf16'): 4.5e-07,
    ((64, 3, 7), 'fp32'): 5.2e-07,
    ((64, 3, 7), 'bf16'): 4.6e-07,
    ((65, 3, 7), 'fp32'): 5.1e-07,
    ((65, 3, 7), 'bf16'): 4.5e-07,
    ((128, 3, 7), 'fp32'): 5.2e-07,
    ((128, 3, 7), 'bf16'): 6.4e-07,
    ((129, 3, 7), 'fp32'): 5e-07,
    ((129, 3, 7), 'bf16'): 6.7e-07,
    ((130, 3, 7), 'fp32'): 4.9e-07,
    ((130, 3, 7), 'bf16'): 5.3e-07,
    ((192, 3, 7), 'fp32'): 6.4e-07,
    ((192, 3, 7), 'bf16'): 5.1e-07,
    ((193, 3, 7), 'fp32'): 4e-07,
    ((193, 3, 7), 'bf16'): 5.5e-07,
    ((256, 3, 7), 'fp32'): 7.7e-07,
    ((256, 3, 7), 'bf16'): 7.6e-07,
    ((257, 3, 7), 'fp32'): 7.3e-07,
    ((257, 3, 7), 'bf16'): 6e-07,
    ((321, 3, 7), 'fp32'): 7.2e-07,
    ((321, 3, 7), 'bf16'): 9.9e-07,
    ((129, 2, 7), 'fp32'): 3.9e-07,
    ((129, 2, 7), 'bf16'): 4.9e-07,
}
E_CLAMP = {'fp32': 7.2e-08, 'bf16': 9.9e-08}
SINGLE_SHARD_H = (1, 65, 129, 257)
TWO_SHARD_H = (65, 130)
M_DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16}

# beta_row_tables: (range, H, update_weight) -> (e_lc abs, e_eg rel,
# and the same two over the bulk of each curve, reference cdf >= 2^-10)
BULK_LC = -10.0
BETA_CASES = [(name, H, uw) for name in TR.BETA_RANGES
              for H in (1, 2, 3, 67) for uw in (1.0, 2.0)]
EG_FLOOR = 1e-30
E_BETA = {
    ('wide', 1, 1.0): (0.0013, 0.00089, 6.6e-07, 5.3e-06),
    ('wide', 1, 2.0): (0.00012, 7.5e-05, 7.7e-07, 6.7e-06),
    ('wide', 2, 1.0): (9.6e-06, 4.9e-06, 5.5e-07, 3.7e-06),
    ('wide', 2, 2.0): (1.8e-05, 5.8e-06, 5.1e-07, 5.7e-06),
    ('wide', 3, 1.0): (0.0021, 0.0015, 9e-07, 6.5e-06),
    ('wide', 3, 2.0): (0.0037, 0.0026, 6.3e-07, 7.2e-06),
    ('wide', 67, 1.0): (0.0044, 0.0031, 1e-06, 8.9e-06),
    ('wide', 67, 2.0): (0.0039, 0.0027, 1.2e-06, 9.4e-06),
    ('moderate', 1, 1.0): (0.00024, 0.00017, 7.4e-07, 5.2e-06),
    ('moderate', 1, 2.0): (0.00031, 0.00021, 6.3e-07, 6e-06),
    ('moderate', 2, 1.0): (0.0039, 0.0027, 5.6e-07, 6e-06),
    ('moderate', 2, 2.0): (0.0015, 0.00098, 6.1e-07, 4.7e-06),
    ('moderate', 3, 1.0): (0.00023, 0.00016, 7.1e-07, 6e-06),
    ('moderate', 3, 2.0): (0.00085, 0.00059, 6.5e-07, 4.6e-06),
    ('moderate', 67, 1.0): (0.004, 0.0028, 2e-06, 6.8e-06),
    ('moderate', 67, 2.0): (0.0043, 0.003, 9e-07, 7.5e-06),
    ('concentrated', 1, 1.0): (0.00016, 0.00011, 4.2e-06, 2.5e-05),
    ('concentrated', 1, 2.0): (0.00031, 0.00022, 1.3e-05, 1.5e-05),
    ('concentrated', 2, 1.0): (0.00068, 0.00047, 2.7e-05, 2e-05),
    ('concentrated', 2, 2.0): (0.00068, 0.00048, 2.8e-05, 1.6e-05),
    ('concentrated', 3, 1.0): (0.004, 0.0028, 1.1e-05, 1.5e-05),
    ('concentrated', 3, 2.0): (0.0041, 0.0028, 1.4e-05, 1.8e-05),
    ('concentrated', 67, 1.0): (0.0098, 0.0068, 5.8e-05, 5.2e-05),
    ('concentrated', 67, 2.0): (0.0098, 0.0069, 5.7e-05, 5.6e-05),
    ('singular0', 1, 1.0): (1.8e-06, 1.2e-06, 6.9e-07, 1.2e-06),
    ('singular0', 1, 2.0): (1.8e-06, 2.7e-06, 4.6e-07, 1.7e-06),
    ('singular0', 2, 1.0): (1.8e-06, 2.2e-06, 9.3e-07, 2.2e-06),
    ('singular0', 2, 2.0): (1.8e-06, 1.5e-06, 5.6e-07, 1.5e-06),
    ('singular0', 3, 1.0): (1.8e-06, 3.5e-06, 1.1e-06, 2.6e-06),
    ('singular0', 3, 2.0): (2.2e-06, 3.6e-06, 6.6e-07, 1.7e-06),
    ('singular0', 67, 1.0): (1.8e-06, 7.4e-06, 1.2e-06, 7.4e-06),
    ('singular0', 67, 2.0): (3.9e-06, 6.8e-06, 7.3e-07, 6.8e-06),
}

# table_commit_*: (H, C, y) -> (e_eg rel, e_delta, e_s_base, e_dall abs)
COMMIT_CASES = [(5, 4, 0), (5, 4, 3), (5, 4, 2),
                (33, 300, 0), (33, 300, 299), (33, 300, 137)]
E_COMMIT = {
    (5, 4, 0): (0.00015, 0.00025, 0.00015, 0.00035),
    (5, 4, 3): (7.4e-05, 9.7e-05, 3.8e-05, 2.5e-05),
    (5, 4, 2): (0.00075, 0.0013, 5.9e-05, 0.00088),
    (33, 300, 0): (1.7e-05, 2.7e-05, 0.00018, 4.3e-05),
    (33, 300, 299): (2.5e-05, 4.6e-05, 0.00026, 6.4e-05),
    (33, 300, 137): (1.8e-05, 5e-05, 0.00018, 0.00017),
}


# ---------------------------------------------------------------------
# CPU-side references and measurements (shared with test_table_ref.py)
# ---------------------------------------------------------------------

def es_inputs(case):
    return TR.make_es_inputs(*case, ES_CASES[case], seed=SEED)


@functools.lru_cache(maxsize=None)
def es_ref(case):
    i = es_inputs(case)
    return TR.ref_es_build(i.s_base, i.delta, i.dall, i.hvals, i.offsets,
                           i.w)


def census(branch) -> tuple:
    return tuple(int((branch == k).sum()) for k in range(4))


def measure_e_es(case) -> float:
    i = es_inputs(case)
    twin, _ = TR.ref_es_build(i.s_base, i.delta, i.dall, i.hvals,
                              i.offsets, i.w, f32=True)
    return TR.rel_err(twin, es_ref(case)[0])


def gathered_inputs(Hg):
    return TR.make_es_inputs(Hg, GATHERED_C, GATHERED_CASES[Hg], seed=SEED,
                             gathered=True)


@functools.lru_cache(maxsize=None)
def gathered_ref(Hg):
    i = gathered_inputs(Hg)
    return TR.ref_es_build_gathered(i.s_base, i.sel_all, i.hvals,
                                    i.offsets, i.w)


def measure_e_gathered(Hg) -> float:
    i = gathered_inputs(Hg)
    twin = TR.ref_es_build_gathered(i.s_base, i.sel_all, i.hvals,
                                    i.offsets, i.w, f32=True)
    return TR.rel_err(twin, gathered_ref(Hg))


@functools.lru_cache(maxsize=None)
def assemble_inputs(case, dt):
    """(inputs, M rounded once to the dtype under test)."""
    ai = TR.make_clamp_inputs() if case == "clamp" \
        else TR.make_assemble_inputs(*case, seed=SEED)
    return ai, ai.M.to(M_DTYPES[dt])


@functools.lru_cache(maxsize=None)
def assemble_ref(case, dt):
    ai, M = assemble_inputs(case, dt)
    return TR.ref_assemble(M, ai.cls, ai.pi_hat, ai.pbest_before,
                           ai.mixture0)


def measure_e_assemble(case, dt) -> float:
    ai, M = assemble_inputs(case, dt)
    twin = TR.ref_assemble(M, ai.cls, ai.pi_hat, ai.pbest_before,
                           ai.mixture0, f32=True)
    return float((twin - assemble_ref(case, dt)).abs().max())


# One fp32 ulp of m = 1. At H = 1 the only model's share is tot / tot
# and the twin's 21 rows all came out exact (spread 0), but x * (1 / x)
# in fp32 may miss 1 by an ulp, which moves -m log2 m by 1.7e-7: no
# recorded spread counts for less than the format's own resolution.
E_ULP = 2.0 ** -23


def assemble_tol(case, dt) -> float:
    rec = E_CLAMP[dt] if case == "clamp" else E_ASSEMBLE[(case, dt)]
    return MARGIN * max(rec, E_ULP)


@functools.lru_cache(maxsize=None)
def beta_ref(name, H, uw):
    a, b = TR.make_beta_cols(name, H, seed=SEED)
    return TR.ref_beta_row_curves(a, b, uw)


def beta_errs(eg, lc, name, H, uw):
    """(max |lc - ref|, max relative eg error where ref >= EG_FLOOR),
    over every element and over the bulk (reference lc >= BULK_LC)."""
    eg64, lc64 = beta_ref(name, H, uw)
    bulk = lc64 >= BULK_LC
    assert bool(bulk.any(-1).all()), "a curve without bulk points"
    return (float((lc.double() - lc64).abs().max()),
            TR.rel_err(eg, eg64, EG_FLOOR),
            float((lc.double() - lc64).abs()[bulk].max()),
            TR.rel_err(eg[bulk], eg64[bulk], EG_FLOOR))


def measure_e_beta(name, H, uw):
    a, b = TR.make_beta_cols(name, H, seed=SEED)
    return beta_errs(*TR.ref_beta_row_curves(a, b, uw, f32=True),
                     name, H, uw)


def commit_inputs(H, C):
    return TR.make_commit_inputs(H, C, seed=SEED)


@functools.lru_cache(maxsize=None)
def commit_ref(H, C, y):
    ci = commit_inputs(H, C)
    return TR.ref_commit_row(ci.dirichlets, y, ci.weights, 1.0)


def commit_errs(EG, delta, s_base, dall, ref):
    return (TR.rel_err(EG, ref.EG, EG_FLOOR),
            float((delta.double() - ref.delta).abs().max()),
            float((s_base.double() - ref.s_base).abs().max()),
            float((dall.double() - ref.dall).abs().max()))


def measure_e_commit(H, C, y):
    ci = commit_inputs(H, C)
    t = TR.ref_commit_row(ci.dirichlets, y, ci.weights, 1.0, f32=True)
    return commit_errs(t.EG, t.delta, t.s_base, t.dall, commit_ref(H, C, y))


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


def _poison(dev, *shape):
    """Best effort against a torch::empty output left unwritten: fill
    the allocator's next block of this size with NaN and free it."""
    junk = torch.full(shape, float("nan"), device=dev)
    del junk


class TestEsBuild:
    @pytest.mark.parametrize("case", list(ES_CASES))
    def test_es_build_vs_fp64(self, ext, dev, case):
        """es_build_kernel + es_build_long_kernel, fp32 and bf16 output,
        against ref_es_build; the branch census proves which of the two
        kernels and which form produced the rows."""
        H, C = case
        i = es_inputs(case)
        ref, branch = es_ref(case)
        B = i.hvals.shape[0]
        assert census(branch) == ES_CENSUS[case], census(branch)
        assert float(ref.min()) >= TR.PR.F32_MIN_NORMAL
        assert float(ref.max()) < 3e38
        args = [t.to(dev) for t in (i.s_base, i.delta, i.dall, i.hvals,
                                    i.offsets, i.w)]
        _poison(dev, C, B, TR.P)
        got = ext.es_build(*args, False)
        got16 = ext.es_build(*args, True)
        again = ext.es_build(*args, False)
        assert got.shape == (C, B, TR.P) and got.dtype == torch.float32
        assert got16.dtype == torch.bfloat16
        assert not bool(torch.isnan(got).any())
        got, got16 = got.cpu(), got16.cpu()
        err = TR.rel_err(got, ref)
        tol = MARGIN * E_ES[case]
        print(f"es_build {case}: B={B} census {census(branch)} "
              f"rel err {err:.3g} tol {tol:.3g}")
        assert err <= tol, (case, err)
        assert torch.equal(got, again.cpu()), "second launch differs"
        assert torch.equal(got16, got.to(torch.bfloat16)), \
            int((got16 != got.to(torch.bfloat16)).sum())


class TestEsBuildGathered:
    @pytest.mark.parametrize("Hg", list(GATHERED_CASES))
    def test_gathered_vs_fp64(self, ext, dev, Hg):
        """es_build_gathered: the 4-way unroll and its tail (bucket
        sizes 0..9 and Hg), fp32 and bf16 output."""
        i = gathered_inputs(Hg)
        ref = gathered_ref(Hg)
        B, C = i.hvals.shape[0], GATHERED_C
        assert (B * C) % 4 != 0
        n = (i.offsets[:, 1:] - i.offsets[:, :-1])
        assert set(GATHERED_CASES[Hg]) <= set(n.flatten().tolist())
        assert float(ref.min()) >= TR.PR.F32_MIN_NORMAL
        args = [t.to(dev) for t in (i.s_base, i.sel_all, i.hvals,
                                    i.offsets, i.w)]
        _poison(dev, C, B, TR.P)
        got = ext.es_build_gathered(*args, False).cpu()
        got16 = ext.es_build_gathered(*args, True).cpu()
        assert got.shape == (C, B, TR.P)
        assert not bool(torch.isnan(got).any())
        err = TR.rel_err(got, ref)
        tol = MARGIN * E_GATHERED[Hg]
        print(f"es_build_gathered Hg={Hg}: B={B} rel err {err:.3g} "
              f"tol {tol:.3g}")
        assert err <= tol, (Hg, err)
        assert torch.equal(got16, got.to(torch.bfloat16))


def _assemble_dev(ai, M, dev):
    return (M.to(dev).contiguous(), ai.cls.to(torch.int32).to(dev),
            ai.pi_hat.to(dev), ai.pbest_before.to(dev).contiguous(),
            ai.mixture0.to(dev))


class TestAssemble:
    @pytest.mark.parametrize("dt", list(M_DTYPES))
    @pytest.mark.parametrize("case", ASSEMBLE_CASES + ["clamp"])
    def test_assemble_vs_fp64(self, ext, dev, case, dt):
        """eig_assemble_k (model axis strided by 256 with four guarded
        terms, then by 128) on H across every stride boundary, and the
        two clamps."""
        ai, M = assemble_inputs(case, dt)
        ref = assemble_ref(case, dt)
        if case == "clamp":
            tot = TR.ref_totals(M, ai.cls)
            assert float(tot[1, 0]) == 0.0
        else:
            v = ai.cls.unsqueeze(1) == torch.arange(case[1]).view(1, -1, 1)
            assert bool(v.any()) and not bool(v.all())
        got = ext.eig_assemble_k(*_assemble_dev(ai, M, dev)).cpu()
        assert got.shape == ref.shape and torch.isfinite(got).all()
        err = float((got.double() - ref).abs().max())
        tol = assemble_tol(case, dt)
        print(f"eig_assemble_k {case} {dt}: err {err:.3g} tol {tol:.3g}")
        assert err <= tol, (case, dt, err)

    @pytest.mark.parametrize("dt", list(M_DTYPES))
    @pytest.mark.parametrize("H", SINGLE_SHARD_H)
    def test_totals_entropy_single_shard(self, ext, dev, H, dt):
        """eig_entropy(M, cls, eig_totals(M, cls)) is eig_assemble_k's
        contract; eig_totals alone against ref_totals."""
        case = (H, 3, 7)
        ai, M = assemble_inputs(case, dt)
        m, cls, pi, pb, mix = _assemble_dev(ai, M, dev)
        tot = ext.eig_totals(m, cls)
        tot64 = TR.ref_totals(M, ai.cls)
        e_tot = TR.rel_err(tot.cpu(), tot64)
        assert e_tot <= H * 2.0 ** -24, (H, e_tot)
        got = ext.eig_entropy(m, cls, tot, pi, pb, mix).cpu()
        err = float((got.double() - assemble_ref(case, dt)).abs().max())
        print(f"totals+entropy H={H} {dt}: tot rel {e_tot:.3g} "
              f"err {err:.3g} tol {assemble_tol(case, dt):.3g}")
        assert err <= assemble_tol(case, dt), (H, dt, err)

    @pytest.mark.parametrize("dt", list(M_DTYPES))
    @pytest.mark.parametrize("H", TWO_SHARD_H)
    def test_two_shard_emulation(self, ext, dev, H, dt):
        """Stride sharding without a communicator: rank r holds models
        h % 2 == r; the partial totals, then the partial entropies, are
        added on the host in rank order and must match the full-H
        reference."""
        case = (H, 3, 7)
        ai, M = assemble_inputs(case, dt)
        C, B = M.shape[0], M.shape[1]
        shards = []
        for r in range(2):
            Mr = M.view(C, B, H, 2)[:, :, r::2].reshape(C, B, -1)
            sub = ai._replace(cls=ai.cls[:, r::2].contiguous(),
                              pbest_before=ai.pbest_before[:, r::2],
                              mixture0=ai.mixture0[r::2].contiguous())
            shards.append(_assemble_dev(sub, Mr, dev))
        assert shards[0][1].shape[1] == (H + 1) // 2
        assert shards[1][1].shape[1] == H // 2
        parts = [ext.eig_totals(s[0], s[1]) for s in shards]
        tot = parts[0] + parts[1]
        e_tot = TR.rel_err(tot.cpu(), TR.ref_totals(M, ai.cls))
        assert e_tot <= H * 2.0 ** -24, (H, e_tot)
        ents = [ext.eig_entropy(s[0], s[1], tot, *s[2:]) for s in shards]
        got = (ents[0] + ents[1]).cpu()
        err = float((got.double() - assemble_ref(case, dt)).abs().max())
        print(f"two-shard H={H} {dt}: err {err:.3g} "
              f"tol {assemble_tol(case, dt):.3g}")
        assert err <= assemble_tol(case, dt), (H, dt, err)


class TestBetaRowTables:
    @pytest.mark.parametrize("name,H,uw", BETA_CASES)
    def test_curves_vs_fp64(self, ext, dev, name, H, uw):
        """beta_row_tables against the fp64 curves: lc absolutely, eg
        relatively wherever the reference is >= 1e-30 (below it the
        kernel's value must be below it too)."""
        a, b = TR.make_beta_cols(name, H, seed=SEED)
        eg64, _ = beta_ref(name, H, uw)
        assert torch.isfinite(eg64).all() and float(eg64.max()) < 3e38
        eg, lc = ext.beta_row_tables(a.to(dev), b.to(dev), uw)
        eg, lc = eg.cpu(), lc.cpu()
        assert eg.shape == (H, 2, TR.P) == lc.shape
        assert torch.isfinite(eg).all() and torch.isfinite(lc).all()
        errs = beta_errs(eg, lc, name, H, uw)
        rec = E_BETA[(name, H, uw)]
        r_eg = rec[1]
        print(f"beta_row_tables {(name, H, uw)}: lc / eg / bulk lc / "
              "bulk eg " + " ".join(f"{e:.3g} (tol {MARGIN * r:.3g})"
                                    for e, r in zip(errs, rec)))
        for e, r, what in zip(errs, rec, ("lc", "eg", "bulk lc",
                                          "bulk eg")):
            assert e <= MARGIN * r, (name, H, uw, what, e)
        small = eg64 < EG_FLOOR
        assert bool((eg.double()[small]
                     <= EG_FLOOR * (1 + MARGIN * r_eg)).all())


def _check_committed(got, before, ref, y, tols, label):
    """Row y of the seven tables against the reference row, the mirrors
    bitwise from the kernel's own fp32 rows, every other row untouched."""
    C = before["EG"].shape[0]
    others = torch.arange(C) != y
    for name in TR.TABLE_NAMES:
        assert torch.equal(got[name][others], before[name][others]), \
            f"{label}: {name} rows other than y changed"
    H = got["EG"].shape[1]
    errs = commit_errs(got["EG"][y], got["delta"][y], got["s_base"][y],
                       got["dall"][y], ref)
    print(f"{label}: eg {errs[0]:.3g} delta {errs[1]:.3g} s_base "
          f"{errs[2]:.3g} dall {errs[3]:.3g} tol "
          + " ".join(f"{MARGIN * t:.3g}" for t in tols))
    for e, t, what in zip(errs, tols, ("EG", "delta", "s_base", "dall")):
        assert e <= MARGIN * t, (label, what, e)
    small = ref.EG < EG_FLOOR
    assert bool((got["EG"][y].double()[small]
                 <= EG_FLOOR * (1 + MARGIN * tols[0])).all())
    assert torch.equal(got["eg16"][y],
                       got["EG"][y].reshape(2 * H, -1).to(torch.bfloat16))
    assert torch.equal(got["delta16"][y],
                       got["delta"][y].to(torch.float16))
    assert bool(TR.PR.a_operand_ok(got["egw"][y], ref.egw).all()), \
        f"{label}: egw off by more than one bf16 ulp"


def _call_order(t, weights):
    return (t["EG"], t["delta"], t["s_base"], weights, t["eg16"], t["egw"],
            t["delta16"], t["dall"])


class TestTableCommit:
    @pytest.mark.parametrize("H,C,y", COMMIT_CASES)
    def test_commit_row_vs_fp64(self, ext, dev, H, C, y):
        """table_commit_row: a_col / b_col, row y of all seven tables,
        all other rows untouched; then a second commit with the SAME y
        tensor refilled in place (y is read from device memory)."""
        ci = commit_inputs(H, C)
        ref = commit_ref(H, C, y)
        before = ci.tables
        t = {k: v.clone().to(dev) for k, v in before.items()}
        w = ci.weights.to(dev)
        dirs = ci.dirichlets.to(dev)
        y_t = torch.tensor([y], dtype=torch.int64, device=dev)
        a_col, b_col = ext.table_commit_row(dirs, y_t, *_call_order(t, w),
                                            1.0)
        assert torch.equal(a_col.cpu().double(), ref.a_col)
        row_sum = ci.dirichlets[:, y, :].double().sum(-1)
        e_b = float(((b_col.cpu().double() - ref.b_col).abs()
                     / row_sum).max())
        assert e_b <= (C + 1) * 2.0 ** -24, e_b
        got = {k: v.cpu() for k, v in t.items()}
        _check_committed(got, before, ref, y, E_COMMIT[(H, C, y)],
                         f"commit_row {(H, C, y)}")
        # same tensor object, new class: the label graph's replay
        y2 = (y + 1) % C
        y_t.fill_(y2)
        ext.table_commit_row(dirs, y_t, *_call_order(t, w), 1.0)
        got2 = {k: v.cpu() for k, v in t.items()}
        for name in TR.TABLE_NAMES:
            assert torch.equal(got2[name][y], got[name][y]), name
        if (H, C, y2) in E_COMMIT:
            tols2 = E_COMMIT[(H, C, y2)]
        else:   # an unrecorded neighbour row: its own twin figure
            tols2 = measure_e_commit(H, C, y2)
        _check_committed(got2, got, commit_ref(H, C, y2), y2, tols2,
                         f"commit_row refilled y {(H, C, y2)}")

    @pytest.mark.parametrize("H,C,y", COMMIT_CASES)
    def test_commit_cols_vs_fp64(self, ext, dev, H, C, y):
        """table_commit_cols (host y, caller's columns): same rows."""
        ci = commit_inputs(H, C)
        ref = commit_ref(H, C, y)
        a = ref.a_col.float()
        b = ref.b_col.float()
        ref_cols = TR.ref_commit_cols(a, b, ci.weights, 1.0)
        before = ci.tables
        t = {k: v.clone().to(dev) for k, v in before.items()}
        ext.table_commit_cols(a.to(dev), b.to(dev), y,
                              *_call_order(t, ci.weights.to(dev)), 1.0)
        got = {k: v.cpu() for k, v in t.items()}
        _check_committed(got, before, ref_cols, y, E_COMMIT[(H, C, y)],
                         f"commit_cols {(H, C, y)}")


class TestHostRejections:
    """Argument checks that fail in a TORCH_CHECK before any launch."""

    @staticmethod
    def _m(dev, C=2, B=3, H=4):
        return (torch.ones(C, B, 2 * H, device=dev),
                torch.zeros(B, H, dtype=torch.int32, device=dev),
                torch.ones(B, C, device=dev),
                torch.full((C,), 0.5, device=dev),
                torch.full((C, H), 0.25, device=dev),
                torch.full((H,), 0.25, device=dev))

    @pytest.mark.parametrize("bad,msg", [
        (lambda c: c.long(), "int32"),
        (lambda c: c.t().contiguous().t(), "contiguous"),
        (lambda c: c[:, :3].contiguous(), r"\(B, H\)"),
        (lambda c: c[:2].contiguous(), r"\(B, H\)"),
        (lambda c: c.cpu(), "ROCm device"),
    ])
    def test_cls_checked(self, ext, dev, bad, msg):
        m, cls, tot, pi, pb, mix = self._m(dev)
        with pytest.raises(RuntimeError, match=msg):
            ext.eig_totals(m, bad(cls))
        with pytest.raises(RuntimeError, match=msg):
            ext.eig_entropy(m, bad(cls), tot, pi, pb, mix)
        with pytest.raises(RuntimeError, match=msg):
            ext.eig_assemble_k(m, bad(cls), pi, pb, mix)
        ext.eig_entropy(m, cls, ext.eig_totals(m, cls), pi, pb, mix)

    @staticmethod
    def _es(dev, C=2, B=3, H=4):
        return {"s_base": torch.zeros(C, 256, device=dev),
                "delta": torch.zeros(C, H, 256, device=dev),
                "dall": torch.zeros(C, 256, device=dev),
                "hvals": torch.arange(H, dtype=torch.int32, device=dev)
                .repeat(B, 1),
                "offsets": torch.zeros(B, C + 1, dtype=torch.int32,
                                       device=dev),
                "w": torch.ones(256, device=dev)}

    @pytest.mark.parametrize("name,bad,msg", [
        ("hvals", lambda t: t[:, :3].contiguous(), r"hvals must be \(B, H\)"),
        ("offsets", lambda t: t[:, :2].contiguous(), r"\(B, C\+1\)"),
        ("offsets", lambda t: t[:2].contiguous(), r"\(B, C\+1\)"),
        ("dall", lambda t: t[:1].contiguous(), r"dall must be \(C, 256\)"),
        ("delta", lambda t: t[:1].contiguous(), r"delta.size\(0\)"),
    ])
    def test_es_build_shapes_checked(self, ext, dev, name, bad, msg):
        a = self._es(dev)
        a[name] = bad(a[name])
        with pytest.raises(RuntimeError, match=msg):
            ext.es_build(*a.values(), False)

    @pytest.mark.parametrize("shape", [(3, 3, 256), (2, 4, 256),
                                       (3, 4, 128), (3, 1024)])
    def test_es_build_gathered_sel_all_checked(self, ext, dev, shape):
        a = self._es(dev)
        sel = torch.zeros(*shape, device=dev)
        with pytest.raises(RuntimeError, match=r"sel_all must be"):
            ext.es_build_gathered(a["s_base"], sel, a["hvals"],
                                  a["offsets"], a["w"], False)
        ext.es_build_gathered(a["s_base"], torch.zeros(3, 4, 256,
                                                       device=dev),
                              a["hvals"], a["offsets"], a["w"], False)
