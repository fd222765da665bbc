"""CPU checks of the v1 P(best) / EIG fp64 stage references
(tests/pbest_ref.py) and of the tolerances tests/test_pbest_kernels.py
derives from them: the references are the project's contract, every
recorded spread is re-measured, the inputs meet the conditions the GPU
module relies on, and each tolerance keeps a floor against the fault it
exists for."""
from __future__ import annotations

import numpy as np
import pytest
import torch

from coda_amd.ops import reference as R
from tests import pbest_ref as PB
from tests import table_ref as TR
from tests import test_pbest_kernels as TPK
from tests.test_ops import _pbest_fp64

BAND = TPK.HOST_BAND


def _in_band(measured: float, recorded: float):
    """measured within HOST_BAND of the recorded figure; a recorded 0
    (counted as E_ULP by the GPU module) only has to stay below E_ULP."""
    assert measured <= max(recorded, TPK.E_ULP) * BAND, (measured, recorded)
    if recorded > 0:
        assert measured >= recorded / BAND, (measured, recorded)


def _all_in_band(measured, recorded):
    assert len(measured) == len(recorded)
    for m, r in zip(measured, recorded):
        _in_band(m, r)


class TestReferencesAreTheContract:
    @pytest.mark.parametrize("fam,R_,H", [
        ("wide", 3, 5), ("moderate", 2, 17), ("singular_ab", 2, 9),
        ("competitive", 2, 12)])
    def test_ref_pbest_is_the_scipy_golden_and_the_eager_op(self, fam, R_,
                                                            H):
        a, b = PB.make_betas(fam, R_, H, seed=5)
        ref = PB.ref_pbest(a, b)
        # the golden integrates with the fp64 grid step, the contract
        # with the fp32 one: a common factor 1 + 1e-8 on every cdf and
        # mass, which normalisation removes
        np.testing.assert_allclose(ref.numpy(), _pbest_fp64(a, b),
                                   rtol=1e-7, atol=1e-12)
        eager = R.pbest_from_beta(a.double(), b.double())
        np.testing.assert_allclose(eager.numpy(), ref.numpy(),
                                   rtol=1e-7, atol=1e-12)
        if fam in ("wide", "moderate"):
            # the eager op in fp32, at tests/test_ops.py's tolerance.
            # Not the other two: its fp32 log-pdf cancels at large
            # counts, and its fp32 grid cannot hold 1 - 1e-6 (one ulp
            # is 6 % of 1 - x there), which a pdf singular at 1 shows
            np.testing.assert_allclose(
                R.pbest_from_beta(a, b).double().numpy(), ref.numpy(),
                rtol=2e-4, atol=2e-6)

    @pytest.mark.parametrize("H", [1, 5, 7, 64, 257])
    def test_windowed_forms_are_the_same_contract(self, H):
        """In fp64 the row kernel's four windows and the wide split are
        ref_pbest."""
        a, b = PB.make_betas("moderate", 1, H, seed=6)
        ref = PB.ref_pbest(a, b)
        assert float((PB.ref_pbest_row(a, b) - ref).abs().max()) <= 1e-13
        for hc in (3, 64, 512):
            got = PB.ref_pbest_windows(a, b, hc)
            assert float((got - ref).abs().max()) <= 1e-13, hc

    def test_row_kernel_windows(self):
        """H = 5: windows of 2 at 0, 2, 4 and an empty one whose start
        (6) lies past H; H < 4 leaves empty windows."""
        assert PB.windows(5, 2, 4) == [(0, 2), (2, 4), (4, 5), (5, 5)]
        assert PB.windows(2, 1, 4) == [(0, 1), (1, 2), (2, 2), (2, 2)]
        assert PB.windows(257, 100) == [(0, 100), (100, 200), (200, 257)]
        assert PB.windows(70, 512) == [(0, 70)]

    @pytest.mark.parametrize("w", [1.0, 0.5])
    def test_hyp_betas_and_the_eig_composition(self, w):
        i = PB.make_hyp_inputs(9, 4, 6, seed=3)
        B, C, H = 6, 4, 9
        a, b = PB.ref_hyp_betas(i.alpha_cc, i.beta_cc, i.cls, w)
        ea, eb = R.hypothetical_betas(i.alpha_cc, i.beta_cc, i.cls, w)
        assert torch.equal(a.reshape(B, C, H), ea)
        assert torch.equal(b.reshape(B, C, H), eb)
        h = PB.ref_h_after(i.alpha_cc, i.beta_cc, i.cls, w, i.pi_hat,
                           i.pbest_before, i.mixture0)
        hb = torch.tensor(3.0, dtype=torch.float64)
        want = R.eig_assemble(
            PB.ref_pbest(a, b).reshape(B, C, H), i.pbest_before.double(),
            i.pi_hat.double(), i.pi_hat_xi.double(), i.mixture0.double(),
            hb)
        got = hb - (i.pi_hat_xi.double() * h).sum(-1)
        assert float((got - want).abs().max()) <= 1e-12


class TestRecordedSpreads:
    """Every figure recorded in test_pbest_kernels.py, re-measured (each
    measure_* also asserts that the fp32 twin is finite)."""

    @pytest.mark.parametrize("case", TPK.PBEST_CASES + TPK.CEILING_CASES)
    def test_pbest(self, case):
        _all_in_band(TPK.measure_e_pbest(*case), TPK.E_PBEST[case])

    @pytest.mark.parametrize("case", TPK.ROW_CASES)
    def test_row(self, case):
        _all_in_band(TPK.measure_e_row(*case), TPK.E_ROW[case])

    @pytest.mark.parametrize("case", TPK.PHASE_CASES)
    def test_phase(self, case):
        _all_in_band(TPK.measure_e_phase(*case), TPK.E_PHASE[case])

    @pytest.mark.parametrize("case", TPK.WIDE_CASES)
    def test_wide(self, case):
        _all_in_band(TPK.measure_e_wide(*case), TPK.E_WIDE[case])

    def test_wide_end_to_end(self):
        _all_in_band(TPK.measure_e_wide_e2e(), TPK.E_WIDE_E2E)

    @pytest.mark.parametrize("case", TPK.EIG_CASES)
    def test_eig(self, case):
        _all_in_band(TPK.measure_e_eig(case), TPK.E_EIG[case])

    def test_eig_clamp_and_dense(self):
        _in_band(TPK.measure_e_eig("clamp")[4], TPK.E_EIG_CLAMP)
        _in_band(TPK.measure_e_dense(), TPK.E_EIG_DENSE)


def _check_rows(fam, p):
    for row in p:
        assert PB.row_conditions(fam, row), (fam, float(row.max()))


class TestInputConditions:
    @pytest.mark.parametrize("case", TPK.PBEST_CASES + TPK.CEILING_CASES)
    def test_pbest_rows(self, case):
        """Big entries hold >= 99 % of every row; no competitive row
        with H >= 3 has an entry above 0.9."""
        _check_rows(case[0], TPK.pbest_ref(*case))

    @pytest.mark.parametrize("case", TPK.ROW_CASES)
    def test_row_kernel_rows(self, case):
        _check_rows(case[0], TPK.row_ref(*case))

    def test_wide_end_to_end_rows(self):
        _check_rows(TPK.WIDE_E2E[0], TPK.wide_e2e_ref())

    def test_competitive_rows_are_contested(self):
        """What the family is for: at H >= 63 several models hold a
        visible share (the independent concentrated draw has one at
        1.000)."""
        for case in TPK.PBEST_CASES:
            if case[0] == "competitive" and case[2] >= 63:
                p = TPK.pbest_ref(*case)
                assert int((p >= 0.02).sum(-1).min()) >= 3, case

    @pytest.mark.parametrize("case", TPK.PHASE_CASES)
    def test_phase_rows_have_a_bulk(self, case):
        ref = TPK.phase_ref(*case)
        assert bool(ref.bulk.any(-1).all())
        assert bool(torch.isfinite(ref.masses).all())
        # every relative figure is taken on normal fp32 numbers
        assert float(ref.total.min()) >= TR.PR.F32_MIN_NORMAL

    def test_virtual_shard_matters(self):
        """The global term is not the local one (how much that moves
        the masses: TestToleranceFloors, couple_local)."""
        for case in TPK.PHASE_CASES:
            ref = TPK.phase_ref(*case)
            d = (ref.slog2_in.double() - ref.slog2).abs()
            if case[0] in PB.END_RANGES:
                assert float(d.max()) <= 1e-4
            else:
                assert float(d.max()) >= 0.5, case

    def test_end_rows_load_the_end_points(self):
        """H = 1 and a < 1 (b < 1): the half-weighted end point holds a
        large part of the unnormalised mass."""
        for fam, pt in (("end0", 0), ("end255", TR.P - 1)):
            a, b = TPK.betas(fam, 2, 1)
            _, pdf, _ = TR.curves(a, b)
            ref = TPK.phase_ref(fam, 2, 1)
            end = 0.5 * pdf[:, 0, pt] * PB._dxf()
            assert float((end / ref.masses[:, 0]).min()) >= 0.05, fam

    @pytest.mark.parametrize("case", TPK.WIDE_CASES)
    def test_wide_windows(self, case):
        fam, R_, H, hc = case
        wins = PB.windows(H, hc)
        assert wins[-1][1] == H and all(h1 > h0 for h0, h1 in wins)
        ref = TPK.wide_ref(*case)
        assert ref.parts.shape[0] == len(wins) == -(-H // min(hc, H))
        assert bool(ref.bulk.any(-1).all())
        assert float(ref.tot_part.min()) >= TR.PR.F32_MIN_NORMAL

    def test_wide_shapes_cover_the_edges(self):
        tails = {(H, hc): PB.windows(H, hc) for _, _, H, hc in
                 TPK.WIDE_CASES}
        assert tails[(130, 64)][-1] == (128, 130)      # uneven tail
        assert tails[(128, 64)][-1] == (64, 128)       # exact multiple
        assert tails[(65, 64)][-1] == (64, 65)         # one-model tail
        assert len(tails[(70, 512)]) == 1              # hc > H
        assert len(tails[(257, 100)]) == 3

    @pytest.mark.parametrize("case", TPK.EIG_CASES)
    def test_hit_census(self, case):
        """Some (b, c) row has no hit, some has every model hit, some
        has exactly one; B * C leaves the last block ragged."""
        H, C, B, w = case
        i, _ = TPK.eig_inputs(case)
        hits = (i.cls.unsqueeze(1) == torch.arange(C).view(1, C, 1)).sum(-1)
        census = set(hits.flatten().tolist())
        assert {0, 1, H} <= census, census
        assert int(hits[0, 0]) == H and int(hits[1, C - 1]) == 1
        assert (B * C) % PB.ROWS_PER_BLOCK != 0
        ref = TPK.eig_ref(case)
        assert bool(ref.phase.bulk.any(-1).all())
        assert float(ref.a.min()) >= 1 and float(ref.b.min()) >= 1

    def test_clamp_case_clamps(self):
        i, w = TPK.eig_inputs("clamp")
        a, b = PB.ref_hyp_betas(i.alpha_cc, i.beta_cc, i.cls, w)
        pb = PB.ref_pbest(a, b)
        C = i.alpha_cc.shape[1]
        pc = torch.arange(pb.shape[0]) % C
        mm = i.mixture0.double() + i.pi_hat.double()[pc].unsqueeze(1) * (
            pb - i.pbest_before.double()[pc])
        assert bool((mm < 1e-12).any()) and bool((mm > 1e-3).any())


def _ratio(errs, recs) -> float:
    """Largest move, in tolerances, over a case's figures."""
    return max(e / TPK.tol(r) for e, r in zip(errs, recs))


class TestToleranceFloors:
    """Each fault is applied to the fp64 reference and must move it by
    at least FLOOR tolerances on at least one case of every kernel it
    could live in (the GPU test sees every case). Loosening a tolerance
    until these fail is loosening it until the GPU test means nothing;
    inputs, not tolerances, are what may change here."""

    FLOOR = 10.0

    def _caught(self, ratios, what, need=1):
        hit = [c for c, r in ratios.items() if r >= self.FLOOR]
        print(f"{what}: caught on {len(hit)} of {len(ratios)} cases, "
              f"max {max(ratios.values()):.3g} tolerances")
        assert len(hit) >= need, (what, ratios)
        return hit

    # -- pbest_kernel / pbest_row_kernel (normalised) -------------------

    @pytest.mark.parametrize("fault", ["drop_last", "lane0_trapezoid"])
    def test_generic_kernel(self, fault):
        ratios = {}
        for case in TPK.PBEST_CASES:
            if case[2] < 2:
                continue
            mut = PB.ref_pbest(*TPK.betas(*case), **{fault: True})
            ratios[case] = _ratio(PB.pbest_errs(mut, TPK.pbest_ref(*case)),
                                  TPK.E_PBEST[case])
        hit = self._caught(ratios, f"pbest_kernel {fault}")
        if fault == "drop_last":
            # a last model without mass whose cdf is 1 wherever the
            # others integrate cannot show; every family has a case
            # where it does
            assert {c[0] for c in hit} == set(TPK.FAMS)

    @pytest.mark.parametrize("fault", ["drop_last", "lane0_trapezoid",
                                       "window_shift", "couple_local"])
    def test_row_kernel(self, fault):
        ratios = {}
        for case in TPK.ROW_CASES:
            if case[1] < 4:             # one model per window at most
                continue
            mut = PB.ref_pbest_row(*TPK.betas(case[0], 1, case[1]),
                                   **{fault: True})
            ratios[case] = _ratio(PB.pbest_errs(mut, TPK.row_ref(*case)),
                                  TPK.E_ROW[case])
        self._caught(ratios, f"pbest_row_kernel {fault}")

    # -- phase kernels (slog2, unnormalised masses) ---------------------

    @pytest.mark.parametrize("fault", ["drop_last", "lane0_trapezoid"])
    def test_phase1(self, fault):
        ratios = {}
        for case in TPK.PHASE_CASES:
            ref = TPK.phase_ref(*case)
            mut = PB.ref_slog2(*TPK.phase_betas(*case)[:2],
                               **{fault: True})
            ratios[case] = _ratio(PB.slog2_errs(mut, ref.slog2, ref.bulk),
                                  TPK.E_PHASE[case][:2])
        hit = self._caught(ratios, f"pbest_phase1 {fault}")
        if fault == "drop_last":
            assert len(hit) == len(ratios)

    @pytest.mark.parametrize("fault", ["drop_last", "lane0_trapezoid",
                                       "couple_local"])
    def test_phase2(self, fault):
        ratios = {}
        for case in TPK.PHASE_CASES:
            if fault == "couple_local" and case[0] in PB.END_RANGES:
                continue                # no second shard there
            ref = TPK.phase_ref(*case)
            m, t = PB.ref_masses(*TPK.phase_betas(*case)[:2],
                                 ref.slog2_in, **{fault: True})
            ratios[case] = _ratio(PB.mass_errs(m, t, ref.masses, ref.total),
                                  TPK.E_PHASE[case][2:])
        hit = self._caught(ratios, f"pbest_phase2 {fault}")
        if fault == "couple_local":
            assert len(hit) == len(ratios)
        if fault == "drop_last":        # see test_generic_kernel
            assert {c[0] for c in hit} >= set(TPK.FAMS)

    @pytest.mark.parametrize("fault,fam", [("full_w0", "end0"),
                                           ("full_w255", "end255")])
    def test_phase2_end_weights(self, fault, fam):
        """A full weight at point 0 / 255. At H = 1 the normalised share
        is 1 whatever the weights: only the unnormalised outputs see
        it."""
        case = (fam, 2, 1)
        ref = TPK.phase_ref(*case)
        a, b = TPK.betas(*case)
        m, t = PB.ref_masses(a, b, ref.slog2_in, **{fault: True})
        errs = PB.mass_errs(m, t, ref.masses, ref.total)
        assert _ratio(errs[:1], TPK.E_PHASE[case][2:3]) >= self.FLOOR
        assert _ratio(errs[1:], TPK.E_PHASE[case][3:]) >= self.FLOOR
        assert float((PB.normalise(m, t) - 1).abs().max()) <= 1e-15

    # -- wide kernels ----------------------------------------------------

    @pytest.mark.parametrize("fault", ["drop_last", "window_shift",
                                       "lane0_trapezoid"])
    def test_phase1_wide(self, fault):
        ratios = {}
        for case in TPK.WIDE_CASES:
            fam, R_, H, hc = case
            if fault == "window_shift" and hc >= H:
                continue                # a single window
            ref = TPK.wide_ref(*case)
            mut = PB.ref_slog2_windows(*TPK.betas(fam, R_, H), hc,
                                       **{fault: True})
            ratios[case] = _ratio(PB.slog2_errs(mut, ref.parts, ref.bulk),
                                  TPK.E_WIDE[case][:2])
        hit = self._caught(ratios, f"pbest_phase1_wide {fault}")
        if fault != "lane0_trapezoid":
            assert len(hit) == len(ratios)

    @pytest.mark.parametrize("fault", ["drop_last", "window_shift",
                                       "couple_local"])
    def test_phase2_wide(self, fault):
        ratios = {}
        for case in TPK.WIDE_CASES:
            fam, R_, H, hc = case
            if fault != "drop_last" and hc >= H:
                continue
            ref = TPK.wide_ref(*case)
            m, t = PB.ref_masses_windows(*TPK.betas(fam, R_, H),
                                         ref.slog2_in, hc, **{fault: True})
            ratios[case] = _ratio(
                PB.mass_errs(m, t, ref.masses, ref.tot_part),
                TPK.E_WIDE[case][2:])
        hit = self._caught(ratios, f"pbest_phase2_wide {fault}")
        assert len(hit) == len(ratios)

    # -- EIG kernels -----------------------------------------------------

    HYP_FAULTS = ["vflip", "w_both", "w_neither", "next_row_class"]

    @pytest.mark.parametrize("fault", HYP_FAULTS)
    def test_eig_phase_kernels(self, fault):
        r1, r2 = {}, {}
        for case in TPK.EIG_CASES:
            i, w = TPK.eig_inputs(case)
            ref = TPK.eig_ref(case).phase
            a, b = PB.ref_hyp_betas(i.alpha_cc, i.beta_cc, i.cls, w,
                                    **{fault: True})
            r1[case] = _ratio(
                PB.slog2_errs(PB.ref_slog2(a, b), ref.slog2, ref.bulk),
                TPK.E_EIG[case][:2])
            m, t = PB.ref_masses(a, b, ref.slog2_in)
            r2[case] = _ratio(PB.mass_errs(m, t, ref.masses, ref.total),
                              TPK.E_EIG[case][2:4])
        assert len(self._caught(r1, f"eig_phase1 {fault}")) == len(r1)
        assert len(self._caught(r2, f"eig_phase2 {fault}")) == len(r2)

    def test_eig_phase2_coupled_against_its_own_partial(self):
        ratios = {}
        for case in TPK.EIG_CASES:
            ref = TPK.eig_ref(case)
            m, t = PB.ref_masses(ref.a, ref.b, ref.phase.slog2_in,
                                 couple_local=True)
            ratios[case] = _ratio(
                PB.mass_errs(m, t, ref.phase.masses, ref.phase.total),
                TPK.E_EIG[case][2:4])
        assert len(self._caught(ratios, "eig_phase2 couple_local")) \
            == len(ratios)

    @pytest.mark.parametrize("fault", HYP_FAULTS)
    def test_eig_chunk(self, fault):
        """h_after of eig_hyp_kernel. At H = 1 the only model's share is
        1 under every fault, so h_after cannot move; the phase kernels'
        outputs above see those."""
        ratios = {}
        for case in TPK.EIG_CASES:
            if case[0] == 1:
                continue
            i, w = TPK.eig_inputs(case)
            mut = PB.ref_h_after(i.alpha_cc, i.beta_cc, i.cls, w, i.pi_hat,
                                 i.pbest_before, i.mixture0,
                                 **{fault: True})
            err = float((mut - TPK.eig_ref(case).h_after).abs().max())
            ratios[case] = err / TPK.tol(TPK.E_EIG[case][4])
        assert len(self._caught(ratios, f"eig_chunk {fault}")) \
            == len(ratios)
