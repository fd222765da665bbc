"""CPU checks of the table engine's fp64 stage references
(tests/table_ref.py) and of the tolerances tests/test_table_kernels.py
derives from them: the references are the project's contract, every
recorded spread is re-measured, the designed cases take the branches
they claim, and each tolerance keeps a floor against the fault it
exists for."""
from __future__ import annotations

import math

import pytest
import torch

from coda_amd.ops import reference as R
from coda_amd.ops import table as tops
from tests import table_ref as TR
from tests import test_table_kernels as TTK

BAND = TTK.HOST_BAND


def _in_band(measured: float, recorded: float, floor: float = 0.0):
    """measured within HOST_BAND of the recorded figure; a figure below
    `floor` (the format's resolution) only has to stay below it."""
    assert measured <= max(recorded, floor) * BAND, (measured, recorded)
    if recorded > floor:
        assert measured >= recorded / BAND, (measured, recorded)


class TestReferencesAreTheContract:
    def test_chain_matches_cpu_table_path(self):
        """ref_es_build -> fp64 GEMM -> ref_assemble is the CPU
        composition pbest_hyp_table / eig_chunk_table."""
        H, C, B = 10, 4, 12
        ai = TR.make_assemble_inputs(H, C, B, seed=1)
        pr, tb = ai.problem, ai.problem.tables
        assert bool((TR.ref_es_build(
            tb.s_base, tb.delta, tb.dall,
            *tops._class_csr(ai.cls, C), tb.weights)[1] % 2 == 1).any()), \
            "no complement row in the chain"
        sel = TR.ref_select(ai.M, ai.cls)
        pb64 = sel / sel.sum(-1, keepdim=True)
        pb = tops.pbest_hyp_table(tb, ai.cls)
        # the fp32 path rounds slog = s_base + sum delta at its own
        # magnitude before exp2 (relative ln2 * ulp(slog) on ES), then
        # accumulates P = 256 non-negative products in fp32; the
        # normaliser repeats both
        slog = tb.s_base.abs().max() + tb.delta.abs().sum(1).max()
        ulp = 2.0 ** (math.floor(math.log2(float(slog))) - 23)
        tol = 2 * (math.log(2) * ulp + TR.P * 2.0 ** -24)
        e_pb = float(((pb.double() - pb64).abs() / pb64).max())
        print(f"pb rel {e_pb:.3g} tol {tol:.3g} (|slog| <= {float(slog):.0f})")
        assert e_pb <= tol, e_pb
        g = torch.Generator().manual_seed(11)
        pi_xi = torch.rand(B, C, generator=g)
        pi_xi /= pi_xi.sum(-1, keepdim=True)
        h64 = TR.ref_assemble(ai.M, ai.cls, ai.pi_hat, ai.pbest_before,
                              ai.mixture0)
        eig64 = float(pr.H_before) - (pi_xi.double() * h64).sum(-1)
        eig = tops.eig_chunk_table(tb, ai.cls, ai.pbest_before, ai.pi_hat,
                                   pi_xi, ai.mixture0, pr.H_before)
        # |d(-m log2 m)| <= (|log2 m| + 1.45) |dm| with m >= 1e-12:
        # 42 |dm|, |dm| <= pb * tol summed over H models, pi_xi sums to 1
        e_eig = float((eig.double() - eig64).abs().max())
        print(f"eig abs {e_eig:.3g}")
        assert e_eig <= 42 * tol + 1e-6, e_eig

    @pytest.mark.parametrize("uw", [1.0, 2.0])
    def test_curves_match_table_precompute(self, uw):
        """ref_beta_row_curves is table_precompute's curve math. In the
        bulk of a curve (cdf >= 2^-10) the fp32 path carries the
        rounding of t2 (ulp of <= 2^7) and a 256-term fp32 cumsum."""
        H, C = 9, 5
        g = torch.Generator().manual_seed(12)
        dirs = torch.rand(H, C, C, generator=g) * 3 + 1.0 \
            + torch.eye(C) * 15
        alpha_cc, beta_cc = R.dirichlet_to_beta(dirs)
        tb = tops.table_precompute(alpha_cc, beta_cc, uw)
        tol_lc = (2.0 ** -17 + TR.P * 2.0 ** -24) / math.log(2) * 2
        for c in range(C):
            eg, lc = TR.ref_beta_row_curves(alpha_cc[:, c], beta_cc[:, c],
                                            uw)
            bulk = lc >= TTK.BULK_LC
            d = lc[:, 1] - lc[:, 0]
            both = bulk[:, 0] & bulk[:, 1]
            e_d = float((tb.delta[c].double() - d).abs()[both].max())
            e_eg = TR.rel_err(tb.EG[c][bulk], eg[bulk], TTK.EG_FLOOR)
            assert e_d <= 2 * tol_lc, (c, e_d)
            assert e_eg <= 2 * tol_lc, (c, e_eg)
            # s_base sums H values of magnitude <= 100
            e_s = float((tb.s_base[c].double() - lc[:, 0].sum(0)).abs()
                        .max())
            assert e_s <= H * 100 * 2.0 ** -22, (c, e_s)

    @pytest.mark.parametrize("case", [(70, 3), (1100, 3)])
    def test_complement_form_equals_direct_sum(self, case):
        """With a CONSISTENT dall (the fp32 sum of delta) the complement
        form is the direct sum, up to dall's own fp32 rounding."""
        i = TTK.es_inputs(case)
        H = case[0]
        dall = i.delta.sum(1)
        args = (i.s_base, i.delta, dall, i.hvals, i.offsets, i.w)
        comp, branch = TR.ref_es_build(*args)
        direct, _ = TR.ref_es_build(*args, no_complement=True)
        is_comp = (branch % 2 == 1).t()                      # (C, B)
        assert bool(is_comp.any())
        assert torch.equal(comp[~is_comp], direct[~is_comp])
        # |fp32 sum - exact| <= H 2^-24 sum |delta| (any order)
        bound = H * 2.0 ** -24 * float(i.delta.double().abs().sum(1).max())
        rel = float(((comp - direct).abs() / direct)[is_comp].max())
        assert 0 < rel <= 1.01 * math.log(2) * bound, (rel, bound)


class TestRecordedSpreads:
    """Every figure recorded in test_table_kernels.py, re-measured."""

    @pytest.mark.parametrize("case", list(TTK.ES_CASES))
    def test_es_build(self, case):
        _in_band(TTK.measure_e_es(case), TTK.E_ES[case])
        ref, _ = TTK.es_ref(case)
        assert float(ref.min()) >= TR.PR.F32_MIN_NORMAL
        assert float(ref.max()) < 3e38

    @pytest.mark.parametrize("Hg", list(TTK.GATHERED_CASES))
    def test_es_build_gathered(self, Hg):
        _in_band(TTK.measure_e_gathered(Hg), TTK.E_GATHERED[Hg])

    @pytest.mark.parametrize("dt", list(TTK.M_DTYPES))
    @pytest.mark.parametrize("case", TTK.ASSEMBLE_CASES + ["clamp"])
    def test_assemble(self, case, dt):
        rec = TTK.E_CLAMP[dt] if case == "clamp" \
            else TTK.E_ASSEMBLE[(case, dt)]
        _in_band(TTK.measure_e_assemble(case, dt), rec, TTK.E_ULP)
        assert TTK.assemble_tol(case, dt) >= TTK.MARGIN * TTK.E_ULP

    def test_clamp_case_hits_both_clamps(self):
        ai, M = TTK.assemble_inputs("clamp", "fp32")
        tot = TR.ref_totals(M, ai.cls)
        assert float(tot[1, 0]) == 0.0 and int((tot == 0).sum()) == 1
        sel = TR.ref_select(M, ai.cls)
        mm = ai.mixture0.double().view(1, 1, -1) + ai.pi_hat.double().view(
            1, -1, 1) * (sel / tot.clamp_min(1e-30).unsqueeze(-1)
                         - ai.pbest_before.double().unsqueeze(0))
        assert bool((mm < 1e-12).any()) and bool((mm > 1e-3).any())

    @pytest.mark.parametrize("name,H,uw", TTK.BETA_CASES)
    def test_beta_row_tables(self, name, H, uw):
        for e, rec in zip(TTK.measure_e_beta(name, H, uw),
                          TTK.E_BETA[(name, H, uw)]):
            _in_band(e, rec)
        eg64, _ = TTK.beta_ref(name, H, uw)
        assert torch.isfinite(eg64).all() and float(eg64.max()) < 3e38

    @pytest.mark.parametrize("H,C,y", TTK.COMMIT_CASES)
    def test_commit(self, H, C, y):
        for e, rec in zip(TTK.measure_e_commit(H, C, y),
                          TTK.E_COMMIT[(H, C, y)]):
            _in_band(e, rec)
        d = TTK.commit_inputs(H, C).dirichlets
        a = d[:, y, y]
        assert float(a.min()) >= 1 and float((d[:, y].sum(-1) - a).min()) >= 2


class TestBranchCensus:
    """The designed es_build cases take the branches the GPU module
    expects (recounted here from the bucket sizes alone)."""

    @pytest.mark.parametrize("case", list(TTK.ES_CASES))
    def test_census(self, case):
        H, C = case
        i = TTK.es_inputs(case)
        n = (i.offsets[:, 1:] - i.offsets[:, :-1]).long()
        assert torch.equal(n[:, 0], torch.tensor(TTK.ES_CASES[case]))
        assert bool((n.sum(1) == H).all())
        counts = [0, 0, 0, 0]
        for k in n.flatten().tolist():
            counts[TR.es_branch(k, H)[2]] += 1
        assert tuple(counts) == TTK.ES_CENSUS[case]
        assert TTK.census(TTK.es_ref(case)[1]) == TTK.ES_CENSUS[case]
        # every hvals row is a permutation sorted by class
        assert torch.equal(i.hvals.long().sort(1).values,
                           torch.arange(H).expand_as(i.hvals))

    def test_regimes(self):
        c = TTK.ES_CENSUS
        assert c[(1100, 3)] == (30, 4, 11, 3)
        assert c[(1024, 2)][2:] == (0, 0) and c[(70, 3)][2:] == (0, 0)
        assert c[(1026, 2)][2] == 2 and c[(1026, 2)][3] == 0
        # the short kernel packs 16 rows per block: a ragged last block
        # without (H <= 1024) and with (H > 1024) the long launch
        rows = {k: len(v) * k[1] for k, v in TTK.ES_CASES.items()}
        assert rows[(70, 3)] % 16 and rows[(1026, 2)] % 16
        # threshold rows: n = H // 2 direct, H // 2 + 1 complement
        for (H, C), sizes in TTK.ES_CASES.items():
            assert H // 2 in sizes and H // 2 + 1 in sizes
            assert not TR.es_branch(H // 2, H)[0]
            assert TR.es_branch(H // 2 + 1, H)[0]

    @pytest.mark.parametrize("Hg", list(TTK.GATHERED_CASES))
    def test_gathered_buckets(self, Hg):
        i = TTK.gathered_inputs(Hg)
        n = (i.offsets[:, 1:] - i.offsets[:, :-1]).flatten().tolist()
        assert set(TTK.GATHERED_CASES[Hg]) <= set(n)
        assert (i.hvals.shape[0] * TTK.GATHERED_C) % 4 != 0
        if Hg >= 70:        # unroll body with every tail length
            assert {k % 4 for k in n if k >= 4} == {0, 1, 2, 3}


class TestToleranceFloors:
    """Each fault is applied to the fp64 reference and must move it by
    at least FLOOR tolerances of the case it would hit. Loosening a
    tolerance until these fail is loosening it until the GPU test means
    nothing; inputs, not tolerances, are what may change here."""

    FLOOR = 10.0

    @pytest.mark.parametrize("case", list(TTK.ES_CASES))
    def test_one_model_dropped_from_a_bucket(self, case):
        i = TTK.es_inputs(case)
        ref, _ = TTK.es_ref(case)
        mut, _ = TR.ref_es_build(i.s_base, i.delta, i.dall, i.hvals,
                                 i.offsets, i.w, drop_last=True)
        n = (i.offsets[:, 1:] - i.offsets[:, :-1]).long()
        H = case[0]
        summed = torch.tensor([[TR.es_branch(int(k), H)[1] for k in row]
                               for row in n]).t() > 0           # (C, B)
        assert bool(summed.any())
        moved = ((mut - ref).abs() / ref)[summed]
        assert float(moved.min()) >= 1 - 2.0 ** -TR.DELTA_FLOOR - 1e-12
        assert float(moved.min()) >= self.FLOOR * TTK.MARGIN * TTK.E_ES[case]

    @pytest.mark.parametrize("Hg", list(TTK.GATHERED_CASES))
    def test_one_model_dropped_gathered(self, Hg):
        i = TTK.gathered_inputs(Hg)
        mut = TR.ref_es_build_gathered(i.s_base, i.sel_all, i.hvals,
                                       i.offsets, i.w, drop_last=True)
        n = (i.offsets[:, 1:] - i.offsets[:, :-1]).t() > 0
        moved = ((mut - TTK.gathered_ref(Hg)).abs()
                 / TTK.gathered_ref(Hg))[n]
        assert float(moved.min()) >= \
            self.FLOOR * TTK.MARGIN * TTK.E_GATHERED[Hg]

    @pytest.mark.parametrize("case", list(TTK.ES_CASES))
    def test_complement_taken_at_half(self, case):
        """`n >= H / 2` for `n > H / 2`: the row with exactly H // 2
        models goes through dall, which the inputs skew by DALL_SKEW."""
        i = TTK.es_inputs(case)
        ref, branch = TTK.es_ref(case)
        mut, mbranch = TR.ref_es_build(i.s_base, i.delta, i.dall, i.hvals,
                                       i.offsets, i.w, comp_ge=True)
        hit = ((branch % 2) != (mbranch % 2)).t()               # (C, B)
        assert bool(hit.any())
        moved = ((mut - ref).abs() / ref)[hit]
        assert float(moved.min()) >= 0.9 * (2.0 ** TR.DALL_SKEW - 1)
        assert float(moved.min()) >= self.FLOOR * TTK.MARGIN * TTK.E_ES[case]

    @pytest.mark.parametrize("q", range(4))
    @pytest.mark.parametrize("case", [(1026, 2), (1100, 3)])
    def test_one_quarter_of_a_long_row_dropped(self, case, q):
        i = TTK.es_inputs(case)
        ref, branch = TTK.es_ref(case)
        mut, _ = TR.ref_es_build(i.s_base, i.delta, i.dall, i.hvals,
                                 i.offsets, i.w, drop_quarter=q)
        is_long = (branch >= TR.DIRECT_LONG).t()
        assert torch.equal(mut[~is_long], ref[~is_long])
        moved = ((mut - ref).abs() / ref)[is_long]              # (rows, P)
        floor = self.FLOOR * TTK.MARGIN * TTK.E_ES[case]
        assert float(moved.median(-1).values.min()) >= floor

    @pytest.mark.parametrize("dt", list(TTK.M_DTYPES))
    @pytest.mark.parametrize("case", TTK.ASSEMBLE_CASES)
    def test_one_vselect_bit_flipped(self, case, dt):
        """One seeded wrong v bit in every row. At H = 1 the share is
        tot / tot whatever is selected, so there the fault shows in
        eig_totals (its own bound) alone."""
        H, C, B = case
        ai, M = TTK.assemble_inputs(case, dt)
        g = torch.Generator().manual_seed(21)
        vflip = torch.randint(0, H, (B, C), generator=g)
        if H == 1:
            t0 = TR.ref_totals(M, ai.cls)
            t1 = TR.ref_totals(M, ai.cls, vflip=vflip)
            assert float(((t1 - t0).abs() / t0).min()) \
                >= self.FLOOR * H * 2.0 ** -24
            return
        mut = TR.ref_assemble(M, ai.cls, ai.pi_hat, ai.pbest_before,
                              ai.mixture0, vflip=vflip)
        moved = (mut - TTK.assemble_ref(case, dt)).abs()
        tol = TTK.assemble_tol(case, dt)
        share = float((moved > tol).double().mean())
        print(case, dt, f"max {float(moved.max()) / tol:.1f} tol, "
              f"share over tol {share:.2f}")
        # a kernel fault hits every row; the test sees the worst one
        assert float(moved.max()) >= self.FLOOR * tol
        assert share >= 0.5

    @pytest.mark.parametrize("dt", list(TTK.M_DTYPES))
    @pytest.mark.parametrize("H", TTK.TWO_SHARD_H)
    def test_shard_totals_not_added(self, H, dt):
        case = (H, 3, 7)
        ai, M = TTK.assemble_inputs(case, dt)
        C, B = M.shape[:2]
        for r in range(2):
            Mr = M.view(C, B, H, 2)[:, :, r::2].reshape(C, B, -1)
            part = TR.ref_totals(Mr, ai.cls[:, r::2])
            mut = TR.ref_entropy(M, ai.cls, part, ai.pi_hat,
                                 ai.pbest_before, ai.mixture0)
            moved = (mut - TTK.assemble_ref(case, dt)).abs()
            assert float(moved.min()) >= \
                self.FLOOR * TTK.assemble_tol(case, dt)

    @pytest.mark.parametrize("name,H,uw", TTK.BETA_CASES)
    def test_curve_variants_swapped(self, name, H, uw):
        """v0 / v1 exchanged: seen by the bulk lc check of every case."""
        a, b = TR.make_beta_cols(name, H, seed=TTK.SEED)
        errs = TTK.beta_errs(*TR.ref_beta_row_curves(a, b, uw, swap_v=True),
                             name, H, uw)
        rec = TTK.E_BETA[(name, H, uw)]
        assert errs[2] >= self.FLOOR * TTK.MARGIN * rec[2], (errs, rec)

    @pytest.mark.parametrize("name,H,uw", [
        c for c in TTK.BETA_CASES if c[0] in ("singular0", "wide")])
    def test_first_trapezoid_counted_at_lane_0(self, name, H, uw):
        """Lane 0 without its guard adds 0.5 (pdf[0] + pdf[3]) dx to
        every cdf. Only a pdf that is not negligible on the first four
        grid points (x <= 0.012) can show it: the singular range always
        does, the wide range where it drew a small alpha; the moderate
        and concentrated ranges cannot."""
        a, b = TR.make_beta_cols(name, H, seed=TTK.SEED)
        errs = TTK.beta_errs(
            *TR.ref_beta_row_curves(a, b, uw, lane0_trapezoid=True),
            name, H, uw)
        rec = TTK.E_BETA[(name, H, uw)]
        caught = [e >= self.FLOOR * TTK.MARGIN * r
                  for e, r in zip(errs, rec)]
        if name == "singular0":
            assert all(caught), (errs, rec)
        elif float(a.min()) < 3:
            assert caught[2], (errs, rec)

    @pytest.mark.parametrize("H,C,y", TTK.COMMIT_CASES)
    def test_commit_written_to_a_neighbour_row(self, H, C, y):
        """A commit to row y +- 1 changes a row that must stay bitwise
        equal, and leaves the filler in row y: that filler is at least
        FLOOR tolerances from the committed row in all four fp32
        tables, and the mirrors differ too."""
        ci = TTK.commit_inputs(H, C)
        ref = TTK.commit_ref(H, C, y)
        t = ci.tables
        errs = TTK.commit_errs(t["EG"][y], t["delta"][y], t["s_base"][y],
                               t["dall"][y], ref)
        for e, rec in zip(errs, TTK.E_COMMIT[(H, C, y)]):
            assert e >= self.FLOOR * TTK.MARGIN * rec, (errs,)
        assert not bool(TR.PR.a_operand_ok(t["egw"][y], ref.egw).all())
        for other in ((y - 1) % C, (y + 1) % C):
            o = TTK.commit_ref(H, C, other)
            assert not torch.equal(o.eg16, ref.eg16)
            assert not torch.equal(o.delta16, ref.delta16)
