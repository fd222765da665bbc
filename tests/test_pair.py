"""v3 pair-factored EIG engine (coda_amd/ops/pair.py), CPU.

The pair engine must reproduce the dense table engine (ops/table.py) and
the fused eager formulation (ops/reference.py) exactly up to fp32
reduction order: same EIG values, same selections, same trajectories.
Reference semantics: coda/coda.py:235-281 with --prefilter-n 0.
"""
from __future__ import annotations

import random

import pytest
import torch

from coda_amd import CODA, Oracle
from coda_amd.datasets import Dataset, make_synthetic_task
from coda_amd.options import LOSS_FNS
from coda_amd.ops import pair as pops
from coda_amd.ops import table as tops
from coda_amd.ops import reference as R
from tests import pair_ref as PR
from tests import test_pair_kernels as TPK


def _random_problem(H=10, N=120, C=7, seed=0):
    g = torch.Generator().manual_seed(seed)
    preds = torch.softmax(torch.randn(H, N, C, generator=g) * 2, dim=-1)
    cls = preds.argmax(-1)                     # (H, N)
    dirichlets = torch.rand(H, C, C, generator=g) * 3 + 0.5
    pi_hat = torch.rand(C, generator=g)
    pi_hat /= pi_hat.sum()
    adjusted = torch.rand(N, C, generator=g) + 0.1
    row_sums = adjusted.sum(-1)
    return preds, cls, dirichlets, pi_hat, adjusted, row_sums


def _check_covers_every_hit(cls_rows, ids, H, C):
    """Every (candidate, class) hit maps through the CSR to exactly one
    representative pair whose (class, hit-set) matches the brute-force
    set (pairs with identical sets are deduplicated)."""
    B = ids.numel()
    ps = pops.build_pairs(cls_rows, ids, C)

    def pair_set(k):
        hs = set(ps.seg_h[int(ps.seg_off[k]):
                          int(ps.seg_off[k + 1])].tolist())
        if int(ps.pair_neg[k]):
            hs = set(range(H)) - hs
        return hs

    seen = {}
    for b in range(B):
        for s in range(int(ps.cand_off[b]), int(ps.cand_off[b + 1])):
            k = int(ps.cand_pairs[s])
            c = int(ps.pair_c[k])
            assert (b, c) not in seen, "duplicate CSR entry"
            seen[(b, c)] = pair_set(k)
    for b in range(B):
        for c in range(C):
            expect = {h for h in range(H) if int(cls_rows[b, h]) == c}
            if expect:
                assert seen[(b, c)] == expect, (b, c)
            else:
                assert (b, c) not in seen
    # dedupe really collapses: fewer evaluated pairs than hits
    n_hits = len(seen)
    assert ps.n_real <= n_hits
    # base/pad pairs have empty segments and no complement flag
    for k in range(ps.K):
        if int(ps.pair_b[k]) < 0:
            assert int(ps.seg_off[k + 1]) == int(ps.seg_off[k])
            assert int(ps.pair_neg[k]) == 0
    return ps


class TestPairStructure:
    def test_covers_every_hit_exactly_once(self):
        """Every (candidate, class) hit maps through the CSR to exactly
        one representative pair whose (class, hit-set) matches the
        brute-force set (pairs with identical sets are deduplicated)."""
        _, cls, *_ = _random_problem(H=9, N=50, C=6, seed=1)
        ids = torch.arange(37)
        cls_rows = cls[:, ids].t().contiguous()
        _check_covers_every_hit(cls_rows, ids, 9, 6)

    def test_covers_every_hit_exactly_once_consensus(self):
        """The same on a consensus-heavy pool, where majority pairs
        store the COMPLEMENT of their hit set (pair_neg)."""
        cls_rows = PR.consensus_classes(9, 50, 6, 0.7, seed=1)[:37]
        ps = _check_covers_every_hit(cls_rows.contiguous(),
                                     torch.arange(37), 9, 6)
        assert bool(ps.pair_neg.any())

    @pytest.mark.parametrize("H,N,C,p", [(10, 3000, 2, 0.5),
                                         (12, 4000, 3, 0.6),
                                         (9, 700, 6, 0.7)])
    def test_tile_groups_partition_the_tiles(self, H, N, C, p):
        """grp_off (tile 128): groups of at most 4 same-class tiles that
        partition the tile range; absent at tile 16."""
        cls_rows = PR.consensus_classes(H, N, C, p, seed=0)
        ids = torch.arange(N)
        ps = pops.build_pairs(cls_rows, ids, C, tile=128)
        g = ps.grp_off
        assert g is not None and g.dtype == torch.int32
        assert ps.K % 128 == 0
        T = ps.K // 128
        assert int(g[0]) == 0 and int(g[-1]) == T
        sizes = g[1:] - g[:-1]
        assert bool((sizes > 0).all()), "not strictly increasing"
        assert int(sizes.max()) <= 4
        # offsets count whole tiles: a boundary is always k = 128 * t
        tile_cls = ps.pair_c.view(T, 128)
        assert bool((tile_cls == tile_cls[:, :1]).all())
        for a, b in zip(g[:-1].tolist(), g[1:].tolist()):
            assert len(set(tile_cls[a:b, 0].tolist())) == 1, (a, b)
        assert pops.build_pairs(cls_rows, ids, C, tile=16).grp_off is None

    def test_tiles_are_class_uniform_and_base_marked(self):
        _, cls, *_ = _random_problem(H=12, N=64, C=5, seed=2)
        ids = torch.arange(64)
        ps = pops.build_pairs(cls[:, ids].t().contiguous(), ids, 5)
        assert ps.K % ps.tile == 0
        pc = ps.pair_c.view(-1, ps.tile)
        assert (pc == pc[:, :1]).all(), "tile straddles classes"
        # base pair of every class exists, has empty segment, b = -1
        for c in range(5):
            k = int(ps.base_pos[c])
            assert int(ps.pair_c[k]) == c
            assert int(ps.pair_b[k]) == -1
            assert int(ps.seg_off[k + 1]) == int(ps.seg_off[k])


class TestPairEig:
    @pytest.mark.parametrize("H,N,C", [(10, 120, 7), (3, 60, 2),
                                       (16, 200, 126)])
    def test_matches_table_engine(self, H, N, C):
        (preds, cls, dirichlets, pi_hat, adjusted,
         row_sums) = _random_problem(H, N, C, seed=H + C)
        alpha_cc, beta_cc = R.dirichlet_to_beta(dirichlets)
        tables = tops.table_precompute(alpha_cc, beta_cc)
        pbest_before = R.pbest_from_beta(alpha_cc.t().contiguous(),
                                         beta_cc.t().contiguous())
        mixture0, H_before = R.mixture_entropy(pbest_before, pi_hat)

        ids = torch.arange(N)
        cls_rows = cls[:, ids].t().contiguous()
        ps = pops.build_pairs(cls_rows, ids, C)
        eig_n = pops.eig_pairs(tables, ps, cls_rows, pbest_before,
                               pi_hat, mixture0, H_before, adjusted,
                               row_sums)

        pi_xi = adjusted / row_sums.clamp_min(1e-12).unsqueeze(-1)
        eig_dense = tops.eig_chunk_table(tables, cls_rows, pbest_before,
                                         pi_hat, pi_xi, mixture0,
                                         H_before)
        torch.testing.assert_close(eig_n, eig_dense, rtol=2e-4,
                                   atol=1e-6)

    def test_trajectory_equals_fused_and_table(self):
        preds, labels = make_synthetic_task(H=12, N=400, C=9, seed=3)
        ds = Dataset.from_tensors(preds, labels, "cpu")
        oracle = Oracle(ds, LOSS_FNS["acc"])

        def run(impl, prefilter):
            random.seed(0)
            torch.manual_seed(0)
            sel = CODA(ds, eig_impl=impl, prefilter_n=prefilter,
                       chunk_size=64)
            traj = []
            for _ in range(6):
                i, q = sel.get_next_item_to_label()
                sel.add_label(i, oracle(int(i)), q)
                traj.append((int(i),
                             int(sel.get_best_model_prediction())))
            return traj, sel.get_pbest()

        for prefilter in (0, 32):
            t_f, p_f = run("fused", prefilter)
            t_t, _ = run("table", prefilter)
            t_p, p_p = run("pair", prefilter)
            assert t_f == t_t == t_p
            torch.testing.assert_close(p_f, p_p, rtol=1e-4, atol=1e-6)

    def test_static_structure_reused_and_masked(self):
        preds, labels = make_synthetic_task(H=8, N=150, C=5, seed=4)
        ds = Dataset.from_tensors(preds, labels, "cpu")
        oracle = Oracle(ds, LOSS_FNS["acc"])
        random.seed(0)
        torch.manual_seed(0)
        sel = CODA(ds, eig_impl="pair")
        i0, q0 = sel.get_next_item_to_label()
        assert sel._pair_acq is not None
        ps0 = sel._pair_acq.ps
        sel.add_label(i0, oracle(int(i0)), q0)
        i1, _ = sel.get_next_item_to_label()
        assert sel._pair_acq.ps is ps0, "structure rebuilt"
        assert int(i1) != int(i0), "labeled point re-selected"
        row = sel._pair_acq.row_of[int(i0)]
        assert not bool(sel._pair_acq.active[row])

    def test_skip_removes_candidate(self):
        preds, labels = make_synthetic_task(H=8, N=150, C=5, seed=5)
        ds = Dataset.from_tensors(preds, labels, "cpu")
        random.seed(0)
        torch.manual_seed(0)
        sel = CODA(ds, eig_impl="pair")
        i0, _ = sel.get_next_item_to_label()
        sel.skip(i0)
        i1, _ = sel.get_next_item_to_label()
        assert int(i1) != int(i0)


class TestDedupeProperties:
    @pytest.mark.parametrize("H,N,C,seed", [(9, 200, 6, 0), (16, 300, 3, 1),
                                            (5, 100, 50, 2), (32, 150, 8, 3)])
    def test_dedupe_equals_no_dedupe(self, H, N, C, seed):
        """EIG through the deduplicated structure == through the
        1:1 structure, for random shapes (guards the set-hash grouping
        and the CSR remap)."""
        (preds, cls, dirichlets, pi_hat, adjusted,
         row_sums) = _random_problem(H, N, C, seed=seed)
        alpha_cc, beta_cc = R.dirichlet_to_beta(dirichlets)
        tables = tops.table_precompute(alpha_cc, beta_cc)
        pbest_before = R.pbest_from_beta(alpha_cc.t().contiguous(),
                                         beta_cc.t().contiguous())
        mixture0, H_before = R.mixture_entropy(pbest_before, pi_hat)
        ids = torch.arange(N)
        cls_rows = cls[:, ids].t().contiguous()
        out = {}
        for dd in (True, False):
            ps = pops.build_pairs(cls_rows, ids, C, dedupe=dd)
            out[dd] = pops.eig_pairs(tables, ps, cls_rows, pbest_before,
                                     pi_hat, mixture0, H_before,
                                     adjusted, row_sums)
        assert out[True].shape == out[False].shape
        torch.testing.assert_close(out[True], out[False], rtol=1e-5,
                                   atol=1e-7)

    def test_strided_candidate_slice_matches_full(self):
        """Slice structures (the sharded per-rank view, incl. strided
        cand_ids) reproduce the full-pool EIG exactly on CPU."""
        (preds, cls, dirichlets, pi_hat, adjusted,
         row_sums) = _random_problem(11, 180, 7, seed=9)
        alpha_cc, beta_cc = R.dirichlet_to_beta(dirichlets)
        tables = tops.table_precompute(alpha_cc, beta_cc)
        pbest_before = R.pbest_from_beta(alpha_cc.t().contiguous(),
                                         beta_cc.t().contiguous())
        mixture0, H_before = R.mixture_entropy(pbest_before, pi_hat)
        ids = torch.arange(180)
        cls_all = cls[:, ids].t().contiguous()
        ps = pops.build_pairs(cls_all, ids, 7)
        q_full = pops.eig_pairs(tables, ps, cls_all, pbest_before,
                                pi_hat, mixture0, H_before, adjusted,
                                row_sums)
        for r in range(3):
            mine = ids[r::3]             # non-contiguous slice
            cls_r = cls[:, mine].t().contiguous()
            ps_r = pops.build_pairs(cls_r, mine, 7)
            assert ps_r.cand_ids.is_contiguous()
            q_r = pops.eig_pairs(tables, ps_r, cls_r, pbest_before,
                                 pi_hat, mixture0, H_before, adjusted,
                                 row_sums)
            torch.testing.assert_close(q_r, q_full[r::3], rtol=1e-6,
                                       atol=1e-8)


class TestStageReferences:
    """The fp64 stage references of tests/pair_ref.py, and the
    tolerances tests/test_pair_kernels.py derives from them (CPU)."""

    def test_consensus_generator(self):
        H, N, C = 12, 400, 5
        ind = PR.consensus_classes(H, N, C, 0.0, seed=3)
        g = torch.Generator().manual_seed(3)
        torch.randint(0, C, (N, 1), generator=g)
        torch.rand(N, H, generator=g)
        assert torch.equal(ind, torch.randint(0, C, (N, H), generator=g))
        con = PR.consensus_classes(H, N, C, 0.6, seed=3)
        assert con.shape == (N, H) and 0 <= int(con.min()) \
            and int(con.max()) < C
        top = torch.stack([(con == c).sum(1) for c in range(C)]).max(0)
        assert float((top.values > H // 2).float().mean()) > 0.5
        ps = pops.build_pairs(con, torch.arange(N), C)
        assert bool(ps.pair_neg.any())

    @pytest.mark.parametrize("H,N,C,p", TPK.DSUM_CASES)
    def test_fp64_chain_matches_eager_unquantised(self, H, N, C, p):
        """With the quantisation taken out (fp32 delta, unrounded A and
        EG) the fp64 stage chain is the eager pair math."""
        pr = PR.make_problem(H, N, C, p, seed=TPK.SEED)
        ps, tb = pr.ps, pr.tables
        assert bool(ps.pair_neg.any())
        A = torch.exp2(PR.ref_dsum(tb.delta, tb.dall, ps))
        egw = (tb.EG.reshape(C, 2 * H, -1).double()
               * (torch.exp2(tb.s_base.double())
                  * tb.weights.double()).unsqueeze(1))
        vbits = PR.vbits_from_cls(pr.cls_rows, ps)
        assert torch.equal(vbits, PR.vbits_from_vmask(ps.vmask, H))
        h64 = PR.ref_gemm_entropy(A, egw, vbits, ps.pair_c, pr.pi_hat,
                                  pr.pbest_before, pr.mixture0)
        h_eager = pops.pair_h_after(tb, ps, pr.cls_rows, pr.pbest_before,
                                    pr.pi_hat, pr.mixture0)
        q64 = PR.ref_finalize(h64, ps, pr.adjusted, pr.row_sums,
                              pr.H_before)
        q_eager = pops.eig_from_pairs(h_eager, ps, pr.adjusted,
                                      pr.row_sums, pr.H_before)[ps.cand_ids]
        e_h = float((h_eager.double() - h64).abs().max())
        e_q = float((q_eager.double() - q64).abs().max())
        print(f"{(H, N, C, p)}: h_after {e_h:.3g} eig {e_q:.3g}")
        # measured: h_after <= 9.8e-7, EIG <= 1.3e-6 over the four shapes
        assert e_h <= 1e-5, e_h
        assert e_q <= 1e-5, e_q

    @pytest.mark.parametrize("case", list(TPK.E32))
    def test_recorded_e32_bounds_the_measurement(self, case):
        e32 = TPK.measure_e32(case)
        print(case, e32)
        rec = TPK.E32[case]
        assert rec / TPK.HOST_BAND <= e32 <= rec * TPK.HOST_BAND, e32
        _, tot = TPK.stage2_ref(*case)
        assert float(tot.min()) > 0.5

    @pytest.mark.parametrize("case", TPK.WIDE_VMASK + TPK.WIDE_CLS)
    def test_sampled_flips_stay_within_the_allowance(self, case):
        """The rounded reference with M accumulated in fp32 differs
        from the fp64 one only where flip_allowance says it may, and by
        no more; rounding M itself moves h_after far more."""
        flips = TPK.measure_flips(case)
        allow = TPK.flip_allowance(case)
        assert bool((flips <= allow).all())
        assert float(allow.max()) < 2e-3
        rounded, _ = TPK.stage2_ref(*case, round_m=True)
        plain, _ = TPK.stage2_ref(*case)
        assert float((rounded - plain).abs().max()) > 3e-4

    @pytest.mark.parametrize("name", list(TPK.FINALIZE))
    def test_recorded_e_fin_bounds_the_measurement(self, name):
        e_fin = TPK.measure_e_fin(name)
        print(name, e_fin)
        rec = TPK.FINALIZE[name][1]
        assert rec / TPK.HOST_BAND <= e_fin <= rec * TPK.HOST_BAND, e_fin


def _bit_flip_detected(case, round_m):
    """Flip one seeded v-select bit in every real pair of the fp64
    reference; (K,) bool exceeds-the-tolerance and the real-pair mask."""
    pr, a16, vbits, args = TPK.stage2_inputs(*case)
    real = (pr.ps.pair_b >= 0).nonzero().squeeze(1)
    g = torch.Generator().manual_seed(5)
    h = torch.randint(0, pr.H, (pr.ps.K,), generator=g)
    mut = vbits.clone()
    mut[real, h[real]] ^= True
    ref, _ = TPK.stage2_ref(*case, round_m=round_m)
    got = PR.ref_gemm_entropy(a16, args[1], mut, *args[3:], round_m)
    tol = TPK.wide_tol(case) if round_m else TPK.fused_tol(case)
    return ((got - ref).abs() > tol)[real]


class TestToleranceFloors:
    """Each stage tolerance catches the faults it exists for: the fault
    is applied to the fp64 reference and must exceed the tolerance
    (CPU). Loosening a tolerance until these fail is loosening it until
    the GPU test means nothing."""

    def test_one_wrong_vselect_bit_fused(self):
        """>= 90 % of real pairs over the fused cases; per case at
        least half (a kernel fault hits every pair, so half the pairs
        is certain detection). Measured 76 % (tile 16, H = 1024) and
        84 % (H = 128) to 100 % (H <= 12), pooled 95 %."""
        hits = {c: _bit_flip_detected(c, False)
                for c in list(TPK.FUSED128) + TPK.TILE16}
        for c, d in hits.items():
            print(c, f"{float(d.double().mean()):.3f}")
            assert float(d.double().mean()) >= 0.5, c
        pooled = torch.cat(list(hits.values())).double().mean()
        assert float(pooled) >= 0.9, float(pooled)

    @pytest.mark.parametrize("case", TPK.WIDE_VMASK + TPK.WIDE_CLS)
    def test_one_wrong_vselect_bit_wide(self, case):
        """At least half of the real pairs (measured 57 % at H = 2048
        to 94 % at H = 70)."""
        d = _bit_flip_detected(case, True)
        print(case, f"{float(d.double().mean()):.3f}")
        assert float(d.double().mean()) >= 0.5

    @staticmethod
    def _a_stage_rows_caught(ps_mut, pr, touched):
        tb = pr.tables
        ref = PR.ref_dsum_es(tb.delta16, tb.dall, pr.ps)
        got = PR.ref_dsum_es(tb.delta16, tb.dall, ps_mut)
        bad_rows = ~PR.a_operand_ok(got, ref).all(1)
        assert not bool(bad_rows[~touched].any())
        return float(bad_rows[touched].double().mean())

    @pytest.mark.parametrize("H,N,C,p", TPK.DSUM_CASES)
    def test_dropped_last_segment_entry(self, H, N, C, p):
        pr = PR.make_problem(H, N, C, p, seed=TPK.SEED)
        ps = pr.ps
        seg = (ps.seg_off[1:] - ps.seg_off[:-1]).long()
        last = (ps.seg_off[1:].long() - 1)[seg >= 2]
        keep = torch.ones(ps.seg_h.numel(), dtype=torch.bool)
        keep[last] = False
        seg2 = seg - (seg >= 2).long()
        off2 = torch.zeros_like(ps.seg_off)
        off2[1:] = seg2.cumsum(0).to(torch.int32)
        mut = ps._replace(seg_h=ps.seg_h[keep], seg_off=off2)
        share = self._a_stage_rows_caught(mut, pr, seg >= 2)
        print((H, N, C, p), share)
        assert share >= 0.9

    @pytest.mark.parametrize("H,N,C,p", TPK.DSUM_CASES)
    def test_ignored_pair_neg(self, H, N, C, p):
        pr = PR.make_problem(H, N, C, p, seed=TPK.SEED)
        mut = pr.ps._replace(pair_neg=torch.zeros_like(pr.ps.pair_neg))
        share = self._a_stage_rows_caught(mut, pr, pr.ps.pair_neg.bool())
        print((H, N, C, p), share)
        assert share >= 0.9

    @pytest.mark.parametrize("case", [(33, 1500, 5, 0.7, 128),
                                      (65, 500, 3, 0.7, 128),
                                      (136, 600, 4, 0.7, 128)])
    def test_vmask_word_zero_for_all_words(self, case):
        """h >= 32 read from word 0: at least half of the pairs whose
        v-select the fault changes (at H = 33 that is ONE model)."""
        pr, a16, vbits, args = TPK.stage2_inputs(*case)
        mut = vbits[:, torch.arange(pr.H) & 31]
        changed = (mut != vbits).any(1)
        assert bool(changed.any())
        ref, _ = TPK.stage2_ref(*case)
        got = PR.ref_gemm_entropy(a16, args[1], mut, *args[3:])
        caught = ((got - ref).abs() > TPK.fused_tol(case))[changed]
        print(case, float(caught.double().mean()))
        assert float(caught.double().mean()) >= 0.5

    @pytest.mark.parametrize("case", list(TPK.FUSED128) + TPK.TILE16)
    def test_skipped_last_column_tile(self, case):
        pr, _, _, args = TPK.stage2_inputs(*case)
        JT = (2 * pr.H + 15) // 16
        keep = torch.arange(2 * pr.H) < 16 * (JT - 1)
        ref, _ = TPK.stage2_ref(*case)
        got = PR.ref_gemm_entropy(*args, col_keep=keep)
        caught = (got - ref).abs() > TPK.fused_tol(case)
        print(case, float(caught.double().mean()))
        assert float(caught.double().mean()) >= 0.9

    def test_finalize_hits_past_the_first_lane_stride(self):
        fi, q64 = TPK.finalize_refs("hits_over_64")
        ps = fi.ps
        counts = (ps.cand_off[1:] - ps.cand_off[:-1]).long()
        pos = torch.arange(ps.cand_pairs.numel()) - torch.repeat_interleave(
            ps.cand_off[:-1].long(), counts)
        got = PR.ref_finalize(fi.h_after, ps, fi.adjusted, fi.row_sums,
                              fi.H_before, hit_keep=pos < 64)
        over = counts > 64
        assert bool(over.any())
        caught = (got - q64).abs() > TPK.fin_tol("hits_over_64")
        # a candidate with 65 hits loses ONE term, which can be small
        assert float(caught[over].double().mean()) >= 0.9
        assert not bool(caught[~over].any())

    @pytest.mark.parametrize("name", ["c3", "c7", "c261", "c1001"])
    def test_finalize_ragged_class_tail(self, name):
        fi, q64 = TPK.finalize_refs(name)
        C = fi.adjusted.shape[1]
        assert C % 4 != 0
        got = PR.ref_finalize(fi.h_after, fi.ps, fi.adjusted, fi.row_sums,
                              fi.H_before, base_cols=C - C % 4)
        assert bool(((got - q64).abs() > TPK.fin_tol(name)).all())
