"""GPU checks of the streaming pair kernels: the strided-grid finalize,
the eight-lane pad-aware cached entropy pass, the tile-per-block
one-class refresh and the mixture the merged graph hands to get_pbest().

Every kernel here kept its arithmetic when its schedule changed, so the
checks are bitwise wherever two runs compute the same quantity:

  finalize   fp64 reference on every FINALIZE case (the recorded
             tolerances of tests/test_pair_kernels.py), and a candidate's
             q independent of WHERE in the launch it sits: reversed,
             permuted and truncated candidate sets, B = 1, and a B just
             past one pass of the grid, so that some waves walk to a
             second candidate and some do not.
  entropy    with run_off / run_live == without them == the fused GEMM
             kernel, every row, on the cache cases, the skewed structure
             and a structure built so that classes' live rows end on a
             16-, a 32- (the kernel's chunk) and a 64-row boundary and
             one class has no hit pair at all (1 live row, 127 pads).
  refresh    a one-class refresh on that structure and on a class with
             more tiles than a group holds writes its run and nothing
             else, and equals a fresh build.
"""
from __future__ import annotations

import pytest
import torch

from tests import pair_ref as PR
from tests import pair_stream_ref as PSR
from tests import test_pair_kernels as TPK
from tests import test_pair_cache_gpu as TPC
from tests.pair_stream_ref import (
    BOUNDARY, BOUNDARY_LIVE, boundary_structure, long_run_structure)
from tests.test_pair_cache_gpu import (  # noqa: F401  (fixtures)
    dev, ext, pool, production)

pytestmark = pytest.mark.gpu

# candidates one pass of the finalize grid covers, from the kernel source
ONE_PASS = PSR.finalize_one_pass()


# ---------------------------------------------------------------------
# finalize
# ---------------------------------------------------------------------

def _fin_args(fi, dev):
    ps = fi.ps
    h_after = fi.h_after.to(dev)
    h_base = h_after.index_select(0, ps.base_pos.to(dev)).contiguous()
    return (h_after, h_base, ps.pair_c.to(dev), fi.adjusted.to(dev),
            fi.row_sums.to(dev))


def _fin_run(ext, dev, fi, args, order=None):
    """q for the structure's candidate rows `order` (all, in order, when
    None): cand_ids / cand_off / cand_ck rebuilt for that candidate set."""
    ps = fi.ps
    h_after, h_base, pair_c, adjusted, row_sums = args
    ids, off, ck = ps.cand_ids, ps.cand_off, ps.cand_ck
    if order is not None:
        order = torch.as_tensor(list(order), dtype=torch.long)
        counts = (off[1:] - off[:-1]).long()[order]
        new_off = torch.zeros(order.numel() + 1, dtype=torch.int32)
        new_off[1:] = counts.cumsum(0).to(torch.int32)
        parts = [ck[int(off[i]):int(off[i + 1])] for i in order.tolist()]
        ck = (torch.cat(parts) if parts
              else torch.empty(0, dtype=torch.int64)).contiguous()
        ids, off = ids[order].contiguous(), new_off
    return ext.pair_eig_finalize(h_after, h_base, pair_c, off.to(dev),
                                 ck.to(dev), ids.to(dev), adjusted,
                                 row_sums, fi.H_before).cpu()


class TestFinalizeStream:
    @pytest.mark.parametrize("name", list(TPK.FINALIZE))
    def test_vs_fp64(self, ext, dev, name):
        fi, q64 = TPK.finalize_refs(name)
        args = _fin_args(fi, dev)
        got, again = (_fin_run(ext, dev, fi, args) for _ in range(2))
        err = float((got.double() - q64).abs().max())
        print(f"finalize {name}: B={got.numel()} err {err:.3g} "
              f"tol {TPK.fin_tol(name):.3g}")
        assert got.shape == q64.shape
        assert err <= TPK.fin_tol(name), (name, err)
        assert torch.equal(got, again)

    @pytest.mark.parametrize("name", list(TPK.FINALIZE))
    def test_placement_independence(self, ext, dev, name):
        """A candidate's q does not depend on which wave of which block
        computes it, nor on what else is in the launch."""
        fi, _ = TPK.finalize_refs(name)
        args = _fin_args(fi, dev)
        full = _fin_run(ext, dev, fi, args)
        B = full.numel()
        assert B > 8
        g = torch.Generator().manual_seed(9)
        counts = fi.ps.cand_off[1:] - fi.ps.cand_off[:-1]
        orders = {
            "identity": list(range(B)),
            "reversed": list(range(B - 1, -1, -1)),
            "permuted": torch.randperm(B, generator=g).tolist(),
            "B-1": list(range(B - 1)),
            "B-3": list(range(B - 3)),
            "tail": list(range(3, B)),
            "one/first": [0],
            "one/last": [B - 1],
            "one/most hits": [int(counts.argmax())],
        }
        for what, order in orders.items():
            got = _fin_run(ext, dev, fi, args, order)
            assert torch.equal(got, full[order]), (name, what)

    def test_second_candidate_per_wave(self, ext, dev):
        """C = 8, B a little over one pass of the grid: waves 0..B -
        ONE_PASS - 1 take a second candidate, the rest do not. Against
        the fp64 reference (tolerance: the fp32 twin's own error times
        the finalize margin) and, bitwise, against the same candidates
        in launches that fit in one pass."""
        B = ONE_PASS + 107
        fi = PR.make_finalize_inputs(8, B, 8, 0.5, 1, seed=TPK.SEED)
        assert fi.ps.cand_ids.numel() == B
        q64 = PR.ref_finalize(fi.h_after, fi.ps, fi.adjusted, fi.row_sums,
                              fi.H_before)
        q32 = PR.ref_finalize(fi.h_after, fi.ps, fi.adjusted, fi.row_sums,
                              fi.H_before, f32=True)
        tol = TPK.FIN_MARGIN * float((q32 - q64).abs().max())
        args = _fin_args(fi, dev)
        got = _fin_run(ext, dev, fi, args)
        err = float((got.double() - q64).abs().max())
        print(f"finalize wrap: B={B} err {err:.3g} tol {tol:.3g}")
        assert err <= tol, err
        lo = _fin_run(ext, dev, fi, args, range(ONE_PASS))
        hi = _fin_run(ext, dev, fi, args, range(ONE_PASS, B))
        assert torch.equal(got, torch.cat([lo, hi]))
        # and with the two halves swapped: the wrapped waves now hold
        # other candidates
        order = list(range(ONE_PASS, B)) + list(range(ONE_PASS))
        assert torch.equal(_fin_run(ext, dev, fi, args, order), got[order])


# ---------------------------------------------------------------------
# cached entropy: live-row arguments
# ---------------------------------------------------------------------

def _entropy_three_ways(ext, dev, pr, ps_h, tb_h=None):
    """(uncached fused kernel, cached without, cached with live args).

    The call with the live-row arguments gets a cache whose rows in
    all-pad chunks are POISONED with NaN (pm, inv and a set vmask bit):
    it equals the others only if it reads none of them, and the call
    without the arguments on the same poisoned cache shows that they
    are what keeps it from reading them."""
    tb = TPC._dev_tables(pr.tables if tb_h is None else tb_h, dev)
    ps = TPC._dev_ps(ps_h, dev)
    pr_d = TPC._step_inputs(pr, dev)
    pm, pinv, a16 = TPC._build(ext, tb, ps)
    want = TPC._uncached(ext, tb, ps, pr_d, a16)
    plain = TPC._cached(ext, pm, pinv, ps, pr_d)
    unread = PSR.unread_rows(ps_h).to(dev)
    assert int(unread.sum()) >= 32
    pm_p, pinv_p, vm_p = pm.clone(), pinv.clone(), ps.vmask.clone()
    pm_p[unread] = float("nan")
    pinv_p[unread] = float("nan")
    vm_p[unread] = 1
    live_rows = ps_h.run_live.to(dev)
    live = ext.pair_entropy_cached(pm_p, pinv_p, vm_p, ps.pair_c, *pr_d,
                                   ps.run_off, live_rows)
    blind = ext.pair_entropy_cached(pm_p, pinv_p, vm_p, ps.pair_c, *pr_d)
    # (max(NaN, 1e-12) = 1e-12 per model: finite, and nowhere near)
    assert bool((blind[unread] != plain[unread]).all())
    assert torch.equal(blind[~unread], plain[~unread])
    # and on the clean cache
    assert torch.equal(ext.pair_entropy_cached(
        pm, pinv, ps.vmask, ps.pair_c, *pr_d, ps.run_off, live_rows), live)
    return want, plain, live


def _check_three(want, plain, live, what):
    assert torch.isfinite(want).all(), what
    assert torch.equal(plain, want), \
        (what, float((plain - want).abs().max()))
    assert torch.equal(live, plain), \
        (what, float((live - plain).abs().max()))


class TestEntropyLiveRows:
    @pytest.mark.parametrize("case", TPC.CASES)
    def test_cases(self, ext, dev, case):
        pr = TPK.stage2_inputs(*case)[0]
        ps = pr.ps
        pads = int(ps.K - ps.run_live.sum())
        print(f"entropy live {case}: K={ps.K} pads {pads} unread "
              f"{int(PSR.unread_rows(ps).sum())}")
        _check_three(*_entropy_three_ways(ext, dev, pr, ps), case)

    def test_skewed(self, ext, dev):
        pr = TPK.stage2_inputs(*TPC.SKEWED)[0]
        _check_three(*_entropy_three_ways(ext, dev, pr,
                                          TPC.skewed_structure()), "skewed")

    def test_boundaries_and_a_class_without_hits(self, ext, dev):
        pr = TPK.stage2_inputs(*BOUNDARY)[0]
        ps = boundary_structure()
        want, plain, live = _entropy_three_ways(ext, dev, pr, ps)
        _check_three(want, plain, live, "boundary")
        # pad rows carry their class's base value
        live = live.cpu()
        base = live[ps.base_pos][ps.pair_c.long()]
        pad = ps.pair_b < 0
        assert int(pad.sum()) == ps.K - sum(BOUNDARY_LIVE) + 5
        assert torch.equal(live[pad], base[pad])

    def test_live_arguments_go_together(self, ext, dev):
        pr = TPK.stage2_inputs(*BOUNDARY)[0]
        ps_h = boundary_structure()
        ps = TPC._dev_ps(ps_h, dev)
        pm = torch.zeros(ps_h.K, BOUNDARY[0], device=dev)
        pinv = torch.zeros(ps_h.K, device=dev)
        with pytest.raises(RuntimeError, match="go together"):
            ext.pair_entropy_cached(pm, pinv, ps.vmask, ps.pair_c,
                                    *TPC._step_inputs(pr, dev), ps.run_off)


# ---------------------------------------------------------------------
# one-class refresh, one block per tile
# ---------------------------------------------------------------------

class TestRefreshPerTile:
    def test_group_boundary(self, ext, dev):
        """Tiles of class 0: more than 4 (two groups at least) and not a
        multiple of 4; the other classes have fewer groups than the
        grid. Rows outside the class keep their bits; the class equals a
        fresh build (TestCacheKernels._refresh_and_check)."""
        ps = long_run_structure()
        tiles0 = int(ps.run_off[1] - ps.run_off[0]) // 128
        per = (ps.cls_grp_off[1:] - ps.cls_grp_off[:-1]).tolist()
        print(f"refresh per tile: class 0 has {tiles0} tiles, groups {per}")
        assert tiles0 > 4 and tiles0 % 4 != 0, tiles0
        assert per[0] == ps.max_grp >= 2 and min(per) < ps.max_grp, per
        pr = TPK.stage2_inputs(*TPC.SKEWED)[0]
        TPC.TestCacheKernels._refresh_and_check(ext, dev, TPC.SKEWED, pr, ps)

    def test_boundary_structure(self, ext, dev):
        """One tile per class, one of them all pads but the base row."""
        pr = TPK.stage2_inputs(*BOUNDARY)[0]
        TPC.TestCacheKernels._refresh_and_check(ext, dev, BOUNDARY, pr,
                                                boundary_structure())


# ---------------------------------------------------------------------
# get_pbest() from the merged graph's mixture
# ---------------------------------------------------------------------

def test_get_pbest_reuses_the_graph_mixture(pool, production):
    """After a replayed label the marginal comes from the graph's own
    mixture0: the same bits as computing it from the rows and pi_hat,
    a tensor of its own, and never served across a skip."""
    import coda_amd.ops as ops
    ds, oracle = pool
    production.delenv("CODA_AMD_NO_GRAPH", raising=False)
    production.delenv("CODA_AMD_NO_PAIR_CACHE", raising=False)
    sel = TPC._selector(ds)
    served = 0
    for step in range(5):
        i, q = sel.get_next_item_to_label()
        sel.add_label(i, oracle(int(i)), q)
        ver, mix = sel._mixture_cache
        hit = mix is not None and ver == sel._posterior_version
        got = sel.get_pbest()
        want = ops.mixture_entropy(sel._pbest_rows_before(), sel.pi_hat)[0]
        assert torch.equal(got, want), step
        if hit:
            served += 1
            assert got.data_ptr() != mix.data_ptr()
    assert sel._label_graph is not None
    # the first label is the warm-up + capture; every replay serves
    assert served == 4, served
    sel.skip(sel._active_candidates[3])
    assert sel._mixture_cache[1] is None
    want = ops.mixture_entropy(sel._pbest_rows_before(), sel.pi_hat)[0]
    assert torch.equal(sel.get_pbest(), want)
