"""The pair cache's HIP kernels and its selector wiring (GPU).

The cache (coda_amd/ops/pair.py PairCache, kernels in ops/hip/pair.hip)
keeps, per pair k of a static 128-tile structure, the selected pairing
masses pm[k, :] (K, H) and their normalizer pinv[k] = 1/max(tot, 1e-30);
the pair's normalized P(best) is pbn[k, h] = pm[k, h] * pinv[k]. The
two factors stay unmultiplied because the fused kernel
pair_gemm_entropy128_kernel feeds that product into an fma without ever
rounding it, and pair_entropy_cached has to reproduce its bits.

Rows. Every row of the cache is computed. The LIVE rows - the ones
anything reads downstream - are each class's base pair and the
representative pairs (pair_b >= 0). Pad rows (pair_b = -1, not a base
pair) have an empty model segment and an all-zero vmask row like their
class's base pair, so they hold the base row's values bit for bit; the
tests check all rows and that equality.

Tolerance of pbn against fp64 (test_pbn_vs_fp64). Not calibrated on
kernel output: e_pbn is the reference's own fp32-vs-fp64 spread of
pb / tot on the test's inputs - tests/pair_ref.py's fp32 twin (M
accumulated in fp32 in a fixed 8-lane order, tot summed the same way,
one rounded division) against the fp64 value, from the same bf16
operands; emulated in fp64, so every host computes the same figure from
the same inputs. tests/test_pair_cache.py recomputes it on the CPU and
holds it within HOST_BAND of the value recorded here. The kernel gets
the pair tests' FUSED_MARGIN = 16 x e_pbn, for the same reasons: MFMA
accumulation order and DPP reduction order (plus the hardware
reciprocal).

  case (H, N, C, p, tile)        reaches                          e_pbn    16*e_pbn
  ----------------------------------------------------------------------------------
  (3, 600, 2, 0.5, 128)          JT 1, 2H % 16 != 0, W = 1        4.2e-08  6.8e-07
  (33, 1500, 5, 0.7, 128)        first H of <8>, W = 2            6.1e-08  9.8e-07
  (128, 400, 5, 0.6, 128)        the benchmark's H, <16>, W = 4   5.7e-08  9.2e-07
  (136, 600, 4, 0.7, 128)        <17>, last fused H               3.1e-08  5.0e-07
  (12, 4000, 3, 0.6, 128)        class runs over 4 tiles          9.9e-08  1.6e-06

(pbn lies in [0, 1]; one fp32 ulp just below 1 is 6e-8.) Every class of
these five structures has the same number of tile groups, so no block
of a one-class launch lies past its class's range; the skewed structure
of test_refresh_blocks_past_the_class_return (group counts 3, 1, 1)
adds that path.

Everything else here is bitwise: pair_entropy_cached against
pair_gemm_entropy (the EIG maximum of the benchmark sits on the fp32
cancellation floor with hundreds of ties, so a last-bit change in
h_after changes the trajectory), a one-class refresh against a fresh
full build, and the selector with the cache against the selector
without it.
"""
from __future__ import annotations

import functools
import random

import pytest
import torch

from tests import pair_ref as PR
from tests import test_pair_kernels as TPK

pytestmark = pytest.mark.gpu

# (H, N, C, p, tile) -> recorded e_pbn (measured value rounded up)
E_PBN = {
    (3, 600, 2, 0.5, 128): 4.2e-08,
    (33, 1500, 5, 0.7, 128): 6.1e-08,
    (128, 400, 5, 0.6, 128): 5.7e-08,
    (136, 600, 4, 0.7, 128): 3.1e-08,
    (12, 4000, 3, 0.6, 128): 9.9e-08,
}
CASES = list(E_PBN)
TABLE_FIELDS = ("EG", "delta", "s_base", "weights", "egw", "delta16", "dall")
PS_FIELDS = ("cand_ids", "pair_b", "pair_c", "seg_off", "seg_h", "base_pos",
             "cand_off", "cand_pairs", "vmask", "pair_neg", "cand_ck",
             "grp_off", "cls_grp_off", "run_off")


# ---------------------------------------------------------------------
# CPU-side references (shared with tests/test_pair_cache.py)
# ---------------------------------------------------------------------

SKEWED = (12, 4000, 3, 0.6, 128)     # tables of this case, own structure


@functools.lru_cache(maxsize=None)
def skewed_structure():
    """A 128-tile structure whose classes have 3, 1 and 1 tile groups:
    class 0 is every point's consensus class."""
    from coda_amd.ops import pair as pops
    H, N, C = SKEWED[:3]
    g = torch.Generator().manual_seed(3)
    agree = torch.rand(N, H, generator=g) < 0.6
    unif = torch.randint(0, C, (N, H), generator=g)
    cls = torch.where(agree, torch.zeros(N, H, dtype=torch.long), unif)
    return pops.build_pairs(cls, torch.arange(N), C, tile=128)


@functools.lru_cache(maxsize=None)
def pbn_ref(case) -> torch.Tensor:
    """(K, H) fp64 pb / max(tot, 1e-30) from the reference A operand."""
    _, _, _, args = TPK.stage2_inputs(*case)
    pb = PR.ref_select(*args[:4])
    tot = pb.sum(-1, keepdim=True).clamp_min(
        PR._f32c(1e-30, torch.float64))
    return pb / tot


def measure_e_pbn(case) -> float:
    """max |fp32 twin - fp64| of pb / tot on the case's inputs."""
    _, _, _, args = TPK.stage2_inputs(*case)
    pb32 = PR.ref_select(*args[:4], m_f32=True, lanes=8)
    tot32 = PR._sum32(pb32, 8).unsqueeze(-1).clamp_min(
        PR._f32c(1e-30, torch.float64))
    pbn32 = PR._r32(pb32 / tot32)
    return float((pbn32 - pbn_ref(case)).abs().max())


def pbn_tol(case) -> float:
    return TPK.FUSED_MARGIN * E_PBN[case]


def clone_tables(tb):
    return tb._replace(**{f: getattr(tb, f).clone() for f in TABLE_FIELDS})


def perturbed_tables(case, y: int):
    """The case's tables after class y's Beta column moved, through the
    project's own row refresh (dall / egw / delta16 stay consistent)."""
    from coda_amd.ops import table as tops
    pr = TPK.stage2_inputs(*case)[0]
    H, C = case[0], case[2]
    assert 0 <= y < C
    g = torch.Generator().manual_seed(77 + y)
    alpha = torch.rand(H, C, generator=g) * 20 + 1.0
    beta = torch.rand(H, C, generator=g) * 5 + 2.0
    tb = clone_tables(pr.tables)
    tops.table_update_rows(tb, alpha, beta, [y])
    assert not torch.equal(tb.egw[y], pr.tables.egw[y])
    return tb


def refresh_classes(ps, C: int):
    """y in {0, C-1, the class with the most groups}."""
    per = (ps.cls_grp_off[1:] - ps.cls_grp_off[:-1])
    return sorted({0, C - 1, int(per.argmax())})


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


def _dev_tables(tb, dev):
    return tb._replace(**{f: getattr(tb, f).to(dev) for f in TABLE_FIELDS})


def _dev_ps(ps, dev):
    return ps._replace(**{f: getattr(ps, f).to(dev) for f in PS_FIELDS})


def _build(ext, tb, ps, a16=None):
    """All-groups build -> (pm, pinv); a16 defaults to pair_dsum_es."""
    if a16 is None:
        a16 = ext.pair_dsum_es(tb.delta16, tb.dall, ps.pair_c, ps.pair_neg,
                               ps.seg_off, ps.seg_h)
    H = tb.EG.shape[1]
    # NaN-filled: a row the kernel skipped cannot pass for computed
    pm = torch.full((ps.K, H), float("nan"), device=a16.device)
    pinv = torch.full((ps.K,), float("nan"), device=a16.device)
    ext.pair_gemm_pbn(a16, tb.egw, ps.vmask, ps.pair_c, ps.grp_off, pm,
                      pinv)
    return pm, pinv, a16


def _uncached(ext, tb, ps, pr_d, a16=None):
    if a16 is None:
        a16 = ext.pair_dsum_es(tb.delta16, tb.dall, ps.pair_c, ps.pair_neg,
                               ps.seg_off, ps.seg_h)
    return ext.pair_gemm_entropy(a16, tb.egw, ps.vmask, ps.pair_c, *pr_d,
                                 ps.tile, 0, ps.grp_off)


def _cached(ext, pm, pinv, ps, pr_d):
    return ext.pair_entropy_cached(pm, pinv, ps.vmask, ps.pair_c, *pr_d)


def _step_inputs(pr, dev):
    return (pr.pi_hat.to(dev), pr.pbest_before.to(dev).contiguous(),
            pr.mixture0.to(dev))


class TestCacheKernels:
    @pytest.mark.parametrize("case", CASES)
    def test_pbn_vs_fp64(self, ext, dev, case):
        """All-groups build from the reference A operand: pm * pinv
        against fp64 pb / tot, every row; pad rows equal their class's
        base row bit for bit."""
        pr, a16, _, _ = TPK.stage2_inputs(*case)
        ps = pr.ps
        assert ps.tile == 128 and ps.K % 128 == 0
        assert TPK.jt_width(case[0]) == TPK.FUSED128[case][0]
        pm, pinv, _ = _build(ext, _dev_tables(pr.tables, dev),
                             _dev_ps(ps, dev), a16.to(dev))
        pm, pinv = pm.cpu(), pinv.cpu()
        assert torch.isfinite(pm).all() and torch.isfinite(pinv).all()
        got = pm.double() * pinv.double().unsqueeze(1)
        ref = pbn_ref(case)
        err = float((got - ref).abs().max())
        print(f"pbn {case}: K={ps.K} max err {err:.3g} "
              f"tol {pbn_tol(case):.3g}")
        assert err <= pbn_tol(case), (case, err)
        pad = ps.pair_b < 0
        pad[ps.base_pos] = False
        base_row = ps.base_pos[ps.pair_c.long()]
        assert torch.equal(pm[pad], pm[base_row][pad])
        assert torch.equal(pinv[pad], pinv[base_row][pad])

    @pytest.mark.parametrize("case", CASES)
    def test_cached_entropy_is_bitwise_the_fused_kernel(self, ext, dev,
                                                        case):
        """pair_entropy_cached(build(...)) == pair_gemm_entropy(...) on
        the same device inputs, every row (live and pad)."""
        pr, a16, _, _ = TPK.stage2_inputs(*case)
        tb, ps = _dev_tables(pr.tables, dev), _dev_ps(pr.ps, dev)
        pr_d = _step_inputs(pr, dev)
        a16 = a16.to(dev)
        pm, pinv, _ = _build(ext, tb, ps, a16)
        got = _cached(ext, pm, pinv, ps, pr_d)
        want = _uncached(ext, tb, ps, pr_d, a16)
        assert got.shape == want.shape == (ps.K,)
        assert torch.isfinite(want).all()
        assert torch.equal(got, want), \
            float((got - want).abs().max())
        assert torch.equal(got, _cached(ext, pm, pinv, ps, pr_d))

    @pytest.mark.parametrize("case", CASES)
    def test_one_class_refresh(self, ext, dev, case):
        """Perturb class y's table rows, refresh y with the class id on
        the device: rows outside y's run keep their bits, the whole
        cache equals a fresh build from the perturbed tables, and so
        does h_after against the uncached kernels."""
        pr = TPK.stage2_inputs(*case)[0]
        per = (pr.ps.cls_grp_off[1:] - pr.ps.cls_grp_off[:-1])
        if case == (12, 4000, 3, 0.6, 128):
            assert int(per.max()) >= 2, "no class with a second group"
        self._refresh_and_check(ext, dev, case, pr, pr.ps)

    def test_refresh_blocks_past_the_class_return(self, ext, dev):
        """Classes with fewer groups than the launch grid (3, 1, 1): the
        surplus blocks of a one-group class's refresh write nothing."""
        pr = TPK.stage2_inputs(*SKEWED)[0]
        ps = skewed_structure()
        per = (ps.cls_grp_off[1:] - ps.cls_grp_off[:-1]).tolist()
        assert per == [3, 1, 1] and ps.max_grp == 3, per
        self._refresh_and_check(ext, dev, SKEWED, pr, ps)

    @staticmethod
    def _refresh_and_check(ext, dev, case, pr, ps_h):
        C = case[2]
        ps = _dev_ps(ps_h, dev)
        pr_d = _step_inputs(pr, dev)
        pm, pinv, _ = _build(ext, _dev_tables(pr.tables, dev), ps)
        a_run = torch.zeros(ps_h.max_run, 256, dtype=torch.bfloat16,
                            device=dev)
        for y in refresh_classes(ps_h, C):
            tb2 = _dev_tables(perturbed_tables(case, y), dev)
            k0, k1 = int(ps_h.run_off[y]), int(ps_h.run_off[y + 1])
            assert k1 - k0 <= ps_h.max_run and (y < C - 1 or k1 == ps_h.K)
            pm_r, pinv_r = pm.clone(), pinv.clone()
            y_t = torch.tensor([y], dtype=torch.long, device=dev)
            ext.pair_dsum_es_cls(tb2.delta16, tb2.dall, ps.pair_c,
                                 ps.pair_neg, ps.seg_off, ps.seg_h,
                                 ps.run_off, y_t, a_run)
            ext.pair_gemm_pbn(a_run, tb2.egw, ps.vmask, ps.pair_c,
                              ps.grp_off, pm_r, pinv_r, ps.cls_grp_off,
                              ps.run_off, y_t, ps_h.max_grp)
            outside = torch.ones(ps_h.K, dtype=torch.bool, device=dev)
            outside[k0:k1] = False
            assert torch.equal(pm_r[outside], pm[outside]), y
            assert torch.equal(pinv_r[outside], pinv[outside]), y
            assert not torch.equal(pm_r[k0:k1], pm[k0:k1]), y
            pm_f, pinv_f, a_f = _build(ext, tb2, ps)
            assert torch.equal(pm_r, pm_f), y
            assert torch.equal(pinv_r, pinv_f), y
            assert torch.equal(_cached(ext, pm_r, pinv_r, ps, pr_d),
                               _uncached(ext, tb2, ps, pr_d, a_f)), y


# ---------------------------------------------------------------------
# selector level
# ---------------------------------------------------------------------

def _pool(dev, N):
    from coda_amd import Oracle
    from coda_amd.datasets import Dataset
    from coda_amd.options import LOSS_FNS
    g = torch.Generator().manual_seed(5)
    cls = PR.consensus_classes(12, N, 3, 0.45, seed=11)       # (N, H)
    logits = torch.randn(12, N, 3, generator=g)
    logits.scatter_add_(2, cls.t().unsqueeze(-1),
                        torch.full((12, N, 1), 4.0))
    preds = torch.softmax(logits, -1).to(dev)
    labels = torch.randint(0, 3, (N,), generator=g).to(dev)
    ds = Dataset.from_tensors(preds, labels, dev)
    return ds, Oracle(ds, LOSS_FNS["acc"])


@pytest.fixture(scope="module")
def pool(dev):
    return _pool(dev, 6000)


@pytest.fixture()
def production(monkeypatch):
    """Guards off: they synchronize per op and keep the graphs out."""
    import coda_amd.selectors.coda as coda_mod
    import coda_amd.ops as ops_mod
    import coda_amd.util as util_mod
    monkeypatch.setattr(coda_mod, "DEBUG", False)
    monkeypatch.setattr(ops_mod, "DEBUG", False)
    monkeypatch.setattr(util_mod, "DEBUG", False)
    return monkeypatch


def _selector(ds):
    """Seeded, and built with torch's deterministic algorithms: the
    consensus prior is a float index_add_ that otherwise sums in block
    arrival order, and its last bits move q by ~5e-7 from one
    construction to the next (bench.reproducible_setup)."""
    import bench
    from coda_amd import CODA
    random.seed(0)
    torch.manual_seed(0)
    with bench.reproducible_setup():
        return CODA(ds)


def _run(pool, mp, *, cache, no_graph=False, ckpt_at=None, skip_at=None,
         tmp_path=None, steps=8, expect_cache=True):
    from coda_amd import checkpoint
    ds, oracle = pool
    for name, on in (("CODA_AMD_NO_PAIR_CACHE", not cache),
                     ("CODA_AMD_NO_GRAPH", no_graph)):
        if on:
            mp.setenv(name, "1")
        else:
            mp.delenv(name, raising=False)
    sel = _selector(ds)
    skipped = []
    for s in range(steps):
        if ckpt_at == s:
            path = str(tmp_path / f"sel_{int(cache)}.pt")
            checkpoint.save(sel, path)
            sel = _selector(ds)
            checkpoint.load(sel, path)
            assert sel._pair_acq is None
        if skip_at == s:
            skipped.append(sel._active_candidates[3])
            sel.skip(skipped[-1])
        i, q = sel.get_next_item_to_label()
        # nothing computed before a skip or a label may be returned
        assert int(i) not in skipped and int(i) not in sel.labeled_idxs
        ps = sel._pair_acq.ps
        if expect_cache:
            assert ps.cand_ids.numel() >= 4096 and ps.tile == 128
        assert (sel._pair_acq.cache is not None) == (cache and expect_cache)
        sel.add_label(i, oracle(int(i)), q)
        sel.get_best_model_prediction()
    assert (sel._label_graph is None) == no_graph
    return sel.labeled_idxs, sel.q_vals


class TestSelector:
    @pytest.mark.parametrize("arrangement", ["plain", "no_graph",
                                             "checkpoint", "skip",
                                             "skip_first"])
    def test_cached_trajectory_is_bitwise_the_uncached(
            self, pool, production, tmp_path, arrangement):
        """Eight steps with the cache and eight with
        CODA_AMD_NO_PAIR_CACHE=1, same seeds: identical labeled_idxs,
        bit-equal q_vals. skip_first skips right after the first label,
        while the selection the label graph's warm-up computed is still
        pending: it must be recomputed, never returned."""
        kw = dict(no_graph=arrangement == "no_graph",
                  ckpt_at=4 if arrangement == "checkpoint" else None,
                  skip_at={"skip": 2, "skip_first": 1}.get(arrangement),
                  tmp_path=tmp_path)
        idx_c, q_c = _run(pool, production, cache=True, **kw)
        idx_u, q_u = _run(pool, production, cache=False, **kw)
        assert len(idx_c) == 8 and len(set(idx_c)) == 8
        assert idx_c == idx_u
        assert [float(v) for v in q_c] == [float(v) for v in q_u]

    def test_small_pool_stays_uncached(self, dev, production):
        """Below the gate (16-pair tiles) the cache is absent and the
        two settings still agree."""
        small = _pool(dev, 600)
        a = _run(small, production, cache=True, expect_cache=False)
        b = _run(small, production, cache=False, expect_cache=False)
        assert a[0] == b[0]
        assert [float(v) for v in a[1]] == [float(v) for v in b[1]]
