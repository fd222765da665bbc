"""The pair cache without a GPU: the eager split it mirrors, the static
per-class views it refreshes through, the tolerance its GPU test uses,
the selector's bookkeeping on the CPU, and the new kernels' resources.

GPU counterpart: tests/test_pair_cache_gpu.py (same cases).
"""
from __future__ import annotations

import os
import random
import re
import subprocess

import pytest
import torch

from coda_amd.ops import pair as pops
from coda_amd.ops.reference import EPS_PROB
from tests import pair_ref as PR
from tests import test_pair_cache_gpu as G
from tests import test_pair_kernels as TPK

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"


def _legacy_pair_h_after(tables, ps, cls_rows, pbest_before, pi_hat,
                         mixture0):
    """pair_h_after as it stood before the pbn / entropy split (kept
    verbatim: the split is held to exact equality with it)."""
    EG, delta, s_base, w = (tables.EG, tables.delta, tables.s_base,
                            tables.weights)
    C, H, _, P = EG.shape
    K = ps.K
    device = EG.device
    seg_len = (ps.seg_off[1:] - ps.seg_off[:-1]).long()
    seg_pair = torch.repeat_interleave(
        torch.arange(K, device=device), seg_len)
    pc_long = ps.pair_c.long()
    dsum = torch.zeros(K, P, device=device)
    if ps.seg_h.numel():
        dsum.index_add_(0, seg_pair,
                        delta[pc_long[seg_pair], ps.seg_h.long()])
    if ps.pair_neg is not None and bool(ps.pair_neg.any()):
        dall = tables.dall if getattr(tables, "dall", None) is not None \
            else delta.sum(1)
        neg = ps.pair_neg.bool()
        dsum[neg] = dall[pc_long[neg]] - dsum[neg]
    A = torch.exp2(dsum + s_base[pc_long]) * w
    M = torch.einsum('kp,kjp->kj', A, EG.reshape(C, 2 * H, P)[pc_long])
    b_safe = ps.pair_b.long().clamp_min(0)
    v = (cls_rows[b_safe] == pc_long.unsqueeze(1)) \
        & (ps.pair_b >= 0).unsqueeze(1)
    j = 2 * torch.arange(H, device=device).unsqueeze(0) + v.long()
    pb = M.gather(1, j)
    tot = pb.sum(-1, keepdim=True).clamp_min(EPS_PROB)
    pbn = pb / tot
    mm = (mixture0.unsqueeze(0)
          + pi_hat[pc_long].unsqueeze(1)
          * (pbn - pbest_before[pc_long])).clamp_min(1e-12)
    return -(mm * torch.log2(mm)).sum(-1)


class TestEagerSplit:
    @pytest.mark.parametrize("case", G.CASES)
    def test_composition_equals_the_unsplit_formula(self, case):
        """pair_pbn o h_after_from_pbn is a pure refactor of
        pair_h_after: exact equality, op for op."""
        pr = TPK.stage2_inputs(*case)[0]
        args = (pr.tables, pr.ps, pr.cls_rows)
        pbn = pops.pair_pbn(*args)
        assert pbn.shape == (pr.ps.K, case[0])
        got = pops.h_after_from_pbn(pbn, pr.ps, pr.pi_hat,
                                    pr.pbest_before, pr.mixture0)
        want = _legacy_pair_h_after(*args, pr.pbest_before, pr.pi_hat,
                                    pr.mixture0)
        assert torch.equal(got, want)
        assert torch.equal(pops.pair_h_after(*args, pr.pbest_before,
                                             pr.pi_hat, pr.mixture0), want)

    def test_class_slice_recomputes_that_class(self):
        """pair_pbn over one class's run is that run of the full
        result (fp32 batched-GEMM blocking may move last bits: 1e-6)."""
        case = (12, 4000, 3, 0.6, 128)
        pr = TPK.stage2_inputs(*case)[0]
        full = pops.pair_pbn(pr.tables, pr.ps, pr.cls_rows)
        for y in range(case[2]):
            k0, k1 = int(pr.ps.run_off[y]), int(pr.ps.run_off[y + 1])
            part = pops.pair_pbn(pr.tables, pr.ps, pr.cls_rows, k0, k1)
            assert part.shape == (k1 - k0, case[0])
            torch.testing.assert_close(part, full[k0:k1], rtol=0, atol=1e-6)


class TestPerClassViews:
    @pytest.mark.parametrize("case", G.CASES + ["skewed"])
    def test_group_and_run_partitions(self, case):
        if case == "skewed":
            ps, C = G.skewed_structure(), G.SKEWED[2]
        else:
            ps, C = TPK.stage2_inputs(*case)[0].ps, case[2]
        cgo, ro, grp = ps.cls_grp_off, ps.run_off, ps.grp_off
        assert cgo.dtype == ro.dtype == torch.int32
        assert cgo.shape == ro.shape == (C + 1,)
        # cls_grp_off partitions grp_off's groups, class by class
        assert int(cgo[0]) == 0 and int(cgo[-1]) == grp.numel() - 1
        assert bool((cgo[1:] > cgo[:-1]).all())
        for c in range(C):
            for g in range(int(cgo[c]), int(cgo[c + 1])):
                k0, k1 = int(grp[g]) * 128, int(grp[g + 1]) * 128
                assert k1 > k0
                assert bool((ps.pair_c[k0:k1] == c).all()), (c, g)
            # the class's groups cover its run exactly
            assert int(grp[int(cgo[c])]) * 128 == int(ro[c])
            assert int(grp[int(cgo[c + 1])]) * 128 == int(ro[c + 1])
        # the run bounds tile K exactly
        assert int(ro[0]) == 0 and int(ro[-1]) == ps.K
        assert torch.equal(ro[:-1].long(), ps.base_pos)
        assert bool(((ro[1:] - ro[:-1]) % 128 == 0).all())
        assert ps.max_run == int((ro[1:] - ro[:-1]).max())
        assert ps.max_grp == int((cgo[1:] - cgo[:-1]).max())

    def test_small_tiles_have_no_views(self):
        ps = PR.make_problem(10, 300, 3, 0.5, seed=TPK.SEED).ps
        assert ps.tile == 16 and ps.cls_grp_off is None
        assert ps.run_off is None and ps.max_grp == 0 and ps.max_run == 0
        assert not pops.pair_cache_gate(
            PR.make_problem(10, 300, 3, 0.5, seed=TPK.SEED).tables, ps)


class TestTolerance:
    @pytest.mark.parametrize("case", G.CASES)
    def test_recorded_e_pbn_bounds_the_measurement(self, case):
        e = G.measure_e_pbn(case)
        print(case, e)
        rec = G.E_PBN[case]
        assert rec / TPK.HOST_BAND <= e <= rec * TPK.HOST_BAND, e
        ref = G.pbn_ref(case)
        # rows are distributions over the models; a dropped or doubled
        # column moves an entry by far more than the tolerance
        assert float((ref.sum(-1) - 1).abs().max()) < 1e-12
        assert float(ref.max()) > 100 * G.pbn_tol(case)


class TestCpuSelector:
    def test_only_the_labelled_class_is_recomputed(self, monkeypatch):
        """fp32 CPU selector on the pair engine, gate open (>= 4096
        candidates, 128-pair tiles): after each label exactly the
        labelled class's rows of the mirror cache move, and the cache
        equals a from-scratch pair_pbn."""
        from coda_amd import CODA, Oracle
        from coda_amd.datasets import Dataset
        from coda_amd.options import LOSS_FNS
        monkeypatch.delenv("CODA_AMD_NO_PAIR_CACHE", raising=False)
        H, N, C = 12, 6000, 3
        g = torch.Generator().manual_seed(5)
        cls = PR.consensus_classes(H, N, C, 0.45, seed=11)
        logits = torch.randn(H, N, C, generator=g)
        logits.scatter_add_(2, cls.t().unsqueeze(-1),
                            torch.full((H, N, 1), 4.0))
        preds = torch.softmax(logits, -1)
        labels = torch.randint(0, C, (N,), generator=g)
        ds = Dataset.from_tensors(preds, labels, "cpu")
        oracle = Oracle(ds, LOSS_FNS["acc"])
        random.seed(0)
        torch.manual_seed(0)
        sel = CODA(ds, eig_impl="pair")
        prev, moved = None, []
        for _ in range(4):
            i, q = sel.get_next_item_to_label()
            ps, cls_rows = sel._pair_acq.ps, sel._pair_acq.cls_rows
            cache = sel._pair_acq.cache
            assert ps.cand_ids.numel() >= 4096 and ps.tile == 128
            assert cache is not None and cache.pbn is not None
            assert cache.pm is None and not sel._pair_acq.stale
            torch.testing.assert_close(
                cache.pbn, pops.pair_pbn(sel._tables, ps, cls_rows),
                rtol=0, atol=1e-6)
            if prev is not None:
                y = sel.labels[-1]
                k0, k1 = int(ps.run_off[y]), int(ps.run_off[y + 1])
                same = torch.ones(ps.K, dtype=torch.bool)
                same[k0:k1] = False
                assert torch.equal(cache.pbn[same], prev[same])
                assert not torch.equal(cache.pbn[k0:k1], prev[k0:k1])
                moved.append(y)
            prev = cache.pbn.clone()
            sel.add_label(i, oracle(int(i)), q)
        assert len(moved) == 3

    def test_env_switch_and_invalidation(self, monkeypatch,
                                         synthetic_dataset, tmp_path):
        """CODA_AMD_NO_PAIR_CACHE=1 and a pool under the gate both leave
        the cache absent; a checkpoint restore drops it, and leaves
        every derived field as a fresh selector has it."""
        from coda_amd import CODA, checkpoint
        monkeypatch.setenv("CODA_AMD_NO_PAIR_CACHE", "1")
        assert not CODA(synthetic_dataset)._use_pair_cache
        monkeypatch.delenv("CODA_AMD_NO_PAIR_CACHE")
        sel = CODA(synthetic_dataset, eig_impl="pair")
        assert sel._use_pair_cache
        i, q = sel.get_next_item_to_label()
        acq = sel._pair_acq
        assert acq.ps.tile == 16
        assert acq.cache is None and acq.declined
        acq.cache = object()                # stand-in: restore must drop it
        path = checkpoint.save(sel, str(tmp_path / "c.pt"))
        checkpoint.load(sel, path)
        assert sel._pair_acq is None
        # nothing was labelled, so the restored state is the initial
        # one: every private field, whatever later changes add, equals
        # a fresh selector's
        fresh = CODA(synthetic_dataset, eig_impl="pair")
        assert vars(sel).keys() == vars(fresh).keys()
        for name, want in vars(fresh).items():
            if name.startswith("_"):
                assert _same_value(getattr(sel, name), want), name

    @pytest.fixture(scope="class")
    def restored_run(self, tmp_path_factory):
        """(uninterrupted 7-step selector, the one saved after 3 steps,
        a fresh one restored from it and run 4 further steps)."""
        from coda_amd import CODA, checkpoint
        ds, oracle = G._pool("cpu", 6000)

        def fresh():
            random.seed(0)
            torch.manual_seed(0)
            return CODA(ds, eig_impl="pair")

        def steps(sel, n):
            for _ in range(n):
                i, q = sel.get_next_item_to_label()
                sel.add_label(i, oracle(int(i)), q)

        with pytest.MonkeyPatch.context() as mp:
            mp.delenv("CODA_AMD_NO_PAIR_CACHE", raising=False)
            whole = fresh()
            steps(whole, 7)
            saved = fresh()
            steps(saved, 3)
            rng = random.getstate()
            path = checkpoint.save(
                saved, str(tmp_path_factory.mktemp("ckpt") / "s.pt"))
            restored = checkpoint.load(fresh(), path)
            assert restored._pair_acq is None and restored._tables is None
            random.setstate(rng)
            steps(restored, 4)
        return whole, saved, restored

    def test_restore_rebuilds_every_derived_object(self, restored_run):
        """Three steps, save, load into a fresh selector, four further
        steps: the restored selector shares no derived object with the
        saved one (structure, cache and mask are rebuilt) and labels
        the points the uninterrupted run labels."""
        whole, saved, restored = restored_run
        assert restored.labeled_idxs == whole.labeled_idxs
        assert restored._pair_acq.cache is not None
        derived = {**_objects(saved._pair_acq), **_objects(saved._tables),
                   **_objects(saved._pbest_rows_cache)}
        acq = saved._pair_acq
        for o in (acq.ps.pair_c, acq.cls_rows, acq.active, acq.row_of,
                  acq.cache.pbn, saved._tables.EG):
            assert id(o) in derived     # the walk reaches what matters
        shared = [name for name, v in vars(restored).items()
                  if _objects(v).keys() & derived.keys()]
        assert not shared, shared

    def test_restore_continues_q_vals_bitwise(self, restored_run):
        """...and reproduces the uninterrupted run's q_vals bit for bit:
        the checkpoint carries the pi_hat accumulators. (Recomputed by
        the full contraction they come out 5.7e-6 off the sum of the
        rank-1 increments here, and q 1e-7 off.)"""
        whole, _, restored = restored_run
        assert ([float(v) for v in restored.q_vals]
                == [float(v) for v in whole.q_vals])

    def test_checkpoint_without_accumulators_still_loads(self,
                                                         restored_run):
        """A checkpoint written before the accumulators were saved
        restores through the full contraction. (Each entry is a sum of
        H*C = 36 positive fp32 terms plus three increments, so either
        order of summation is within ~40 * 2^-24 = 2.4e-6 relative of
        the exact sum: 1e-5 between the two.)"""
        from coda_amd import CODA, checkpoint
        _, saved, _ = restored_run
        state = checkpoint.state_dict(saved)
        want = state["_adjusted"]
        del state["_adjusted"], state["_row_sums"]
        sel = checkpoint.load_state_dict(
            CODA(saved.dataset, eig_impl="pair"), state)
        torch.testing.assert_close(sel._adjusted, want, rtol=1e-5, atol=0)
        torch.testing.assert_close(sel.pi_hat, saved.pi_hat, rtol=1e-5,
                                   atol=0)


def _same_value(a, b):
    if torch.is_tensor(a) or torch.is_tensor(b):
        return (torch.is_tensor(a) and torch.is_tensor(b)
                and torch.equal(a, b))
    if isinstance(a, tuple):
        return (isinstance(b, tuple) and len(a) == len(b)
                and all(map(_same_value, a, b)))
    return a == b


def _objects(v, depth=3):
    """{id: object} of the tensors, mutable containers and class
    instances reachable from a value, a few levels down. (Tuples are
    looked through, not recorded: equal constants share one object.)"""
    if v is None or isinstance(v, (bool, int, float, str)):
        return {}
    out = {} if isinstance(v, tuple) else {id(v): v}
    if depth and not torch.is_tensor(v):
        kids = (v if isinstance(v, (tuple, set))
                else v.values() if isinstance(v, dict)
                else vars(v).values() if hasattr(v, "__dict__") else ())
        for k in kids:
            out.update(_objects(k, depth - 1))
    return out


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_cache_kernels_resource_envelope(tmp_path):
    """pair_entropy_cached keeps everything in registers; each
    pbn-writing GEMM stays within the registers and LDS of the fused
    kernel it derives from (figures read from the same compile)."""
    import sysconfig
    import torch.utils.cpp_extension as ce
    cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC",
           "-c", os.path.join(REPO, "coda_amd", "ops", "hip", "pair.hip"),
           "-o", str(tmp_path / "pair.o"),
           "-Rpass-analysis=kernel-resource-usage",
           "-DTORCH_EXTENSION_NAME=_kra", "-DTORCH_API_INCLUDE_EXTENSION_H",
           f"-D_GLIBCXX_USE_CXX11_ABI={int(torch.compiled_with_cxx11_abi())}",
           "-DUSE_ROCM=1", "-D__HIP_PLATFORM_AMD__=1"]
    cmd += [f"-I{p}" for p in ce.include_paths()]
    cmd += [f"-I{sysconfig.get_paths()['include']}"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    kernels, cur = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name:\s*(\S+)", line)
        if m:
            cur = m.group(1)
            kernels[cur] = {}
        for key, pat in (("vgpr", r" VGPRs:\s*(\d+)"),
                         ("agpr", r"AGPRs:\s*(\d+)"),
                         ("scratch", r"ScratchSize \[bytes/lane\]:\s*(\d+)"),
                         ("lds", r"LDS Size \[bytes/block\]:\s*(\d+)")):
            m = re.search(pat, line)
            if m and cur:
                kernels[cur][key] = int(m.group(1))

    def find(substr):
        hits = [v for k, v in kernels.items() if substr in k]
        assert len(hits) == 1, (substr, sorted(kernels))
        return hits[0]

    cached = find("pair_entropy_cached_kernel")
    assert cached["scratch"] == 0, cached
    assert find("pair_dsum_es_cls_kernel")["scratch"] == 0
    for jt in (4, 8, 16, 17):
        base = find(f"pair_gemm_entropy128_kernelILi{jt}E")
        pbn = find(f"pair_gemm_pbn128_kernelILi{jt}E")
        print(jt, base, pbn)
        assert pbn["vgpr"] + pbn["agpr"] <= base["vgpr"] + base["agpr"]
        assert pbn["lds"] <= base["lds"]
        assert pbn["scratch"] <= base["scratch"]
