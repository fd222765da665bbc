"""Hit-sparse ModelPicker entropy: the gfx950 kernel against the fp64
contract (tests/modelpicker_ref.py), and the selector on the GPU.

RECORDED_TOL is the absolute tolerance on dev per (H, C): 16x the worst
|fp32 twin - dev64| over the case's rows, the three posteriors and the
two epsilons, measured on the CPU (modelpicker_ref.measured_tolerance) -
never from kernel output. tests/test_modelpicker_sparse.py re-measures it
and holds it within a factor 1.5 of these values. dev itself is O(0.1):
the tolerances sit 4 to 5 digits below it.
"""
import numpy as np
import pytest
import torch

from coda_amd import ops
from tests import modelpicker_ref as R

RECORDED_TOL = {
    (3, 2): 6.06e-07, (3, 10): 1.38e-06, (3, 1000): 1.38e-06,
    (3, 32767): 1.38e-06,
    (64, 2): 3.22e-06, (64, 10): 2.43e-06, (64, 1000): 2.61e-06,
    (64, 32767): 3.1e-06,
    (65, 2): 2.82e-06, (65, 10): 3.03e-06, (65, 1000): 2.83e-06,
    (65, 32767): 3.42e-06,
    (128, 2): 2.44e-06, (128, 10): 4.1e-06, (128, 1000): 5.4e-06,
    (128, 32767): 5.4e-06,
    (1000, 2): 2.22e-05, (1000, 10): 2.16e-05, (1000, 1000): 7.45e-05,
    (1000, 32767): 7.45e-05,
    (1024, 2): 6.96e-06, (1024, 10): 6.68e-06, (1024, 1000): 6.32e-05,
    (1024, 32767): 6.33e-05,
}

pytestmark = pytest.mark.gpu

GPU_N = (1, 5, 257)   # a single wave, a partial block, a ragged grid


def _dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _struct(rows, n, device):
    """The static structure of the first n rows, built on the device."""
    st = ops.modelpicker_build(
        torch.from_numpy(np.array(rows[:n])).to(device))
    cpu = ops.modelpicker_build(torch.from_numpy(np.array(rows[:n])))
    assert torch.equal(st.packed.cpu(), cpu.packed)
    assert torch.equal(st.nseg.cpu(), cpu.nseg)
    return st


@pytest.mark.parametrize("C", R.GPU_C)
@pytest.mark.parametrize("H", R.GPU_H)
def test_kernel_matches_fp64_contract(H, C):
    """Every (N, epsilon, posterior) of the shape; the rows hold the
    all-agree, all-distinct, 63|64-boundary, 900-model-segment and
    inactive cases (modelpicker_ref.make_rows)."""
    device = _dev()
    rows, active = R.make_rows(H, C)
    tol = RECORDED_TOL[(H, C)]
    for n in GPU_N:
        st = _struct(rows, n, device)
        act = torch.from_numpy(np.array(active[:n])).to(device)
        for kind in R.GPU_POSTERIORS:
            for eps in R.GPU_EPS:
                post = torch.from_numpy(
                    np.array(R.make_posterior(H, kind, eps))).to(device)
                out = ops.modelpicker_dev(st, post, R.gamma_of(eps), act)
                again = ops.modelpicker_dev(st, post, R.gamma_of(eps), act)
                assert out.dtype == torch.float32 and out.shape == (n,)
                assert torch.equal(out.view(torch.int32),
                                   again.view(torch.int32)), "not bit-equal"
                got = out.cpu().double().numpy()
                want = R.dev64_cached(H, C, kind, eps)[:n]
                a = active[:n]
                assert np.all(np.isposinf(got[~a])), (n, kind, eps)
                err = float(np.abs(got - want)[a].max())
                print(f"H={H} C={C} N={n} {kind} eps={eps}: "
                      f"max |kernel - dev64| = {err:.3g} (tol {tol:.3g})")
                assert np.all(np.isfinite(got[a]))
                if n > 1:
                    assert got[1] == 0.0, "all models agree: exactly 0"
                assert err <= tol, (n, kind, eps, err, tol)


def test_inactive_points_get_inf_and_all_inactive():
    device = _dev()
    rows, _ = R.make_rows(128, 10)
    st = _struct(rows, 257, device)
    post = torch.from_numpy(np.array(R.make_posterior(128, "spread60",
                                                      0.36))).to(device)
    none = torch.zeros(257, dtype=torch.uint8, device=device)
    out = ops.modelpicker_dev(st, post, R.gamma_of(0.36), none)
    assert torch.isposinf(out).all()
    one = none.clone()
    one[200] = 1
    out = ops.modelpicker_dev(st, post, R.gamma_of(0.36), one)
    assert torch.isposinf(out).sum() == 256 and torch.isfinite(out[200])


def _onehot_pool(H, N, C, device, seed=0):
    """(H, N, C) fp32 one-hot predictions of a consensus-heavy pool."""
    g = torch.Generator().manual_seed(seed)
    true = torch.randint(0, C, (1, N), generator=g)
    agree = torch.rand(H, N, generator=g) < 0.6
    cls = torch.where(agree, true.expand(H, N),
                      torch.randint(0, C, (H, N), generator=g)).to(device)
    preds = torch.zeros(H, N, C, device=device)
    preds.scatter_(2, cls.unsqueeze(-1), 1.0)
    return preds, true.flatten(), cls


def test_auto_resolves_sparse_on_a_big_pool():
    """(H=128, N=4096, C=1000): N*C*H > 2**28, so auto picks the kernel.
    Three steps run; the scores of 64 sampled points are held to fp64.
    The dense path is never run at this size."""
    from coda_amd.baselines import ModelPicker
    from coda_amd.datasets import Dataset
    device = _dev()
    H, N, C, eps = 128, 4096, 1000, 0.45
    preds, labels, cls = _onehot_pool(H, N, C, device)
    sel = ModelPicker(Dataset.from_tensors(preds, labels, device),
                      epsilon=eps)
    del preds
    assert sel.entropy_impl == "sparse"
    rows = cls.t().cpu().numpy()
    sample = np.random.default_rng(0).choice(N, size=64, replace=False)
    tol = RECORDED_TOL[(128, 1000)]
    torch.manual_seed(0)
    for step in range(3):
        ent = sel.sparse_entropies().cpu().double().numpy()
        post = sel.posterior.cpu().numpy()
        want = (R.dense_e0_64(post)
                + R.dev64(rows[sample], post, sel.gamma) / C)
        unl = np.ones(N, dtype=bool)
        unl[sel.d_l_idxs] = False
        dis = sel._disagreement_mask.cpu().numpy()
        act = unl & dis if (unl & dis).any() else unl
        assert np.array_equal(np.isposinf(ent), ~act)
        keep = act[sample]
        err = float(np.abs(ent[sample] - want)[keep].max())
        # e0 is an fp32 sum of H terms next to dev / C
        e0_tol = 2 * (H + 4) * 2.0 ** -24 * np.log2(H)
        print(f"step {step}: max |entropies - fp64| = {err:.3g} "
              f"(tol {e0_tol + tol / C:.3g})")
        assert err <= e0_tol + tol / C
        idx, q = sel.get_next_item_to_label()
        assert act[idx] and ent[idx] == ent[act].min()
        assert q == 1.0 / (N - step)
        sel.add_label(idx, int(labels[idx]), q)


def test_selector_gpu_matches_cpu_sparse_teacher_forced():
    """30 steps, GPU sparse against CPU sparse; the CPU pick is applied
    to both (the landscape has exact plateaus)."""
    from coda_amd.baselines import ModelPicker
    from coda_amd.datasets import Dataset, make_synthetic_task
    device = _dev()
    H, N, C, eps = 12, 300, 40, 0.38
    preds, labels = make_synthetic_task(H=H, N=N, C=C, seed=5)
    cpu = ModelPicker(Dataset.from_tensors(preds, labels, "cpu"),
                      epsilon=eps, entropy_impl="sparse")
    gpu = ModelPicker(Dataset.from_tensors(preds, labels, device),
                      epsilon=eps, entropy_impl="sparse")
    rows = cpu.classes_nh.numpy()
    for step in range(30):
        post = cpu.posterior.numpy()
        packed, nseg = cpu._struct.packed.numpy(), cpu._struct.nseg.numpy()
        twin = R.closed_dev(packed, nseg, post, cpu.gamma, f32=True)
        tol = (R.MARGIN * float(np.abs(
            twin - R.dev64(rows, post, cpu.gamma)).max()) / C
            + 2 * (H + 4) * 2.0 ** -24 * np.log2(H))
        e_cpu = cpu.sparse_entropies()
        e_gpu = gpu.sparse_entropies().cpu()
        assert torch.equal(torch.isinf(e_cpu), torch.isinf(e_gpu))
        fin = torch.isfinite(e_cpu)
        err = float((e_cpu[fin] - e_gpu[fin]).abs().max())
        print(f"step {step}: max |gpu - cpu| = {err:.3g} (tol {2 * tol:.3g})")
        # each side is within tol of fp64
        assert err <= 2 * tol
        assert abs(float(e_cpu.min()) - float(e_gpu.min())) <= 2 * tol
        torch.manual_seed(100 + step)
        idx, q = cpu.get_next_item_to_label()
        torch.manual_seed(100 + step)
        idx_g, q_g = gpu.get_next_item_to_label()
        assert q == q_g and not torch.isinf(e_gpu[idx_g])
        y = int(labels[idx])
        cpu.add_label(idx, y, q)
        gpu.add_label(idx, y, q)
        torch.testing.assert_close(gpu.posterior.cpu(), cpu.posterior,
                                   rtol=1e-5, atol=1e-7)
