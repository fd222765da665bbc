"""Hit-sparse ModelPicker entropy on the CPU: the eager twin of the HIP
kernel (ops.reference.modelpicker_dev) against the fp64 contract, the
tolerances and their mutation floors, and the selector's sparse path
against the dense one. References: tests/modelpicker_ref.py."""
import os
import random

import numpy as np
import pytest
import torch

import main as harness
from coda_amd import checkpoint as ckpt
from coda_amd import ops, tracking
from coda_amd.baselines import ModelPicker
from coda_amd.datasets import (Dataset, make_synthetic_task,
                               write_synthetic_task)
from tests import modelpicker_ref as R
from tests.test_modelpicker_sparse_gpu import RECORDED_TOL

# 16x the twin's error on the floor problems themselves
# (modelpicker_ref.measured_floor_tolerance), recorded
RECORDED_FLOOR_TOL = {
    (64, 10, "uniform"): 2.29e-07,
    (65, 1000, "spread3"): 1.99e-07,
    (128, 1000, "uniform"): 3.82e-07,
    (128, 1000, "spread60"): 4.15e-07,
    (1024, 300, "spread60"): 4.21e-07,
}


def _t(a):
    return torch.from_numpy(np.array(a))


def _within_factor(measured, recorded, factor=1.5):
    return recorded / factor <= measured <= recorded * factor


@pytest.mark.parametrize("C", R.GPU_C)
@pytest.mark.parametrize("H", R.GPU_H)
def test_tolerance_and_eager_twin(H, C):
    """The recorded tolerance is re-measured (fp32 twin vs dev64, x16),
    and the eager twin - what runs off the GPU - meets it."""
    measured = R.measured_tolerance(H, C)
    recorded = RECORDED_TOL[(H, C)]
    print(f"H={H} C={C}: measured tol {measured:.3g}, recorded "
          f"{recorded:.3g}")
    assert _within_factor(measured, recorded)

    rows, active = R.make_rows(H, C)
    st = ops.modelpicker_build(_t(rows))
    for kind in R.GPU_POSTERIORS:
        for eps in R.GPU_EPS:
            out = ops.modelpicker_dev(st, _t(R.make_posterior(H, kind, eps)),
                                      R.gamma_of(eps), _t(active))
            got = out.double().numpy()
            assert out.dtype == torch.float32
            assert np.all(np.isposinf(got[~active]))
            assert got[1] == 0.0          # all models agree
            err = float(np.abs(got - R.dev64_cached(H, C, kind, eps))
                        [active].max())
            print(f"  {kind} eps={eps}: max |eager - dev64| = {err:.3g}")
            assert err <= recorded


def test_static_structure_layout():
    rows = np.array([[5, 2, 5, 0, 2, 2],
                     [7, 7, 7, 7, 7, 7]])
    st = ops.modelpicker_build(_t(rows))
    pk = st.packed.numpy().astype(np.int32) & 0xffff
    # stable sort by class: ties keep ascending model index
    assert (pk[0] & 0x7fff).tolist() == [3, 1, 4, 5, 0, 2]
    assert (pk[0] >> 15).tolist() == [0, 1, 0, 0, 1, 0]
    assert (pk[1] & 0x7fff).tolist() == [0, 1, 2, 3, 4, 5]
    assert (pk[1] >> 15).tolist() == [0] * 6
    assert st.nseg.tolist() == [3, 1]
    assert st.packed.dtype == torch.int16


@pytest.mark.parametrize("H,C,kind,share", R.FLOOR_SHAPES)
def test_mutation_floors(H, C, kind, share):
    """Each fault, applied to the fp64 closed form, moves dev past the
    tolerance. A dropped hit class must do so on FLOOR_SHAPES' share of
    the rows; the other faults on at least one row in two (a dropped
    model can be one that carries no mass)."""
    eps = 0.45
    g = R.gamma_of(eps)
    rows = R.uniform_rows(H, C)
    post = R.make_posterior(H, kind, eps)
    packed, nseg = R.build(rows)
    want = R.dev64(rows, post, g)
    tol = R.measured_floor_tolerance(H, C, kind)
    recorded = RECORDED_FLOOR_TOL[(H, C, kind)]
    print(f"H={H} C={C} {kind}: measured tol {tol:.3g}, recorded "
          f"{recorded:.3g}")
    assert _within_factor(tol, recorded)
    clean = R.closed_dev(packed, nseg, post, g, f32=False)
    # the closed form ignores the clamp; that difference is far inside
    assert float(np.abs(clean - want).max()) <= recorded / R.MARGIN
    for fault in R.FAULTS:
        if fault == "ignore_pos64" and H <= 64:
            continue                      # no such position
        bad = R.closed_dev(packed, nseg, post, g, f32=False, fault=fault)
        caught = float((np.abs(bad - want) > recorded).mean())
        print(f"  {fault}: caught on {100 * caught:.0f} % of the rows")
        assert caught >= (share if fault == "drop_class" else 0.5), fault


def _ent_tol(H, C, dev_tol):
    """|fp32 entropies - fp64| of either path: an fp32 sum of H terms
    p log2 p (each a few roundings) of total size <= log2 H, twice for
    the two paths' own e0, next to dev_tol / C."""
    return 2 * (H + 4) * 2.0 ** -24 * np.log2(max(H, 2)) + dev_tol / C


def _dense_scores(sel):
    """The dense path's score vector over all N points (+inf on
    inactive ones), as get_next_item_to_label forms it."""
    preds_u = sel.classes_nh[sel.d_u_idxs]
    mask = sel._disagreement_mask[sel.d_u_idxs]
    ent = sel.compute_entropies(preds_u, sel.posterior, sel.Hl, sel.C,
                                sel.gamma).clone()
    if mask.any():
        ent[~mask] = float("inf")
    full = torch.full((sel.N,), float("inf"))
    full[sel.d_u_idxs] = ent
    return full


def _step_dev_tol(sel):
    """16x |fp32 twin - dev64| on the selector's own pool and posterior."""
    rows = sel.classes_nh.numpy()
    post = sel.posterior.numpy()
    twin = R.closed_dev(sel._struct.packed.numpy(), sel._struct.nseg.numpy(),
                        post, sel.gamma, f32=True)
    return R.MARGIN * float(np.abs(twin - R.dev64(rows, post,
                                                  sel.gamma)).max())


@pytest.mark.parametrize("H,N,C", [(3, 50, 2), (8, 120, 5), (65, 40, 10),
                                   (16, 60, 300)])
def test_entropies_match_dense_path(H, N, C):
    preds, labels = make_synthetic_task(H=H, N=N, C=C, seed=H)
    ds = Dataset.from_tensors(preds, labels, "cpu")
    dense = ModelPicker(ds, epsilon=0.4, entropy_impl="dense")
    sparse = ModelPicker(ds, epsilon=0.4, entropy_impl="sparse")
    for step in range(4):
        tol = _ent_tol(H, C, _step_dev_tol(sparse))
        want = _dense_scores(dense)
        got = sparse.sparse_entropies()
        assert torch.equal(torch.isinf(want), torch.isinf(got))
        fin = torch.isfinite(want)
        err = float((want[fin] - got[fin]).abs().max())
        print(f"step {step}: max |sparse - dense| = {err:.3g} "
              f"(tol {tol:.3g})")
        assert err <= tol
        torch.manual_seed(step)
        idx, q = dense.get_next_item_to_label()
        for s in (dense, sparse):
            s.add_label(idx, int(labels[idx]), q)


@pytest.mark.parametrize("H,N,C", [(6, 400, 4), (12, 300, 40)])
def test_trajectory_teacher_forced(H, N, C):
    """60 steps; the entropy landscape has exact plateaus, so the dense
    pick is applied to both (tests/test_reference_parity_long.py)."""
    preds, labels = make_synthetic_task(H=H, N=N, C=C, seed=11)
    ds = Dataset.from_tensors(preds, labels, "cpu")
    dense = ModelPicker(ds, epsilon=0.38, entropy_impl="dense")
    sparse = ModelPicker(ds, epsilon=0.38, entropy_impl="sparse")
    worst = 0.0
    for step in range(60):
        tol = _ent_tol(H, C, _step_dev_tol(sparse))
        want = _dense_scores(dense)
        got = sparse.sparse_entropies()
        assert torch.equal(torch.isinf(want), torch.isinf(got)), step
        fin = torch.isfinite(want)
        err = float((want[fin] - got[fin]).abs().max())
        worst = max(worst, err / tol)
        assert err <= tol, (step, err, tol)
        assert abs(float(want.min()) - float(got.min())) <= tol

        random.seed(1000 + step); torch.manual_seed(1000 + step)
        idx_d, q_d = dense.get_next_item_to_label()
        after_dense = torch.get_rng_state()
        random.seed(1000 + step); torch.manual_seed(1000 + step)
        idx_s, q_s = sparse.get_next_item_to_label()
        # one randint each: the streams stay in step
        assert torch.equal(torch.get_rng_state(), after_dense)
        assert q_s == q_d
        assert float(got[idx_s]) == float(got.min())
        y = int(labels[idx_d])
        dense.add_label(idx_d, y, q_d)
        sparse.add_label(idx_d, y, q_d)
        assert torch.equal(dense.posterior, sparse.posterior)
        assert sparse.d_u_idxs == dense.d_u_idxs
    print(f"worst |sparse - dense| / tol over 60 steps: {worst:.3g}")


def test_checkpoint_resume_sparse(tmp_path):
    preds, labels = make_synthetic_task(H=6, N=400, C=4, seed=3)
    ds = Dataset.from_tensors(preds, labels, "cpu")

    def run(sel, lo, hi):
        picks = []
        for step in range(lo, hi):
            torch.manual_seed(step)
            idx, q = sel.get_next_item_to_label()
            sel.add_label(idx, int(labels[idx]), q)
            picks.append(idx)
        return picks

    full = ModelPicker(ds, epsilon=0.4, entropy_impl="sparse")
    want = run(full, 0, 40)

    first = ModelPicker(ds, epsilon=0.4, entropy_impl="sparse")
    assert run(first, 0, 20) == want[:20]
    state = ckpt.state_dict(first)
    assert set(state) == {"__class__", "d_l_idxs", "d_l_ys", "d_u_idxs",
                          "posterior", "correct_counts", "stochastic"}
    path = ckpt.save(first, str(tmp_path / "mp.ckpt"))
    resumed = ModelPicker(ds, epsilon=0.4, entropy_impl="sparse")
    ckpt.load(resumed, path)
    assert int(resumed._unlabeled.sum()) == 400 - 20
    assert not resumed._unlabeled[want[:20]].any()
    assert run(resumed, 20, 40) == want[20:]
    assert torch.equal(resumed.posterior, full.posterior)


def test_entropy_impl_resolution():
    preds, labels = make_synthetic_task(H=6, N=50, C=4, seed=0)
    ds = Dataset.from_tensors(preds, labels, "cpu")
    assert ModelPicker(ds).entropy_impl == "dense"          # CPU, small
    assert ModelPicker(ds, entropy_impl="auto").entropy_impl == "dense"
    assert ModelPicker(ds, entropy_impl="sparse").entropy_impl == "sparse"
    with pytest.raises(ValueError):
        ModelPicker(ds, entropy_impl="fast")
    # over the size threshold but on the CPU: still dense
    big = ModelPicker.from_classes(torch.zeros(3000, 100, dtype=torch.long),
                                   num_classes=1000)
    assert big.N * big.C * big.H > ModelPicker.SPARSE_MIN_ELEMS
    assert big.entropy_impl == "dense"

    wide = Dataset.from_tensors(torch.rand(1025, 4, 2), None, "cpu")
    assert ModelPicker(wide).entropy_impl == "dense"
    with pytest.raises(ValueError):
        ModelPicker(wide, entropy_impl="sparse")
    many = Dataset.from_tensors(torch.rand(2, 3, 40000), None, "cpu")
    assert ModelPicker(many).entropy_impl == "dense"
    with pytest.raises(ValueError):
        ModelPicker(many, entropy_impl="sparse")
    shard = Dataset.from_tensors(preds, labels, "cpu", shard=(0, 2))
    assert ModelPicker(shard).entropy_impl == "dense"
    with pytest.raises(ValueError):
        ModelPicker(shard, entropy_impl="sparse")


def test_from_classes_matches_dataset_selector():
    preds, labels = make_synthetic_task(H=6, N=80, C=4, seed=2)
    a = ModelPicker(Dataset.from_tensors(preds, labels, "cpu"),
                    epsilon=0.4, entropy_impl="sparse")
    b = ModelPicker.from_classes(a.classes_nh, 4, epsilon=0.4,
                                 entropy_impl="sparse")
    assert torch.equal(a.sparse_entropies(), b.sparse_entropies())


def test_cli_mp_entropy_sparse(tmp_path):
    write_synthetic_task(str(tmp_path / "data"), name="synthtask",
                         H=6, N=200, C=4, seed=0)
    cwd = os.getcwd()
    os.chdir(tmp_path)
    try:
        tracking.set_tracking_uri("sqlite:///coda.sqlite")
        tracking._EXPERIMENT = None
        tracking._RUN_STACK.clear()
        seen = []
        orig = harness.build_selector

        def spy(*a, **k):
            seen.append(orig(*a, **k))
            return seen[-1]

        harness.build_selector = spy
        try:
            harness.main(["--task", "synthtask", "--data-dir", "data",
                          "--device", "cpu", "--method", "model_picker",
                          "--mp-entropy", "sparse", "--iters", "5",
                          "--seeds", "1", "--no-mlflow"])
        finally:
            harness.build_selector = orig
    finally:
        os.chdir(cwd)
    assert seen and seen[0].entropy_impl == "sparse"
    assert len(seen[0].d_l_idxs) == 5
