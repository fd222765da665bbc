"""Trajectory parity against the upstream reference implementation.

The reference (justinkay/coda) is pure PyTorch. What it computes on these
synthetic tasks with these seeds is recorded under
tests/golden/reference_parity/ (oracle/record_parity_golden.py makes the
recordings from a checkout of the reference); the tests run this engine on
the same task with the same seeds and require identical selection
trajectories.
"""
import os
import random

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)),
                      "golden", "reference_parity")


def _golden(name, H, N, C, seed):
    """Load a recording, checking it was made on this very task."""
    g = np.load(os.path.join(GOLDEN, name + ".npz"))
    assert g["task"].tolist() == [H, N, C, seed], \
        f"{name}: recorded on task {g['task'].tolist()}, re-record"
    return g


def _mk(seed=0, H=8, N=300, C=5):
    from coda_amd.datasets import make_synthetic_task
    return make_synthetic_task(H=H, N=N, C=C, seed=seed)


def test_coda_trajectory_parity():
    from coda_amd.datasets import Dataset
    from coda_amd import CODA

    ref = _golden("coda_trajectory", 8, 300, 5, 0)
    preds, labels = _mk()

    random.seed(0); torch.manual_seed(0)
    mine = CODA(Dataset.from_tensors(preds, labels, "cpu"))

    torch.testing.assert_close(torch.from_numpy(ref["pbest0"]),
                               mine.get_pbest().reshape(-1),
                               rtol=1e-4, atol=1e-6)

    for m in range(5):
        ir, qr = int(ref["idx"][m]), float(ref["q"][m])
        random.seed(100 + m)
        im, qm = mine.get_next_item_to_label()
        assert ir == int(im), (m, ir, int(im))
        assert abs(qr - qm) < 1e-5
        y = int(labels[ir])
        mine.add_label(int(im), y, qm)
        assert int(ref["best"][m]) == \
            int(mine.get_best_model_prediction())


def test_modelpicker_entropy_parity():
    from coda_amd.datasets import Dataset
    from coda_amd.baselines import ModelPicker

    ref = _golden("modelpicker_entropy", 8, 300, 5, 3)
    preds, labels = _mk(seed=3)
    mine = ModelPicker(Dataset.from_tensors(preds, labels, "cpu"),
                       epsilon=0.45)

    preds_u = preds.argmax(2).transpose(0, 1)[:60]
    e_ref = torch.from_numpy(ref["entropies"])
    e_mine = mine.compute_entropies(preds_u, mine.posterior, mine.Hl,
                                    mine.C, mine.gamma)
    torch.testing.assert_close(e_ref, e_mine, rtol=1e-5, atol=1e-6)


def test_oracle_losses_parity():
    from coda_amd.datasets import Dataset
    from coda_amd.oracle import Oracle
    from coda_amd.options import LOSS_FNS

    ref = _golden("oracle_losses", 8, 300, 5, 4)
    preds, labels = _mk(seed=4)
    mine = Oracle(Dataset.from_tensors(preds, labels, "cpu"),
                  loss_fn=LOSS_FNS["acc"])
    torch.testing.assert_close(torch.from_numpy(ref["true_losses"]),
                               mine.true_losses(preds))


def test_coda_prefilter_and_ablation_parity():
    """Prefiltered candidates + no-diag-prior ablation match the
    reference's trajectories too."""
    from coda_amd.datasets import Dataset
    from coda_amd import CODA

    ref = _golden("coda_prefilter_ablation", 6, 250, 4, 6)
    preds, labels = _mk(seed=6, H=6, N=250, C=4)

    random.seed(3); torch.manual_seed(3)
    mine = CODA(Dataset.from_tensors(preds, labels, "cpu"),
                prefilter_n=40, disable_diag_prior=True)

    for m in range(3):
        ir = int(ref["idx"][m])
        random.seed(50 + m)
        im, qm = mine.get_next_item_to_label()
        assert ir == int(im), (m, ir, int(im))
        y = int(labels[ir])
        mine.add_label(int(im), y, qm)


def test_baseline_acquisition_distributions_parity():
    """ActiveTesting / VMA acquisition DISTRIBUTIONS equal the
    reference's (selection draws consume the same seeded RNG, so equal
    distributions => equal trajectories)."""
    from coda_amd.datasets import Dataset
    from coda_amd.baselines import ActiveTesting, VMA
    from coda_amd.options import LOSS_FNS

    ref = _golden("baseline_acquisition", 5, 120, 4, 7)
    preds, labels = _mk(seed=7, H=5, N=120, C=4)
    ds = Dataset.from_tensors(preds, labels, "cpu")

    # ActiveTesting: same normalized scores over the unlabeled pool
    mat = ActiveTesting(ds, LOSS_FNS["acc"])
    pi_y = preds.mean(0)
    cls = preds.argmax(2)
    y_star = pi_y[torch.arange(120), cls]
    ref_scores = (1 - y_star).sum(0)
    ref_scores = ref_scores / ref_scores.sum()
    mine_scores = mat._acq_mass / mat._acq_mass.sum()
    torch.testing.assert_close(mine_scores, ref_scores, rtol=1e-5,
                               atol=1e-7)
    # identical seeded draw
    ri, rq = int(ref["at"][0]), float(ref["at"][1])
    random.seed(11)
    mi, mq = mat.get_next_item_to_label()
    assert ri == int(mi) and abs(rq - mq) < 1e-6

    # VMA: same pairwise-difference masses (ours via the sorted identity)
    mv = VMA(ds, LOSS_FNS["acc"])
    ri, rq = int(ref["vma"][0]), float(ref["vma"][1])
    random.seed(12)
    mi, mq = mv.get_next_item_to_label()
    assert ri == int(mi) and abs(rq - mq) < 1e-6
