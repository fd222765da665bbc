"""Record what the upstream reference (justinkay/coda, pure PyTorch) computes
on the parity tests' synthetic tasks into tests/golden/reference_parity/.

tests/test_reference_parity.py and tests/test_reference_parity_long.py
replay these recordings instead of importing the reference, so the suite
needs nothing outside the repository. Only numbers the reference produced
while running are stored (scores, selections, posteriors); none of its code.

Every recording also stores the task parameters and seeds it was made
with; the tests assert that theirs are the same, so a change on one side
only fails loudly. Re-record after changing a task shape or seed in a test:

    python oracle/record_parity_golden.py --reference /path/to/coda-checkout

The reference runs on CPU; the full set takes a few minutes.
"""
from __future__ import annotations

import argparse
import contextlib
import io
import os
import random
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(REPO, "tests", "golden", "reference_parity")


class _RefDS:
    pass


def _task(H, N, C, seed):
    from coda_amd.datasets import make_synthetic_task
    preds, labels = make_synthetic_task(H=H, N=N, C=C, seed=seed)
    rds = _RefDS()
    rds.preds, rds.labels = preds.clone(), labels.clone()
    rds.device = torch.device("cpu")
    return rds, preds, labels


def _np(t):
    return t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)


def _save(name, task, **arrays):
    os.makedirs(OUT, exist_ok=True)
    H, N, C, seed = task
    path = os.path.join(OUT, name + ".npz")
    np.savez_compressed(path, task=np.array([H, N, C, seed], np.int64),
                        **{k: _np(v) for k, v in arrays.items()})
    print(f"{path}: {os.path.getsize(path)} bytes")


def _quiet():
    return contextlib.redirect_stderr(io.StringIO())


def ref_select(q_vals, candidates, seed):
    """The reference's greedy selection rule applied to a given EIG
    vector, with seeded tie randomization (same helper as the tests)."""
    random.seed(seed)
    best = q_vals.max()
    ties = torch.isclose(q_vals, best, rtol=1e-8)
    if int(ties.sum()) > 1:
        pos = random.choice(torch.nonzero(ties, as_tuple=True)[0].tolist())
    else:
        pos = int(q_vals.argmax())
    return int(list(candidates)[pos]), float(q_vals[pos])


# -- tests/test_reference_parity.py ---------------------------------------
def short_coda(ref_coda):
    task = (8, 300, 5, 0)
    rds, _, labels = _task(*task)
    random.seed(0); torch.manual_seed(0)
    ref = ref_coda.CODA(rds)
    pbest0 = ref.get_pbest().reshape(-1).clone()
    idx, q, best = [], [], []
    for m in range(5):
        random.seed(100 + m)
        with _quiet():
            ir, qr = ref.get_next_item_to_label()
        ref.add_label(int(ir), int(labels[int(ir)]), qr)
        idx.append(int(ir)); q.append(float(qr))
        best.append(int(ref.get_best_model_prediction()))
    _save("coda_trajectory", task, pbest0=pbest0, idx=np.array(idx),
          q=np.array(q, np.float64), best=np.array(best))


def short_modelpicker(ref_mp):
    task = (8, 300, 5, 3)
    rds, _, _ = _task(*task)
    ref = ref_mp.ModelPicker(rds, epsilon=0.45)
    preds_u = ref.dataset.preds.argmax(2).transpose(0, 1)[:60]
    e_ref = ref.compute_entropies(preds_u, ref.posterior, ref.H, ref.C,
                                  ref.gamma)
    _save("modelpicker_entropy", task, entropies=e_ref)


def short_oracle(RefOracle, REF_LOSS):
    task = (8, 300, 5, 4)
    rds, preds, _ = _task(*task)
    ref = RefOracle(rds, loss_fn=REF_LOSS["acc"])
    _save("oracle_losses", task, true_losses=ref.true_losses(preds))


def short_prefilter(ref_coda):
    task = (6, 250, 4, 6)
    rds, _, labels = _task(*task)
    random.seed(3); torch.manual_seed(3)
    ref = ref_coda.CODA(rds, prefilter_n=40, disable_diag_prior=True)
    idx, q = [], []
    for m in range(3):
        random.seed(50 + m)
        with _quiet():
            ir, qr = ref.get_next_item_to_label()
        ref.add_label(int(ir), int(labels[int(ir)]), qr)
        idx.append(int(ir)); q.append(float(qr))
    _save("coda_prefilter_ablation", task, idx=np.array(idx),
          q=np.array(q, np.float64))


def short_baselines(RefAT, RefVMA, REF_LOSS):
    task = (5, 120, 4, 7)
    rds, _, _ = _task(*task)
    rat = RefAT(rds, REF_LOSS["acc"])
    random.seed(11)
    ai, aq = rat.get_next_item_to_label()
    rv = RefVMA(rds, REF_LOSS["acc"])
    random.seed(12)
    vi, vq = rv.get_next_item_to_label()
    _save("baseline_acquisition", task,
          at=np.array([int(ai), float(aq)], np.float64),
          vma=np.array([int(vi), float(vq)], np.float64))


# -- tests/test_reference_parity_long.py ----------------------------------
def _teacher_forced_eig(ref, labels, steps, seed_base, pbest_every):
    """Run the reference along its own seeded selections; returns the EIG
    vector and candidate list of every step (flattened) and its P(best)
    every `pbest_every` steps (0: only after the last step)."""
    qs, cands, lens, pbests = [], [], [], []
    for m in range(steps):
        with _quiet():
            q_r, cand_r = ref.eig_batched()
        qs.append(_np(q_r).astype(np.float32))
        cands.append(np.asarray(list(cand_r), np.int32))
        lens.append(len(cands[-1]))
        idx, q = ref_select(q_r, cand_r, seed=seed_base + m)
        ref.add_label(idx, int(labels[idx]), q)
        if pbest_every and (m + 1) % pbest_every == 0:
            pbests.append(_np(ref.get_pbest().reshape(-1)).copy())
    if not pbest_every:
        pbests.append(_np(ref.get_pbest().reshape(-1)).copy())
    return dict(q_flat=np.concatenate(qs), cand_flat=np.concatenate(cands),
                lens=np.array(lens, np.int64), pbest=np.stack(pbests))


def long_coda(ref_coda):
    for H, N, C, steps in ((8, 300, 5, 100), (6, 400, 2, 100),
                           (10, 120, 126, 100)):
        task = (H, N, C, H + C)
        rds, _, labels = _task(*task)
        random.seed(0); torch.manual_seed(0)
        ref = ref_coda.CODA(rds)
        _save(f"coda_100step_{H}_{N}_{C}", task,
              **_teacher_forced_eig(ref, labels, steps, 1000, 10))


def long_hyper(ref_coda):
    task = (6, 200, 4, 33)
    for i, kwargs in enumerate(({"learning_rate": 0.1},
                                {"alpha": 0.5},
                                {"multiplier": 1.0},
                                {"learning_rate": 0.05, "alpha": 0.8,
                                 "multiplier": 4.0})):
        rds, _, labels = _task(*task)
        random.seed(0); torch.manual_seed(0)
        ref = ref_coda.CODA(rds, **kwargs)
        _save(f"coda_hyper_{i}", task,
              **_teacher_forced_eig(ref, labels, 25, 500, 0))


def long_iid(ref_iid, REF_LOSS):
    task = (7, 250, 6, 21)
    rds, _, labels = _task(*task)
    ref = ref_iid.IID(rds, REF_LOSS["acc"])
    idx, q, risk = [], [], []
    for m in range(100):
        random.seed(1000 + m)
        ir, qr = ref.get_next_item_to_label()
        ref.add_label(int(ir), int(labels[int(ir)]), qr)
        idx.append(int(ir)); q.append(float(qr))
        risk.append(_np(ref.get_risk_estimates()).copy())
    _save("iid_100step", task, idx=np.array(idx),
          q=np.array(q, np.float64), risk=np.stack(risk))


def long_baselines(mods, REF_LOSS):
    task = (7, 250, 6, 21)
    for method in ("uncertainty", "activetesting", "vma", "model_picker"):
        rds, _, labels = _task(*task)
        if method == "uncertainty":
            ref = mods["unc"].Uncertainty(rds, REF_LOSS["acc"])
        elif method == "activetesting":
            ref = mods["at"].ActiveTesting(rds, REF_LOSS["acc"])
        elif method == "vma":
            ref = mods["vma"].VMA(rds, REF_LOSS["acc"])
        else:
            ref = mods["mp"].ModelPicker(rds, epsilon=0.38)
        idx, q, state = [], [], []
        for m in range(100):
            random.seed(1000 + m); torch.manual_seed(1000 + m)
            with _quiet():
                ir, qr = ref.get_next_item_to_label()
            ref.add_label(int(ir), int(labels[int(ir)]), qr)
            idx.append(int(ir)); q.append(float(qr))
            if method == "model_picker":
                state.append(_np(ref.posterior).copy())
            elif method in ("activetesting", "vma"):
                state.append(_np(ref.get_lure_risks_and_vars()[0]).copy())
        extra = {"state": np.stack(state)} if state else {}
        _save(f"baseline_100step_{method}", task, idx=np.array(idx),
              q=np.array(q, np.float64), **extra)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--reference", required=True,
                    help="checkout of the upstream reference (the "
                         "directory that holds its coda/ package)")
    args = ap.parse_args()
    sys.path.insert(0, REPO)
    sys.path.insert(0, os.path.abspath(args.reference))
    import coda.coda as ref_coda
    import coda.baselines.iid as ref_iid
    import coda.baselines.uncertainty as ref_unc
    import coda.baselines.activetesting as ref_at
    import coda.baselines.vma as ref_vma
    import coda.baselines.modelpicker as ref_mp
    from coda.oracle import Oracle as RefOracle
    from coda.options import LOSS_FNS as REF_LOSS

    short_coda(ref_coda)
    short_modelpicker(ref_mp)
    short_oracle(RefOracle, REF_LOSS)
    short_prefilter(ref_coda)
    short_baselines(ref_at.ActiveTesting, ref_vma.VMA, REF_LOSS)
    long_iid(ref_iid, REF_LOSS)
    long_baselines(dict(unc=ref_unc, at=ref_at, vma=ref_vma, mp=ref_mp),
                   REF_LOSS)
    long_hyper(ref_coda)
    long_coda(ref_coda)


if __name__ == "__main__":
    main()
