"""ModelPicker (Karimi et al. 2021 style) Bayesian posterior baseline.

Reference parity: coda/baselines/modelpicker.py:5-110 - posterior over
"which model is correct" with noise parameter epsilon; picks the unlabeled
point minimizing expected posterior entropy; per-task tuned epsilon table.

The reference loops over classes in compute_entropies (modelpicker.py:74-86);
here the class loop is a single batched tensor expression. Entropies are in
log2 (behaviorally load-bearing).

That dense expression carries (Nu, C, H) temporaries and cannot run at
full-pool scale. entropy_impl="sparse" scores the whole pool through
ops.modelpicker_dev instead: a class no model predicts on a point leaves
the posterior unchanged, a class that is hit changes the entropy by a
closed form in two sums over the models predicting it, so a point costs
O(H) and a step is one pass over a static (N, H) int16 structure.
"""
from __future__ import annotations

import torch

from ..base import ModelSelector
from .. import ops


TASK_EPS = {
    # from the original ModelPicker paper
    "imagenet_v2_matched-frequency": 0.48,
    "cifar10_4070": 0.47,
    "cifar10_5592": 0.47,
    "pacs": 0.45,
    "glue/cola": 0.45,
    "glue/mnli": 0.43,
    "glue/qnli": 0.44,
    "glue/qqp": 0.47,
    "glue/rte": 0.39,
    "glue/sst2": 0.36,
    # from the reference's reproduction of the grid search
    "real_clipart": 0.42,
    "real_painting": 0.35,
    "real_sketch": 0.45,
    "sketch_real": 0.35,
    "sketch_clipart": 0.35,
    "sketch_painting": 0.37,
    "clipart_painting": 0.45,
    "clipart_real": 0.45,
    "clipart_sketch": 0.43,
    "painting_sketch": 0.39,
    "painting_real": 0.44,
    "painting_clipart": 0.39,
    "iwildcam": 0.49,
    "civilcomments": 0.46,
    "fmow": 0.44,
    "camelyon": 0.47,
}


class ModelPicker(ModelSelector):
    ENTROPY_IMPLS = ("auto", "dense", "sparse")
    # "auto" goes sparse once one dense fp32 (N, C, H) temporary is 1 GiB
    SPARSE_MIN_ELEMS = 2 ** 28

    def __init__(self, dataset, epsilon: float = 0.46,
                 entropy_impl: str = "auto"):
        self.dataset = dataset
        self.device = dataset.preds.device
        self.Hl, self.N, self.C = dataset.preds.shape
        self.H = getattr(dataset, "total_models", self.Hl)

        self.classes_nh = ops.pred_classes(dataset.preds).t().contiguous()  # (N, Hl)
        self._setup(epsilon, entropy_impl)

    @classmethod
    def from_classes(cls, classes_nh: torch.Tensor, num_classes: int,
                     epsilon: float = 0.46, entropy_impl: str = "auto"):
        """A selector over cached (N, H) argmax classes alone: the
        selection rule reads nothing else of the pool, and a million-point
        pool of class ids fits where its (H, N, C) predictions do not."""
        self = cls.__new__(cls)
        self.dataset = None
        self.device = classes_nh.device
        self.N, self.Hl = classes_nh.shape
        self.C = int(num_classes)
        self.H = self.Hl
        self.classes_nh = classes_nh.long().contiguous()
        self._setup(epsilon, entropy_impl)
        return self

    def _setup(self, epsilon, entropy_impl):
        self._disagreement_mask = ops.disagreement_mask(self.classes_nh.t())

        self.epsilon = float(epsilon)
        self.gamma = (1.0 - self.epsilon) / self.epsilon
        self.posterior = torch.ones(self.Hl, device=self.device) / self.H

        self.d_l_idxs = []
        self.d_l_ys = []
        self.d_u_idxs = list(range(self.N))
        self.correct_counts = torch.zeros(self.Hl, dtype=torch.long,
                                          device=self.device)
        self.stochastic = True

        self.entropy_impl = self._resolve_entropy_impl(entropy_impl)
        if self.entropy_impl == "sparse":
            self._struct = ops.modelpicker_build(self.classes_nh)
            self._rebuild_unlabeled_mask()

    def _resolve_entropy_impl(self, impl: str) -> str:
        if impl not in self.ENTROPY_IMPLS:
            raise ValueError(f"entropy_impl must be one of "
                             f"{self.ENTROPY_IMPLS}, got {impl!r}")
        fits = (self.Hl == self.H and self.H <= ops.MODELPICKER_MAX_H
                and self.C <= ops.MODELPICKER_MAX_C)
        if impl == "sparse" and not fits:
            raise ValueError(
                "entropy_impl='sparse' needs an unsharded pool with "
                f"H <= {ops.MODELPICKER_MAX_H} and C <= "
                f"{ops.MODELPICKER_MAX_C}; got Hl={self.Hl}, H={self.H}, "
                f"C={self.C}")
        if impl != "auto":
            return impl
        big = self.N * self.C * self.H > self.SPARSE_MIN_ELEMS
        on_hip = self.classes_nh.is_cuda and ops.hip_available()
        return "sparse" if (fits and big and on_hip) else "dense"

    def _rebuild_unlabeled_mask(self):
        """(N,) device mask of unlabeled points from d_u_idxs (init and
        checkpoint load; add_label keeps it current after that)."""
        unl = torch.zeros(self.N, dtype=torch.bool)
        unl[torch.as_tensor(self.d_u_idxs, dtype=torch.long)] = True
        self._unlabeled = unl.to(self.device)

    def sparse_entropies(self):
        """Expected posterior entropy of every pool point, (N,) fp32,
        +inf on inactive points (labeled, or agreed-upon while a
        disagreement point is left): e0 + dev / C."""
        cand = self._unlabeled & self._disagreement_mask
        active = torch.where(cand.any(), cand, self._unlabeled)
        dev = ops.modelpicker_dev(self._struct, self.posterior, self.gamma,
                                  active)
        p = (self.posterior / self.posterior.sum()).clamp(min=1e-12)
        e0 = -(p * torch.log2(p)).sum()
        return e0 + dev / self.C

    def get_next_item_to_label(self):
        if self.entropy_impl == "sparse":
            entropies = self.sparse_entropies()
            min_val = torch.min(entropies)
            loc = torch.nonzero(entropies == min_val).flatten()
            i_star = int(loc[torch.randint(len(loc), (1,))].item())
            return i_star, 1.0 / float(len(self.d_u_idxs))
        preds_u = self.classes_nh[self.d_u_idxs]          # (Nu, Hl)
        mask = self._disagreement_mask[self.d_u_idxs]
        entropies = self.compute_entropies(preds_u, self.posterior,
                                           self.Hl, self.C, self.gamma)
        if mask.any():
            entropies = entropies.clone()
            entropies[~mask] = float("inf")
        min_val = torch.min(entropies)
        loc = torch.nonzero(entropies == min_val).flatten()
        i_star = int(loc[torch.randint(len(loc), (1,))].item())
        return self.d_u_idxs[i_star], 1.0 / float(len(self.d_u_idxs))

    def compute_entropies(self, predictions_unlabeled, posterior,
                          num_models, num_classes, gamma):
        """Expected posterior log2-entropy per point, averaged over classes.

        Batched over the class axis: agreements (Nu, C, H) one-hot of each
        model's class; hypothetical posterior ~ posterior * gamma^agree.
        """
        agree = (predictions_unlabeled.unsqueeze(1) ==
                 torch.arange(num_classes, device=self.device).view(1, -1, 1))
        new_post = posterior.view(1, 1, -1) * torch.where(
            agree, torch.as_tensor(gamma, dtype=posterior.dtype,
                                   device=self.device),
            torch.ones((), dtype=posterior.dtype, device=self.device))
        new_post = new_post / new_post.sum(dim=-1, keepdim=True)
        p = new_post.clamp(min=1e-12)
        conditional = -(p * torch.log2(p)).sum(dim=-1)    # (Nu, C)
        return conditional.mean(dim=1)                    # (Nu,)

    def add_label(self, chosen_idx, true_class, selection_prob=None):
        chosen_idx = int(chosen_idx)
        self.d_u_idxs.remove(chosen_idx)
        self.d_l_idxs.append(chosen_idx)
        self.d_l_ys.append(true_class)
        if self.entropy_impl == "sparse":
            self._unlabeled[chosen_idx] = False
        preds = self.classes_nh[chosen_idx]               # (Hl,)
        self.correct_counts += (preds == true_class).long()
        agreements = (preds == true_class).float()
        next_post = self.posterior * (self.gamma ** agreements)
        self.posterior = next_post / next_post.sum()

    def get_best_model_prediction(self):
        if len(self.d_l_idxs) == 0:
            return int(torch.randint(self.Hl, (1,), device=self.device).item())
        max_acc = torch.max(self.correct_counts)
        ties = torch.nonzero(self.correct_counts == max_acc).flatten()
        return int(ties[torch.randint(len(ties), (1,),
                                      device=self.device)].item())
