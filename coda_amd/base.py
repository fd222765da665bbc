"""ModelSelector interface.

The three-method contract every selection algorithm implements, plus the
`stochastic` attribute the harness reads to decide whether further seeds are
needed (reference: coda/base.py:1-16, main.py:105,164-168).
"""
from __future__ import annotations


class ModelSelector:
    """Abstract active-model-selection algorithm.

    Attributes:
        stochastic: True if the algorithm made any random choice so far, in
            which case the harness runs additional seeds.
        supports_batch: True if the algorithm hands out a batch of points
            per acquisition (get_next_items_to_label / add_labels); the
            harness labels the others one point at a time.
    """

    stochastic: bool = False
    # True where get_next_items_to_label(k) / add_labels exist
    supports_batch: bool = False

    def get_next_item_to_label(self):
        """Pick the next unlabeled point to send to the oracle.

        Returns:
            (index, selection_probability_or_score)
        """
        raise NotImplementedError

    def add_label(self, chosen_idx, true_class, selection_prob):
        """Incorporate an oracle label for a point."""
        raise NotImplementedError

    def get_best_model_prediction(self):
        """Return the index of the currently-believed-best model."""
        raise NotImplementedError
