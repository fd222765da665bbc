"""Batch acquisition's cost at the bench.py headline shape (GPU): the
captured step with batch outputs off / flat / distinct (host clock per
step, device events per graph replay), torch.topk(qbuf, 1024) as the
alternative it replaces, and the one-off build of the pattern groups.
Prints one JSON line per figure (profiles/batch_acq.md).

    python scripts/batch_acq_probe.py
"""
import json
import os
import random
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
from coda_amd import CODA, Oracle  # noqa: E402
from coda_amd.datasets import Dataset, STORAGE_DTYPES  # noqa: E402
from coda_amd.options import LOSS_FNS  # noqa: E402
from coda_amd.ops.reference import group_rows  # noqa: E402

dev = torch.device("cuda", 0)
preds, labels = bench.synth_preds(list(range(bench.H_MODELS)),
                                  bench.N_PER_GPU, bench.C_CLASSES, dev,
                                  dtype=STORAGE_DTYPES[bench.STORAGE])
ds = Dataset.from_tensors(preds, labels, dev, shard=None)
ds.total_models = bench.H_MODELS
oracle = Oracle(ds, LOSS_FNS["acc"])
random.seed(0)
torch.manual_seed(0)
with bench.reproducible_setup():
    sel = CODA(ds, prefilter_n=bench.PREFILTER_N, chunk_size=bench.CHUNK)


def one_step():
    idx, q = sel.get_next_item_to_label()
    sel.add_label(idx, oracle(int(idx)), q)
    return sel.get_best_model_prediction()


def timed(steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        one_step()
    torch.cuda.synchronize()
    return 1000.0 * (time.perf_counter() - t0) / steps


def replay_us(n=300):
    """Device time of one replay of the merged label+acquire graph (same
    label replayed: the work does not depend on which)."""
    g = sel._label_graph
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), \
        torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        g.replay()
    b.record()
    torch.cuda.synchronize()
    return 1000.0 * a.elapsed_time(b) / n


for _ in range(50):
    one_step()
acq = sel._pair_acq
B = acq.qbuf.numel()
print(json.dumps({"B": B, "merged": sel._merged_acq,
                  "cache": acq.cache is not None}), flush=True)

t0 = time.perf_counter()
g, G = group_rows(acq.cls_rows)
torch.cuda.synchronize()
t1 = time.perf_counter()
g, G = group_rows(acq.cls_rows)
torch.cuda.synchronize()
t2 = time.perf_counter()
print(json.dumps({"group_build_ms_first": 1000 * (t1 - t0),
                  "group_build_ms_second": 1000 * (t2 - t1),
                  "n_groups": G, "n_groups_over_B": G / B}), flush=True)

STEPS = 300
res = {}
for rnd in range(2):
    for mode in ("off", "flat", "distinct"):
        if mode == "off":
            acq.topk_distinct = None
        else:
            acq.enable_topk(mode == "distinct")
        sel._drop_graphs()
        for _ in range(20):
            one_step()          # re-captures, warms
        assert sel._label_graph is not None
        assert len(acq.topk_args()) == {"off": 0, "flat": 1,
                                        "distinct": 3}[mode]
        ms = timed(STEPS)
        res.setdefault(mode, []).append(ms)
        print(json.dumps({"mode": mode, "round": rnd,
                          "ms_per_step": ms}), flush=True)

# device time of the replay alone: replaying the same label again only
# moves the posterior, the kernels' work is the same
for mode in ("off", "flat", "distinct", "off"):
    if mode == "off":
        acq.topk_distinct = None
    else:
        acq.enable_topk(mode == "distinct")
    sel._drop_graphs()
    for _ in range(5):
        one_step()
    replay_us(50)
    print(json.dumps({"mode": mode, "replay_us": replay_us()}), flush=True)

# the alternative: torch.topk on qbuf after the replay
torch.cuda.synchronize()
for _ in range(20):
    torch.topk(acq.qbuf, 1024)
a, b = torch.cuda.Event(enable_timing=True), \
    torch.cuda.Event(enable_timing=True)
a.record()
for _ in range(300):
    torch.topk(acq.qbuf, 1024)
b.record()
torch.cuda.synchronize()
print(json.dumps({"torch_topk_1024_us": 1000.0 * a.elapsed_time(b) / 300}),
      flush=True)
print(json.dumps({m: [round(v, 4) for v in vs] for m, vs in res.items()}))
