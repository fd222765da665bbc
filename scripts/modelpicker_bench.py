"""Time ModelPicker steps: the hit-sparse HIP entropy kernel at full-pool
scale, and dense against sparse where dense still fits.

The selection rule reads only the cached (N, H) argmax classes, so the
pools are seeded class-id pools fed through ModelPicker.from_classes -
no (H, N, C) prediction tensor is materialised. Each point has a true
class; a model predicts it with probability --agree and a uniform class
otherwise.

  sparse   ms per get_next_item_to_label + add_label at --n and --big-n
           points (the step ends in the pick's .item(), a device
           synchronise), the one-off structure build, and the
           modelpicker_dev call alone under device events
  dense    against sparse at the largest N whose dense fp32 (N, C, H)
           temporaries stay under --dense-gb each; the two alternate in
           rounds within this process, and their score vectors are
           compared at that size

Prints one JSON line. Needs a ROCm device: there is no CPU fallback.

    python scripts/modelpicker_bench.py
    # kernel time, in a run of its own:
    rocprofv3 --kernel-trace --stats --output-format csv -d prof -- \
        python scripts/modelpicker_bench.py --steps 20 --skip-dense
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from coda_amd import ops  # noqa: E402
from coda_amd.baselines import ModelPicker  # noqa: E402


def make_classes(N, H, C, agree, device, seed=0, chunk=1 << 16):
    """(N, H) int64 classes and (N,) true classes, built on the device."""
    g = torch.Generator(device=device).manual_seed(seed)
    cls = torch.empty(N, H, dtype=torch.long, device=device)
    true = torch.randint(0, C, (N,), generator=g, device=device)
    for n0 in range(0, N, chunk):
        t = true[n0:n0 + chunk].unsqueeze(1)
        n = t.shape[0]
        keep = torch.rand(n, H, generator=g, device=device) < agree
        unif = torch.randint(0, C, (n, H), generator=g, device=device)
        cls[n0:n0 + chunk] = torch.where(keep, t.expand(n, H), unif)
    return cls, true


def time_steps(sel, labels, steps, warmup):
    """ms per get_next_item_to_label + add_label (host clock; the pick's
    .item() synchronises every step)."""
    torch.manual_seed(0)
    for _ in range(warmup):
        idx, q = sel.get_next_item_to_label()
        sel.add_label(idx, labels[idx], q)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        idx, q = sel.get_next_item_to_label()
        sel.add_label(idx, labels[idx], q)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / steps


def time_dev_call(sel, reps):
    """ms per ops.modelpicker_dev call (prologue + kernel), device events."""
    active = sel._unlabeled & sel._disagreement_mask
    for _ in range(5):
        ops.modelpicker_dev(sel._struct, sel.posterior, sel.gamma, active)
    a, b = (torch.cuda.Event(enable_timing=True) for _ in range(2))
    a.record()
    for _ in range(reps):
        ops.modelpicker_dev(sel._struct, sel.posterior, sel.gamma, active)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def sparse_case(N, H, C, args, device):
    cls, true = make_classes(N, H, C, args.agree, device)
    labels = true.cpu().tolist()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    sel = ModelPicker.from_classes(cls, C, epsilon=args.eps,
                                   entropy_impl="sparse")
    torch.cuda.synchronize()
    build_ms = (time.perf_counter() - t0) * 1e3
    step_ms = time_steps(sel, labels, args.steps, args.warmup)
    dev_ms = time_dev_call(sel, 200)
    return {"N": N, "H": H, "C": C, "init_ms": round(build_ms, 1),
            "step_ms": round(step_ms, 4), "dev_call_ms": round(dev_ms, 4),
            "struct_mb": round(N * H * 2 / 1e6, 1),
            "distinct_classes_per_point":
                round(float(sel._struct.nseg.float().mean()), 1)}


def dense_vs_sparse(H, C, args, device):
    N = int(args.dense_gb * 1e9 / 4 / (C * H))
    cls, true = make_classes(N, H, C, args.agree, device, seed=1)
    labels = true.cpu().tolist()
    out = {"N": N, "H": H, "C": C,
           "dense_temp_gb": round(N * C * H * 4 / 1e9, 2)}
    # same scores first: faster and different is not faster
    d = ModelPicker.from_classes(cls, C, epsilon=args.eps,
                                 entropy_impl="dense")
    s = ModelPicker.from_classes(cls, C, epsilon=args.eps,
                                 entropy_impl="sparse")
    for sel in (d, s):                     # a few labels: non-uniform posterior
        for idx in range(8):
            sel.add_label(idx, labels[idx], 1.0)
    ent_d = d.compute_entropies(d.classes_nh[d.d_u_idxs], d.posterior, d.Hl,
                                d.C, d.gamma)
    ent_s = s.sparse_entropies()[d.d_u_idxs]
    fin = torch.isfinite(ent_s)
    out["max_abs_score_diff"] = float((ent_d[fin] - ent_s[fin]).abs().max())
    out["score_spread"] = float(ent_d[fin].max() - ent_d[fin].min())
    dense_ms, sparse_ms = [], []
    for _ in range(args.rounds):
        dense_ms.append(time_steps(d, labels, args.dense_steps, 2))
        sparse_ms.append(time_steps(s, labels, args.dense_steps, 2))
    out["dense_step_ms_rounds"] = [round(x, 3) for x in dense_ms]
    out["sparse_step_ms_rounds"] = [round(x, 4) for x in sparse_ms]
    out["peak_mem_gb"] = round(torch.cuda.max_memory_allocated() / 1e9, 2)
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__,
                                 formatter_class=argparse.RawTextHelpFormatter)
    ap.add_argument("--h", type=int, default=128)
    ap.add_argument("--c", type=int, default=1000)
    ap.add_argument("--n", type=int, default=50000)
    ap.add_argument("--big-n", type=int, default=1000000)
    ap.add_argument("--agree", type=float, default=0.6)
    ap.add_argument("--eps", type=float, default=0.46)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--dense-gb", type=float, default=2.0)
    ap.add_argument("--dense-steps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--skip-dense", action="store_true")
    args = ap.parse_args(argv)

    if not torch.cuda.is_available():
        raise SystemExit("modelpicker_bench needs a ROCm device")
    device = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0), "eps": args.eps,
           "agree": args.agree, "steps": args.steps,
           "sparse": [sparse_case(n, args.h, args.c, args, device)
                      for n in (args.n, args.big_n) if n > 0]}
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    if not args.skip_dense:
        res["dense_vs_sparse"] = dense_vs_sparse(args.h, args.c, args, device)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
