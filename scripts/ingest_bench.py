"""Time pool ingest: legacy .pt route vs sharded fused-ingest route.

legacy: Dataset("<task>.pt", storage_dtype=S, stream_chunk_mb=M), then
        ops.init_model_stats, then the class-major mirror permute - what a
        selector needs from the pool before its first step.
shards: Dataset("<task>.shards", storage_dtype=S, stream_chunk_mb=M) -
        the same three products out of the fused ingest kernel.

Both read the same seeded pool, stored on disk in --dtype. Routes
alternate within one process; each timed window ends in a device
synchronize. Prints one JSON line with per-route wall times, host-wire
bytes and the ingest kernel's byte floor (computed from shapes), and
checks that both routes produce the same pool, classes and mirror.

logits: (--kind both | logits) Dataset("<task>_logits.shards", ...) - the
        same seeded pool stored as LOGITS (format 2), whose temperature
        softmax the ingest kernel takes in the same pass. --kind both
        alternates it with the probability shards of the same shape and
        dtype, and reports the host wire of the session: a pinned
        chunk-sized host->device copy and the staging memcpy into it.

    python scripts/ingest_bench.py --h 16 --n 20000 --c 1000 --reps 3
    python scripts/ingest_bench.py --kind both --dtype fp16 --storage fp16
    # kernel time, in a run of its own:
    rocprofv3 --kernel-trace --stats --output-format csv -d prof -- \
        python scripts/ingest_bench.py --route shards --reps 1 --warmup 0
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import tempfile
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from coda_amd import ops  # noqa: E402
from coda_amd.datasets import (Dataset, STORAGE_DTYPES,  # noqa: E402
                               write_sharded_task)


def make_pool(work, H, N, C, dtype, per_shard, seed=0, with_logits=False):
    """Seeded softmax pool, written model by model (no fp32 full copy);
    with_logits also writes the logits themselves as a format-2 task."""
    dt = STORAGE_DTYPES[dtype]
    g = torch.Generator().manual_seed(seed)
    full = torch.empty((H, N, C), dtype=dt)
    raw = torch.empty((H, N, C), dtype=dt) if with_logits else None
    for h in range(H):
        logits = torch.randn(N, C, generator=g)
        logits[torch.arange(N), torch.randint(0, C, (N,), generator=g)] += 3.0
        full[h] = torch.softmax(logits, -1).to(dt)
        if with_logits:
            raw[h] = logits.to(dt)
    pt = os.path.join(work, "pool.pt")
    torch.save(full, pt)
    sh = os.path.join(work, "pool.shards")
    write_sharded_task(sh, full, dtype, per_shard)
    lg = None
    if with_logits:
        lg = os.path.join(work, "pool_logits.shards")
        write_sharded_task(lg, raw, dtype, per_shard, kind="logits")
    return pt, sh, lg


def measure_wire(dev, nbytes, reps=5):
    """Host wire of this session for one chunk of nbytes: the pinned
    host->device copy, and the pageable->pinned staging memcpy before it
    (GB/s, medians)."""
    src = torch.empty(nbytes, dtype=torch.uint8).random_(0, 255)
    pinned = torch.empty(nbytes, dtype=torch.uint8).pin_memory()
    stage, h2d = [], []
    for _ in range(reps + 1):
        t0 = time.perf_counter()
        pinned.copy_(src)
        t1 = time.perf_counter()
        torch.cuda.synchronize(dev)
        t2 = time.perf_counter()
        out = pinned.to(dev, non_blocking=True)
        torch.cuda.synchronize(dev)
        t3 = time.perf_counter()
        del out
        stage.append(nbytes / (t1 - t0) / 1e9)
        h2d.append(nbytes / (t3 - t2) / 1e9)
    med = lambda v: sorted(v[1:])[len(v[1:]) // 2]  # noqa: E731
    return {"chunk_bytes": nbytes, "h2d_gbps": med(h2d),
            "stage_gbps": med(stage)}


def run_legacy(pt, dev, storage, chunk_mb):
    ds = Dataset(pt, dev, storage_dtype=storage, stream_chunk_mb=chunk_mb)
    classes, ens = ops.init_model_stats(ds.preds)
    mirror = ds.preds.permute(0, 2, 1).contiguous()
    return ds.preds, classes, ens, mirror


def run_shards(sh, dev, storage, chunk_mb):
    ds = Dataset(sh, dev, storage_dtype=storage, stream_chunk_mb=chunk_mb)
    st = ds.init_stats
    return ds.preds, st["classes"], st["ens_sum"], st["preds_t"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--h", type=int, default=16)
    ap.add_argument("--n", type=int, default=20000)
    ap.add_argument("--c", type=int, default=1000)
    ap.add_argument("--dtype", default="fp8", choices=sorted(STORAGE_DTYPES))
    ap.add_argument("--storage", default="fp8",
                    choices=sorted(STORAGE_DTYPES))
    ap.add_argument("--chunk-mb", type=int, default=64)
    ap.add_argument("--models-per-shard", type=int, default=4)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--route", default="both",
                    choices=["both", "legacy", "shards"])
    ap.add_argument("--kind", default="probs",
                    choices=["probs", "logits", "both"],
                    help="probs: the routes above; logits: the sharded "
                         "route on a logits task; both: probability shards "
                         "and logits shards alternating")
    ap.add_argument("--work-dir", default=None)
    args = ap.parse_args()
    if args.kind != "probs" and args.dtype == "fp8":
        ap.error("--kind logits/both needs --dtype fp32, fp16 or bf16")

    assert torch.cuda.is_available(), "ingest_bench needs a GPU"
    assert ops.hip_available(), "HIP extension not built"
    dev = torch.device("cuda:0")
    H, N, C = args.h, args.n, args.c
    if args.kind == "both":
        routes = ["shards", "logits"]
    elif args.kind == "logits":
        routes = ["logits"]
    else:
        routes = (["legacy", "shards"] if args.route == "both"
                  else [args.route])
    fns = {"legacy": run_legacy, "shards": run_shards, "logits": run_shards}

    with tempfile.TemporaryDirectory(dir=args.work_dir) as work:
        pt, sh, lg = make_pool(work, H, N, C, args.dtype,
                               args.models_per_shard,
                               with_logits=args.kind != "probs")
        paths = {"legacy": pt, "shards": sh, "logits": lg}
        times = {r: [] for r in routes}
        outs = {}
        for rep in range(args.warmup + args.reps):
            for r in routes:            # alternate the routes
                outs.pop(r, None)
                torch.cuda.synchronize(dev)
                t0 = time.perf_counter()
                out = fns[r](paths[r], dev, args.storage, args.chunk_mb)
                torch.cuda.synchronize(dev)
                dt = time.perf_counter() - t0
                if rep >= args.warmup:
                    times[r].append(dt)
                outs[r] = out
        same = None
        if routes == ["shards", "logits"]:
            # not the same bits (PARITY.md, L2): report how close
            a, b = outs["shards"], outs["logits"]
            same = {"preds_max_abs_diff":
                    float((a[0].float() - b[0].float()).abs().max()),
                    "classes_differ":
                    float((a[1] != b[1]).float().mean()),
                    "ens_max_abs_diff": float((a[2] - b[2]).abs().max())}
        elif len(routes) == 2:
            a, b = outs["legacy"], outs["shards"]
            raw = (lambda t: t.view(torch.uint8)
                   if t.dtype == torch.float8_e4m3fn else t)
            same = {"preds": bool(torch.equal(raw(a[0]), raw(b[0]))),
                    "classes": bool(torch.equal(a[1], b[1])),
                    "mirror": bool(torch.equal(raw(a[3]), raw(b[3]))),
                    "ens_max_abs_diff": float((a[2] - b[2]).abs().max())}

    wsz = torch.empty(0, dtype=STORAGE_DTYPES[args.dtype]).element_size()
    ssz = torch.empty(0, dtype=STORAGE_DTYPES[args.storage]).element_size()
    elems = H * N * C
    # the loader's chunking: whole models per call while they fit the
    # budget (never across a shard), else one model at a time (its
    # sub-splits along n touch disjoint consensus rows). n_calls counts
    # whole-(N, C) consensus read-modify-writes.
    rows = max(1, (args.chunk_mb << 20) // (N * C * wsz))
    n_calls = 0
    for h0 in range(0, H, args.models_per_shard):
        k = min(args.models_per_shard, H - h0)
        n_calls += -(-k // rows)
    wire = None
    if args.kind == "both":
        wire = measure_wire(dev, min(rows, args.models_per_shard, H)
                            * N * C * wsz)
    res = {
        "shape": [H, N, C], "disk_dtype": args.dtype,
        "storage": args.storage, "chunk_mb": args.chunk_mb,
        "wall_s": {r: sorted(v) for r, v in times.items()},
        "wall_s_median": {r: sorted(v)[len(v) // 2]
                          for r, v in times.items() if v},
        "wall_s_spread": {r: (max(v) - min(v)) / sorted(v)[len(v) // 2]
                          for r, v in times.items() if v},
        # legacy up-casts on the host and ships fp32 (an fp16 file bound
        # for fp16 storage ships as it is); shards ship the file
        "host_wire_bytes": {
            "legacy": elems * (2 if args.dtype == args.storage == "fp16"
                               else 4),
            "shards": elems * wsz, "logits": elems * wsz},
        "ingest_calls": n_calls, "host_wire": wire,
        # wire in + pool out + mirror out + one consensus RMW per call
        "ingest_kernel_floor_bytes":
            elems * (wsz + 2 * ssz) + n_calls * 2 * N * C * 4,
        "routes_agree": same,
    }
    print(json.dumps(res))


if __name__ == "__main__":
    main()
