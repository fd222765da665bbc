"""Convert prediction-tensor files to a compact on-disk dtype.

The benchmark .pt files ship fp16/fp32; storing bf16 or fp8-e4m3 halves /
quarters both disk and host->device wire bytes (the loader up-casts to
fp32 for compute either way - coda_amd/datasets.py); fp16 halves an fp32
file and is lossless for data that was fp16 to begin with. Labels files
are copied unchanged.

Usage:
    python scripts/convert_task.py --task T [--data-dir data]
        [--dtype fp16|bf16|fp8] [--out-dir data_bf16]
    python scripts/convert_task.py --all --data-dir data --dtype fp8
    python scripts/convert_task.py --task T --dtype fp8 --shards
        [--models-per-shard 16]
    python scripts/convert_task.py --task T --dtype fp16 --shards
        --kind logits [--temperature 2.0]

--shards writes the sharded format `<out-dir>/<task>.shards/`
(coda_amd/datasets.py) instead of one .pt: the source is opened with mmap
and converted one shard at a time, so no full-size copy - fp32 or
otherwise - is ever made. That is the route for pools beyond host memory.

--kind logits (with --shards; fp32 / fp16 / bf16) declares the input .pt
to hold pre-softmax logits: the task is written in format
coda_amd.shards/2 and the loader's ingest pass applies the temperature
softmax (--temperature is recorded as the task's default; the loader's
own --temperature overrides it). Every shard is checked as it is written:
entries finite or -inf, a finite entry in every row.
"""
from __future__ import annotations

import argparse
import os
import shutil
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from coda_amd.datasets import (STORAGE_DTYPES, WIRE_DTYPES,  # noqa: E402
                               write_sharded_task)


def convert(task: str, data_dir: str, out_dir: str, dtype: str):
    src = os.path.join(data_dir, task + ".pt")
    dst = os.path.join(out_dir, task + ".pt")
    t = torch.load(src, map_location="cpu", weights_only=True)
    t = t.to(STORAGE_DTYPES[dtype])
    os.makedirs(out_dir, exist_ok=True)
    torch.save(t, dst)
    lbl = src.replace(".pt", "_labels.pt")
    if os.path.exists(lbl):
        shutil.copyfile(lbl, dst.replace(".pt", "_labels.pt"))
    print(f"{task}: {os.path.getsize(src)/1e6:.1f} MB -> "
          f"{os.path.getsize(dst)/1e6:.1f} MB ({dtype})")


def convert_shards(task: str, data_dir: str, out_dir: str, dtype: str,
                   models_per_shard: int, kind: str = "probs",
                   temperature=None):
    src = os.path.join(data_dir, task + ".pt")
    dst = os.path.join(out_dir, task + ".shards")
    t = torch.load(src, map_location="cpu", weights_only=True, mmap=True)
    labels = None
    lbl = src.replace(".pt", "_labels.pt")
    if os.path.exists(lbl):
        labels = torch.load(lbl, map_location="cpu", weights_only=True)
    write_sharded_task(dst, t, dtype, models_per_shard, labels=labels,
                       kind=kind, temperature=temperature)
    n = -(-t.shape[0] // models_per_shard)
    what = dtype if kind == "probs" else f"{dtype} logits"
    print(f"{task}: {os.path.getsize(src)/1e6:.1f} MB -> {n} shard(s) of "
          f"<= {models_per_shard} models ({what}) in {dst}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--task", default=None)
    ap.add_argument("--all", action="store_true")
    ap.add_argument("--data-dir", default="data")
    ap.add_argument("--dtype", default="bf16", choices=sorted(WIRE_DTYPES))
    ap.add_argument("--out-dir", default=None)
    ap.add_argument("--shards", action="store_true",
                    help="write <task>.shards/ instead of one .pt")
    ap.add_argument("--models-per-shard", type=int, default=16)
    ap.add_argument("--kind", default="probs", choices=["probs", "logits"],
                    help="what the input .pt holds (logits need --shards)")
    ap.add_argument("--temperature", type=float, default=None,
                    help="default softmax temperature of a logits task")
    args = ap.parse_args()
    if args.kind == "logits" and not args.shards:
        ap.error("--kind logits needs --shards")
    if args.temperature is not None and args.kind != "logits":
        ap.error("--temperature needs --kind logits")
    if not args.shards and args.dtype not in STORAGE_DTYPES:
        ap.error(f"--dtype {args.dtype} needs --shards")
    out_dir = args.out_dir or f"{args.data_dir}_{args.dtype}"
    if args.all:
        tasks = sorted(f[:-3] for f in os.listdir(args.data_dir)
                       if f.endswith(".pt")
                       and not f.endswith("_labels.pt"))
    else:
        assert args.task, "--task or --all"
        tasks = [args.task]
    for t in tasks:
        if args.shards:
            convert_shards(t, args.data_dir, out_dir, args.dtype,
                           args.models_per_shard, args.kind,
                           args.temperature)
        else:
            convert(t, args.data_dir, out_dir, args.dtype)


if __name__ == "__main__":
    main()
