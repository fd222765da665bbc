"""Prediction-tensor datasets.

On-disk format (identical to the reference, coda/datasets.py:4-23): a
`<task>.pt` tensor of shape (H, N, C) holding post-softmax scores - H models,
N points, C classes - optionally with `<task>_labels.pt` holding (N,) integer
ground-truth labels. Stored dtype may be fp16/bf16; compute is always fp32
(the loader up-casts, or - storage_dtype="fp16" - keeps the fp16 bits and
every consumer up-casts, which is the same computation at half the bytes).

Additions over the reference:
  - model-axis sharding for multi-GPU runs (`shard` argument): rank r keeps
    rows h where h % world == r, so every rank's slice is balanced.
  - pinned-host staging for large tensors (`pin=True`): the (H,N,C) tensor is
    loaded to pinned CPU memory and copied to the device on a side stream
    (non_blocking), instead of the reference's single blocking load.
  - synthetic task generator with a planted best model (for tests/benchmarks).
  - a sharded low-precision format for pools beyond host memory,
    `<task>.shards/`:
      manifest.json  {"format": "coda_amd.shards/1", "H", "N", "C",
                      "dtype": "fp32|fp16|bf16|fp8",
                      "shards": [{"file", "h0", "h1"}, ...],
                      "labels": "labels.pt" | null}
      one torch.save'd contiguous (h1-h0, N, C) tensor per shard in the
      manifest dtype (fp8 = float8_e4m3fn, the OCP encoding gfx950 uses);
      shards partition [0, H) in ascending order along the model axis.
    `Dataset(<dir or manifest>)` streams it chunk by chunk in the file's
    own dtype through the fused ingest op (ops.ingest_chunk) - see
    Dataset._init_sharded; `write_sharded_task` writes it.
  - logit pools, in the sharded format only: a manifest with
      "format": "coda_amd.shards/2", "kind": "logits",
      "temperature": T | [T_0, ..., T_{H-1}]        (optional, default 1)
    holds pre-softmax logits (fp32 / fp16 / bf16; entries finite or -inf,
    at least one finite per row). The ingest op applies the per-model
    temperature softmax softmax(x / T_h) in the same pass, so the loaded
    `Dataset` is an ordinary probability pool and `Dataset(...,
    temperature=)` re-tempers at load time without rewriting the file.
    The format number moves so that a build that predates logits refuses
    such a task instead of reading logits as probabilities. `.pt` files
    and `Dataset.from_tensors` are probability-only.
"""
from __future__ import annotations

import json
import os
import math
from typing import Optional, Tuple

import torch


STORAGE_DTYPES = {
    "fp32": torch.float32,
    "fp16": torch.float16,
    "bf16": torch.bfloat16,
    "fp8": torch.float8_e4m3fn,
}

# on-disk / host-wire dtypes of the sharded format
WIRE_DTYPES = dict(STORAGE_DTYPES)
# in-memory pools Dataset.from_tensors keeps when no storage dtype is asked
# for; an fp16 tensor is up-cast there, like an fp16 file by default
_KEPT_DTYPES = (torch.float32, torch.bfloat16, torch.float8_e4m3fn)
SHARD_FORMAT = "coda_amd.shards/1"
# logits tasks: same layout plus "kind" and an optional "temperature"
SHARD_FORMAT_LOGITS = "coda_amd.shards/2"
SHARD_FORMATS = (SHARD_FORMAT, SHARD_FORMAT_LOGITS)
TASK_KINDS = ("probs", "logits")
LOGIT_WIRE_DTYPES = ("fp32", "fp16", "bf16")
MANIFEST_NAME = "manifest.json"


class Dataset:
    # what the task file held; a logits task also records the (H,) fp64
    # temperatures its softmax was taken at (global model ids)
    kind = "probs"
    temperature = None

    def __init__(self, filepath: str, device,
                 shard: Optional[Tuple[int, int]] = None,
                 pin: bool = False,
                 storage_dtype: str = "fp32",
                 stream_chunk_mb: int = 0,
                 temperature=None):
        """Load a prediction tensor.

        Args:
            filepath: path to the (H, N, C) .pt file, or to a sharded task
                (the `<task>.shards/` directory or its manifest.json);
                for the latter stream_chunk_mb bounds every host chunk
                (256 when 0; fractions allowed) and `init_stats` is set.
            device: target device.
            shard: optional (rank, world_size); keeps models h with
                h % world_size == rank.
            pin: stage through pinned host memory with an async copy.
            storage_dtype: on-device storage format - "fp32" (reference
                parity), "fp16", "bf16" or "fp8" (e4m3). Compute always
                up-casts to fp32 (the reference's own fp16-on-disk ->
                .float() pattern, coda/datasets.py:14, generalized).
                Halving / quartering storage is what fits large model
                pools into the 288 GB of HBM3E. "fp16" is lossless for
                fp16 source data (the benchmark files) at half of fp32:
                fp16 -> fp32 is exact, so a run on it computes what the
                fp32-stored run computes. An fp16 .pt file then skips
                the host up-cast and is staged and copied as fp16.
            stream_chunk_mb: >0 streams the tensor host->device in chunks
                of this size through pinned buffers on a side stream
                (dtype conversion on device), instead of one blocking copy.
            temperature: softmax temperature of a sharded LOGITS task
                (manifest "kind": "logits"): one positive number or one
                per model (length H, global model ids whatever `shard`
                is). Overrides the manifest's value; default is the
                manifest's, else 1. A ValueError for a probability task
                (sharded or .pt), whose softmax is already in the file.
        """
        self.device = torch.device(device)
        if _is_sharded_path(filepath):
            self._init_sharded(filepath, shard, storage_dtype,
                               stream_chunk_mb, temperature)
            return
        if temperature is not None:
            raise ValueError("temperature applies to sharded logits tasks "
                             f"only; {filepath} holds probabilities")
        preds = torch.load(filepath, map_location="cpu", weights_only=True)
        dt = STORAGE_DTYPES[storage_dtype]
        # an fp16 file bound for fp16 storage stays fp16 on the host, on
        # the wire and on the device; anything else goes through fp32
        if not (dt == torch.float16 and preds.dtype == dt):
            preds = preds.float()
        self.total_models = preds.shape[0]
        self.shard = shard
        if shard is not None:
            rank, world = shard
            self.model_idxs = torch.arange(rank, self.total_models, world)
            preds = preds[self.model_idxs]
        else:
            self.model_idxs = torch.arange(self.total_models)
        self.storage_dtype = storage_dtype
        if stream_chunk_mb and self.device.type == "cuda":
            self.preds = _stream_to_device(preds, self.device, dt,
                                           stream_chunk_mb)
        else:
            self.preds = _to_device(preds, self.device, pin).to(dt)

        self.labels = None
        label_p = filepath.replace(".pt", "_labels.pt")
        if os.path.exists(label_p):
            labels = torch.load(label_p, map_location="cpu", weights_only=True)
            self.labels = labels.to(self.device)

    def _init_sharded(self, path, shard, storage_dtype, stream_chunk_mb,
                      temperature=None):
        """Load a `<task>.shards/` directory (format: module docstring).

        The host never holds more than two chunks, in the file's own
        dtype: each shard is opened with mmap, bounded chunks (at most
        `stream_chunk_mb` MB, 256 when 0; sub-split along the point axis
        when one model exceeds that) are staged through two pinned
        buffers, copied on a side stream, and handed to ops.ingest_chunk
        on that stream - one fused pass that rounds to the storage dtype
        and produces the selector's init statistics (`init_stats`) and,
        HBM headroom permitting, the class-major mirror. On a CPU device
        the same loop runs with the eager twin.

        A logits task (manifest "kind": "logits") takes the same route
        with the same host footprint: every chunk carries its models'
        k_h = float32(log2(e) / T_h) and the ingest pass applies the
        temperature softmax before rounding, so everything downstream
        sees a probability pool."""
        from . import ops
        from .util import mirror_fits

        man = read_shard_manifest(path)
        root = man["root"]
        H, N, C = man["H"], man["N"], man["C"]
        wire_dt = WIRE_DTYPES[man["dtype"]]
        dt = STORAGE_DTYPES[storage_dtype]
        dev = self.device
        self.total_models = H
        self.shard = shard
        rank, world = shard if shard is not None else (0, 1)
        self.model_idxs = torch.arange(rank, H, world)
        self.storage_dtype = storage_dtype
        Hl = self.model_idxs.numel()
        logits = man["kind"] == "logits"
        self.kind = man["kind"]
        self.temperature = None
        scale = None
        if logits:
            if temperature is None:
                temperature = man["temperature"]
            temps = _check_temperature(
                1.0 if temperature is None else temperature, H,
                "temperature")
            if len(temps) == 1:
                temps = temps * H
            # by GLOBAL model id; k_h rounded once, from fp64
            self.temperature = torch.tensor(temps, dtype=torch.float64)
            scale = ((math.log2(math.e) / self.temperature)
                     .to(torch.float32)[self.model_idxs].to(dev))
        elif temperature is not None:
            raise ValueError("temperature applies to logits tasks only; "
                             f"{path} holds probabilities")

        esize = torch.empty(0, dtype=wire_dt).element_size()
        budget = max(1, int((stream_chunk_mb or 256) * (1 << 20)))
        per_model = N * C * esize
        if per_model <= budget:
            rows, npts = max(1, budget // per_model), N
        else:
            rows, npts = 1, max(1, budget // (C * esize))

        on_gpu = dev.type == "cuda"
        pool_bytes = Hl * N * C * torch.empty(0, dtype=dt).element_size()
        want_t = (on_gpu and ops.hip_available()
                  and mirror_fits(dev, pool_bytes, pool_resident=False))
        preds = torch.empty((Hl, N, C), dtype=dt, device=dev)
        classes = torch.empty((Hl, N), dtype=torch.long, device=dev)
        ens = torch.zeros((N, C), dtype=torch.float32, device=dev)
        preds_t = (torch.empty((Hl, C, N), dtype=dt, device=dev)
                   if want_t else None)

        if on_gpu:
            side = torch.cuda.Stream(device=dev)
            side.wait_stream(torch.cuda.current_stream(dev))  # ens zeros
            bufs = [torch.empty(min(rows, max(Hl, 1)) * npts * C,
                                dtype=wire_dt).pin_memory()
                    for _ in range(2)]
            events = [torch.cuda.Event(), torch.cuda.Event()]
            for e in events:
                e.record(side)
        i = 0
        for sh in man["shards"]:
            # local models inside this shard: h = rank + l * world
            l0 = -(-(sh["h0"] - rank) // world) if sh["h0"] > rank else 0
            l1 = min(Hl, -(-(sh["h1"] - rank) // world))
            if l1 <= l0:
                continue
            t = torch.load(os.path.join(root, sh["file"]),
                           map_location="cpu", weights_only=True, mmap=True)
            _check_shard_tensor(t, sh, N, C, wire_dt)
            for la in range(l0, l1, rows):
                lb = min(la + rows, l1)
                a = rank + la * world - sh["h0"]
                b = rank + (lb - 1) * world - sh["h0"] + 1
                for n0 in range(0, N, npts):
                    n1 = min(n0 + npts, N)
                    src = t[a:b:world, n0:n1]
                    k_h = scale[la:lb] if logits else None
                    if not on_gpu:
                        ops.ingest_chunk(src.contiguous(), la, n0, preds,
                                         classes, ens, preds_t, k_h)
                        continue
                    k = i % 2
                    i += 1
                    events[k].synchronize()  # buffer free to reuse
                    stage = bufs[k][:src.numel()].view(src.shape)
                    stage.copy_(src)
                    with torch.cuda.stream(side):
                        wire = stage.to(dev, non_blocking=True)
                        ops.ingest_chunk(wire, la, n0, preds, classes, ens,
                                         preds_t, k_h)
                        events[k].record(side)
            del t
        if on_gpu:
            torch.cuda.current_stream(dev).wait_stream(side)
        # the one guard against a logits file our writer did not check
        # (a NaN / +inf entry or an all -inf row makes its row non-finite)
        if logits and not bool(torch.isfinite(ens).all()):
            raise ValueError(f"{path}: non-finite probabilities from a "
                             "logits task (logits must be finite or -inf, "
                             "with a finite entry in every row)")

        self.preds = preds
        self.init_stats = {"classes": classes, "ens_sum": ens,
                           "preds_t": preds_t}
        self.labels = None
        if man["labels"] is not None:
            labels = torch.load(os.path.join(root, man["labels"]),
                                map_location="cpu", weights_only=True)
            self.labels = labels.to(dev)

    @classmethod
    def from_tensors(cls, preds: torch.Tensor, labels: Optional[torch.Tensor],
                     device, shard: Optional[Tuple[int, int]] = None,
                     storage_dtype: Optional[str] = None):
        """Build a Dataset from in-memory tensors (tests, synthetic tasks).

        A tensor already in fp32 / bf16 / fp8-e4m3 is kept as is -
        up-casting a 1M-point fp8 pool to fp32 would be 512 GB; any other
        dtype, fp16 included, is up-cast to fp32. storage_dtype, when
        given, names the storage dtype instead: the pool is converted to
        it (through fp32), or kept if it already has that dtype.
        """
        self = cls.__new__(cls)
        self.device = torch.device(device)
        if storage_dtype is not None:
            dt = STORAGE_DTYPES[storage_dtype]
            if preds.dtype != dt:
                preds = preds.float().to(dt)
            self.storage_dtype = storage_dtype
        elif preds.dtype not in _KEPT_DTYPES:
            preds = preds.float()
        self.total_models = preds.shape[0]
        self.shard = shard
        if shard is not None:
            rank, world = shard
            self.model_idxs = torch.arange(rank, self.total_models, world)
            preds = preds[self.model_idxs]
        else:
            self.model_idxs = torch.arange(self.total_models)
        self.preds = preds.to(self.device)
        self.labels = labels.to(self.device) if labels is not None else None
        return self


def resolve_task_path(data_dir: str, task: str) -> str:
    """`<data_dir>/<task>.pt` when it exists (as always); only when it is
    missing, `<data_dir>/<task>.shards` if that holds a manifest."""
    pt = os.path.join(data_dir, task + ".pt")
    if not os.path.exists(pt):
        shards = os.path.join(data_dir, task + ".shards")
        if os.path.exists(os.path.join(shards, MANIFEST_NAME)):
            return shards
    return pt


def _is_sharded_path(path: str) -> bool:
    return os.path.isdir(path) or os.path.basename(path) == MANIFEST_NAME


def _check_temperature(t, H: int, what: str) -> list:
    """One positive finite number, or a list of 1 or H of them -> list."""
    if isinstance(t, torch.Tensor):
        t = t.tolist()
    vals = list(t) if isinstance(t, (list, tuple)) else [t]
    if len(vals) not in (1, H):
        raise ValueError(f"{what}: expected one value or one per model "
                         f"({H}), got {len(vals)}")
    out = []
    for v in vals:
        if (isinstance(v, bool) or not isinstance(v, (int, float))
                or not math.isfinite(v) or v <= 0):
            raise ValueError(f"{what}: {v!r} is not a positive finite "
                             "number")
        out.append(float(v))
    return out


def read_shard_manifest(path: str, formats=SHARD_FORMATS) -> dict:
    """Read and validate `<task>.shards/manifest.json` (path may be the
    directory or the manifest). Returns the manifest with a `root` key
    (the directory) and `kind` / `temperature` filled in ("probs" / None
    when absent); raises ValueError on an unknown format (one not in
    `formats`), dtype or kind, a malformed temperature, or shards that do
    not partition [0, H) in ascending order."""
    root = path if os.path.isdir(path) else os.path.dirname(path)
    mpath = os.path.join(root, MANIFEST_NAME)
    if not os.path.exists(mpath):
        raise FileNotFoundError(f"no {MANIFEST_NAME} in {root}")
    with open(mpath) as f:
        man = json.load(f)
    formats = tuple(formats)
    if man.get("format") not in formats:
        want = formats[0] if len(formats) == 1 else f"one of {formats}"
        raise ValueError(f"{mpath}: unknown format {man.get('format')!r} "
                         f"(expected {want!r})")
    if man.get("dtype") not in WIRE_DTYPES:
        raise ValueError(f"{mpath}: unknown dtype {man.get('dtype')!r} "
                         f"(expected one of {sorted(WIRE_DTYPES)})")
    for k in ("H", "N", "C"):
        if not isinstance(man.get(k), int) or man[k] <= 0:
            raise ValueError(f"{mpath}: {k} must be a positive integer")
    shards = man.get("shards")
    if not isinstance(shards, list) or not shards:
        raise ValueError(f"{mpath}: no shards listed")
    at = 0
    for sh in shards:
        h0, h1 = sh.get("h0"), sh.get("h1")
        if not (isinstance(h0, int) and isinstance(h1, int) and h0 < h1
                and isinstance(sh.get("file"), str)):
            raise ValueError(f"{mpath}: malformed shard entry {sh!r}")
        if h0 > at:
            raise ValueError(f"{mpath}: gap in model ranges - models "
                             f"[{at}, {h0}) are in no shard")
        if h0 < at:
            raise ValueError(f"{mpath}: shard {sh['file']} [{h0}, {h1}) "
                             f"overlaps the models before {at}")
        at = h1
    if at != man["H"]:
        raise ValueError(f"{mpath}: shards cover [0, {at}) but H = "
                         f"{man['H']}")
    if man["format"] == SHARD_FORMAT_LOGITS:
        if man.get("kind") != "logits":
            raise ValueError(f"{mpath}: format {SHARD_FORMAT_LOGITS!r} "
                             f"needs \"kind\": \"logits\", got "
                             f"{man.get('kind')!r}")
        if man["dtype"] not in LOGIT_WIRE_DTYPES:
            raise ValueError(f"{mpath}: logits in {man['dtype']} are not "
                             f"supported (one of {LOGIT_WIRE_DTYPES})")
        if man.get("temperature") is not None:
            _check_temperature(man["temperature"], man["H"],
                               f"{mpath}: temperature")
    else:
        if man.get("kind", "probs") != "probs":
            raise ValueError(f"{mpath}: kind {man.get('kind')!r} needs "
                             f"format {SHARD_FORMAT_LOGITS!r}")
        if man.get("temperature") is not None:
            raise ValueError(f"{mpath}: temperature applies to logits "
                             "tasks only")
    man.setdefault("kind", "probs")
    man.setdefault("temperature", None)
    man.setdefault("labels", None)
    man["root"] = root
    return man


def _check_shard_tensor(t, sh, N, C, wire_dt):
    want = (sh["h1"] - sh["h0"], N, C)
    if not isinstance(t, torch.Tensor) or tuple(t.shape) != want:
        got = tuple(t.shape) if isinstance(t, torch.Tensor) else type(t)
        raise ValueError(f"shard {sh['file']}: shape {got} does not match "
                         f"the manifest's {want}")
    if t.dtype != wire_dt:
        raise ValueError(f"shard {sh['file']}: dtype {t.dtype} does not "
                         f"match the manifest's {wire_dt}")


def _check_logit_shard(out: torch.Tensor, name: str) -> None:
    """Logits as written: finite or -inf, a finite entry in every row
    (checked a model at a time: no shard-size fp32 transient)."""
    for h in range(out.shape[0]):
        x = out[h].float()
        fin = torch.isfinite(x)
        if bool((~fin & (x != float("-inf"))).any()):
            raise ValueError(f"shard {name}: logits of model {h} of the "
                             "shard hold NaN or +inf (entries must be "
                             "finite or -inf)")
        if not bool(fin.any(dim=-1).all()):
            raise ValueError(f"shard {name}: model {h} of the shard has a "
                             "row without a finite logit")


def write_sharded_task(out_dir: str, shard_iter_or_tensor, dtype: str,
                       models_per_shard: int = 16, labels=None,
                       kind: str = "probs", temperature=None) -> str:
    """Write a `<task>.shards/` directory in on-disk dtype `dtype`
    ("fp32" | "fp16" | "bf16" | "fp8").

    kind="probs" (post-softmax scores) writes format coda_amd.shards/1 as
    always. kind="logits" (fp32 / fp16 / bf16 only) writes format
    coda_amd.shards/2 with "kind": "logits" and, when `temperature` is
    given (one positive number or one per model), "temperature"; every
    shard is checked as written - entries finite or -inf, a finite entry
    in every row - and a violation raises ValueError naming the shard.

    The source is either one (H, N, C) tensor (an mmap'd one is fine: it
    is cut into `models_per_shard`-model slices, converted one at a time)
    or an iterable of (k, N, C) tensors, each written as one shard. No
    full-size copy is made. Returns the manifest path."""
    if dtype not in WIRE_DTYPES:
        raise ValueError(f"unknown dtype {dtype!r} "
                         f"(expected one of {sorted(WIRE_DTYPES)})")
    if kind not in TASK_KINDS:
        raise ValueError(f"unknown kind {kind!r} (expected one of "
                         f"{TASK_KINDS})")
    if kind == "logits" and dtype not in LOGIT_WIRE_DTYPES:
        raise ValueError(f"logits in {dtype} are not supported (one of "
                         f"{LOGIT_WIRE_DTYPES})")
    if kind != "logits" and temperature is not None:
        raise ValueError("temperature applies to kind=\"logits\" only")
    dt = WIRE_DTYPES[dtype]
    if isinstance(shard_iter_or_tensor, torch.Tensor):
        src = shard_iter_or_tensor
        if src.dim() != 3:
            raise ValueError("expected an (H, N, C) tensor")
        k = max(1, int(models_per_shard))
        pieces = (src[h:h + k] for h in range(0, src.shape[0], k))
    else:
        pieces = iter(shard_iter_or_tensor)
    os.makedirs(out_dir, exist_ok=True)
    shards, at, N, C = [], 0, None, None
    for piece in pieces:
        if piece.dim() != 3 or piece.shape[0] == 0:
            raise ValueError("each shard must be a non-empty (k, N, C) tensor")
        if N is None:
            N, C = int(piece.shape[1]), int(piece.shape[2])
        elif (int(piece.shape[1]), int(piece.shape[2])) != (N, C):
            raise ValueError("shards disagree on (N, C)")
        out = piece if piece.dtype == dt else piece.float().to(dt)
        h1 = at + int(piece.shape[0])
        name = f"h{at:06d}-{h1:06d}.pt"
        if kind == "logits":
            _check_logit_shard(out, name)
        # clone: a slice would drag its whole backing storage into the file
        torch.save(out.contiguous().clone(), os.path.join(out_dir, name))
        shards.append({"file": name, "h0": at, "h1": h1})
        at = h1
    if not shards:
        raise ValueError("no shards to write")
    label_name = None
    if labels is not None:
        label_name = "labels.pt"
        torch.save(labels.cpu().clone(), os.path.join(out_dir, label_name))
    man = {"format": SHARD_FORMAT, "H": at, "N": N, "C": C, "dtype": dtype,
           "shards": shards, "labels": label_name}
    if kind == "logits":
        man["format"] = SHARD_FORMAT_LOGITS
        man["kind"] = "logits"
        if temperature is not None:
            temps = _check_temperature(temperature, at, "temperature")
            man["temperature"] = temps[0] if len(temps) == 1 else temps
    mpath = os.path.join(out_dir, MANIFEST_NAME)
    with open(mpath, "w") as f:
        json.dump(man, f, indent=1)
    return mpath


def _stream_to_device(t: torch.Tensor, device: torch.device,
                      dtype: torch.dtype, chunk_mb: int) -> torch.Tensor:
    """Pinned double-buffered host->HBM streaming with on-device dtype
    conversion (the host wire is t's dtype: fp32, or fp16 for an fp16
    file bound for fp16 storage, which needs no conversion). Chunks along
    the model axis."""
    H = t.shape[0]
    out = torch.empty(t.shape, dtype=dtype, device=device)
    bytes_per_model = t[0].numel() * t.element_size()
    rows = max(1, (chunk_mb << 20) // max(1, bytes_per_model))
    side = torch.cuda.Stream(device=device)
    bufs = [torch.empty((min(rows, H),) + t.shape[1:],
                        dtype=t.dtype).pin_memory() for _ in range(2)]
    events = [torch.cuda.Event(), torch.cuda.Event()]
    for e in events:
        e.record(side)
    for i, h0 in enumerate(range(0, H, rows)):
        h1 = min(h0 + rows, H)
        buf = bufs[i % 2]
        events[i % 2].synchronize()  # buffer free to reuse
        buf[:h1 - h0].copy_(t[h0:h1])
        with torch.cuda.stream(side):
            staged = buf[:h1 - h0].to(device, non_blocking=True)
            out[h0:h1].copy_(staged.to(dtype))
            events[i % 2].record(side)
    torch.cuda.current_stream(device).wait_stream(side)
    return out


def _to_device(t: torch.Tensor, device: torch.device, pin: bool) -> torch.Tensor:
    if device.type != "cuda" or not pin:
        return t.to(device)
    # Pinned staging + async copy on a side stream; keeps the default stream
    # free while a large pool streams into HBM.
    pinned = t.pin_memory()
    side = torch.cuda.Stream(device=device)
    with torch.cuda.stream(side):
        out = pinned.to(device, non_blocking=True)
    torch.cuda.current_stream(device).wait_stream(side)
    return out


def make_synthetic_task(H: int = 8, N: int = 500, C: int = 10,
                        seed: int = 0, best_acc: float = 0.9,
                        worst_acc: float = 0.5, temperature: float = 3.0):
    """Random (H, N, C) prediction tensor with a planted best model.

    Model h's accuracy interpolates from best_acc (h=0) to worst_acc
    (h=H-1); predictions are softmaxed logits biased toward the model's
    (possibly corrupted) predicted class. Returns (preds, labels) on CPU.
    """
    g = torch.Generator().manual_seed(seed)
    labels = torch.randint(0, C, (N,), generator=g)
    accs = torch.linspace(best_acc, worst_acc, H)
    preds = torch.empty(H, N, C)
    for h in range(H):
        correct = torch.rand(N, generator=g) < accs[h]
        wrong = torch.randint(1, C, (N,), generator=g)
        pred_class = torch.where(correct, labels, (labels + wrong) % C)
        logits = torch.randn(N, C, generator=g)
        logits[torch.arange(N), pred_class] += temperature
        preds[h] = torch.softmax(logits, dim=-1)
    return preds, labels


def write_synthetic_task(data_dir: str, name: str = "synthetic", **kwargs):
    """Materialize a synthetic task as <data_dir>/<name>.pt (+ _labels.pt)."""
    os.makedirs(data_dir, exist_ok=True)
    preds, labels = make_synthetic_task(**kwargs)
    torch.save(preds, os.path.join(data_dir, f"{name}.pt"))
    torch.save(labels, os.path.join(data_dir, f"{name}_labels.pt"))
    return os.path.join(data_dir, f"{name}.pt")
