"""fp16 prediction-pool storage on the CPU: loader, sharded ingest, every
selector, the CLIs.

fp16 -> fp32 is an exact conversion, so a run on an fp16-stored pool whose
values are fp16-representable is the same computation as the run on the
fp32-stored pool. Nothing here is approximate: stored values are compared
through their bit patterns and trajectories with ==.
"""
import os
import random
import subprocess
import sys

import pytest
import torch

from coda_amd.datasets import (Dataset, STORAGE_DTYPES, WIRE_DTYPES,
                               make_synthetic_task, write_sharded_task)

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F16 = torch.float16
SHAPES = [(8, 300, 5), (6, 200, 33)]
STEPS = 25


def _bits(t):
    assert t.dtype == F16
    return t.view(torch.int16)


@pytest.fixture(scope="module")
def pools():
    """fp16-representable synthetic pools, one per shape (never modified)."""
    out = {}
    for H, N, C in SHAPES:
        p, labels = make_synthetic_task(H=H, N=N, C=C, seed=H)
        out[(H, N, C)] = (p.half(), labels)
    return out


def test_fp16_is_a_storage_dtype():
    assert STORAGE_DTYPES["fp16"] == F16
    assert WIRE_DTYPES["fp16"] == F16


@pytest.mark.parametrize("file_dt", [F16, torch.float32, torch.bfloat16])
def test_legacy_pt_loads_as_fp16(tmp_path, pools, file_dt, monkeypatch):
    p16, labels = pools[SHAPES[0]]
    src = (p16 if file_dt == F16
           else make_synthetic_task(H=4, N=50, C=7, seed=3)[0].to(file_dt))
    path = str(tmp_path / "t.pt")
    torch.save(src, path)
    torch.save(labels, str(tmp_path / "t_labels.pt"))

    upcasts = []
    real_float = torch.Tensor.float

    def spy(self, *a, **k):
        upcasts.append(tuple(self.shape))
        return real_float(self, *a, **k)
    monkeypatch.setattr(torch.Tensor, "float", spy)
    ds = Dataset(path, "cpu", storage_dtype="fp16")
    monkeypatch.undo()

    assert ds.preds.dtype == F16 and ds.storage_dtype == "fp16"
    assert ds.preds.element_size() == 2
    assert torch.equal(_bits(ds.preds), _bits(src.float().to(F16)))
    if file_dt == F16:
        assert torch.equal(_bits(ds.preds), _bits(src))
        assert not upcasts, "an fp16 file must skip the host up-cast"
    else:
        assert upcasts
    assert torch.equal(ds.labels, labels)
    # the default stays what it was: fp32 storage, up-cast on load
    assert Dataset(path, "cpu").preds.dtype == torch.float32


def test_legacy_pt_fp16_model_shard(tmp_path, pools):
    p16, _ = pools[SHAPES[0]]
    path = str(tmp_path / "t.pt")
    torch.save(p16, path)
    ds = Dataset(path, "cpu", shard=(1, 3), storage_dtype="fp16")
    assert torch.equal(_bits(ds.preds), _bits(p16[1::3]))


@pytest.mark.parametrize("wire", ["fp32", "fp16", "bf16", "fp8"])
def test_sharded_task_loads_as_fp16(tmp_path, wire):
    src, labels = make_synthetic_task(H=5, N=40, C=7, seed=2,
                                      temperature=0.5)
    d = str(tmp_path / "t.shards")
    write_sharded_task(d, src, wire, models_per_shard=2, labels=labels)
    want = src.to(WIRE_DTYPES[wire]).float().to(F16)
    for chunk_mb in (0, 13 * 7 * 4 / (1 << 20)):   # whole shards / n-splits
        ds = Dataset(d, "cpu", storage_dtype="fp16",
                     stream_chunk_mb=chunk_mb)
        assert ds.preds.dtype == F16
        assert torch.equal(_bits(ds.preds), _bits(want))
        assert torch.equal(ds.init_stats["classes"], want.float().argmax(-1))
        assert ds.init_stats["preds_t"] is None     # no mirror on the CPU
        assert torch.equal(ds.labels, labels)


@pytest.mark.parametrize("shape", SHAPES, ids=["8x300x5", "6x200x33"])
def test_sharded_init_stats_equal_fp32_storage(tmp_path, pools, shape):
    p16, labels = pools[shape]
    d = str(tmp_path / "t.shards")
    write_sharded_task(d, p16, "fp16", models_per_shard=3, labels=labels)
    a = Dataset(d, "cpu", storage_dtype="fp16")
    b = Dataset(d, "cpu", storage_dtype="fp32")
    assert torch.equal(_bits(a.preds), _bits(p16))
    assert torch.equal(a.preds.float(), b.preds)
    assert torch.equal(a.init_stats["classes"], b.init_stats["classes"])
    assert torch.equal(a.init_stats["ens_sum"], b.init_stats["ens_sum"])


def test_from_tensors_storage_keyword(pools):
    p16, labels = pools[SHAPES[0]]
    # default: an fp16 tensor is still up-cast
    assert Dataset.from_tensors(p16, labels, "cpu").preds.dtype \
        == torch.float32
    kept = Dataset.from_tensors(p16, labels, "cpu", storage_dtype="fp16")
    assert kept.preds.dtype == F16 and kept.storage_dtype == "fp16"
    assert torch.equal(_bits(kept.preds), _bits(p16))
    p32, _ = make_synthetic_task(H=3, N=20, C=4, seed=1)
    conv = Dataset.from_tensors(p32, None, "cpu", storage_dtype="fp16")
    assert torch.equal(_bits(conv.preds), _bits(p32.to(F16)))
    up = Dataset.from_tensors(p16, None, "cpu", storage_dtype="fp32")
    assert torch.equal(up.preds, p16.float())
    b16 = Dataset.from_tensors(p32, None, "cpu", storage_dtype="bf16")
    assert torch.equal(b16.preds.view(torch.int16),
                       p32.to(torch.bfloat16).view(torch.int16))


def _selectors():
    from coda_amd import CODA
    from coda_amd.baselines.activetesting import ActiveTesting
    from coda_amd.baselines.iid import IID
    from coda_amd.baselines.modelpicker import ModelPicker
    from coda_amd.baselines.uncertainty import Uncertainty
    from coda_amd.baselines.vma import VMA
    from coda_amd.options import accuracy_loss
    return {
        "coda": lambda ds: CODA(ds, chunk_size=64),
        "coda_fp32_pi_hat": lambda ds: CODA(ds, chunk_size=64,
                                            pi_hat_precision="fp32"),
        "coda_prefilter50": lambda ds: CODA(ds, chunk_size=64,
                                            prefilter_n=50),
        "iid": lambda ds: IID(ds, accuracy_loss),
        "uncertainty": lambda ds: Uncertainty(ds, accuracy_loss),
        "activetesting": lambda ds: ActiveTesting(ds, accuracy_loss),
        "vma": lambda ds: VMA(ds, accuracy_loss),
        "modelpicker": lambda ds: ModelPicker(ds),
    }


def _trajectory(make, ds, labels):
    random.seed(0)
    torch.manual_seed(0)
    sel = make(ds)
    out = []
    for _ in range(STEPS):
        idx, q = sel.get_next_item_to_label()
        sel.add_label(idx, int(labels[int(idx)]), q)
        out.append((int(idx), float(q),
                    int(sel.get_best_model_prediction())))
    return out


@pytest.mark.parametrize("shape", SHAPES, ids=["8x300x5", "6x200x33"])
@pytest.mark.parametrize("method", ["coda", "coda_fp32_pi_hat",
                                    "coda_prefilter50", "iid", "uncertainty",
                                    "activetesting", "vma", "modelpicker"])
def test_trajectory_equals_fp32_storage(pools, shape, method):
    """Chosen index, selection value and best model, step for step."""
    p16, labels = pools[shape]
    make = _selectors()[method]
    ds16 = Dataset.from_tensors(p16, labels, "cpu", storage_dtype="fp16")
    ds32 = Dataset.from_tensors(p16.float(), labels, "cpu")
    assert ds16.preds.dtype == F16 and ds32.preds.dtype == torch.float32
    got = _trajectory(make, ds16, labels)
    want = _trajectory(make, ds32, labels)
    for step, (g, w) in enumerate(zip(got, want)):
        assert g == w, (step, g, w)


def test_coda_keeps_fp32_pi_hat_on_fp16(pools):
    """The fp8 rule (no fp32 contraction on fp8 storage) must not catch
    fp16."""
    from coda_amd import CODA
    p16, labels = pools[SHAPES[0]]
    ds = Dataset.from_tensors(p16, labels, "cpu", storage_dtype="fp16")
    sel = CODA(ds, chunk_size=64, pi_hat_precision="fp32")
    assert sel.pi_hat_precision == "fp32"


def test_ensemble_mean_chunks_equal_whole(pools):
    """The fp16 up-cast is chunked along the point axis; every chunking
    gives preds.float().mean(0)."""
    from coda_amd.ops import reference
    p16, _ = pools[SHAPES[1]]
    want = p16.float().mean(dim=0)
    for chunk_n in (0, 37, 1):
        got = reference.ensemble_mean(p16, chunk_n)
        assert got.dtype == torch.float32 and torch.equal(got, want)
    # the other storage dtypes keep the mean in their own dtype
    b = p16.float().to(torch.bfloat16)
    assert torch.equal(reference.ensemble_mean(b), b.mean(dim=0))


def test_cli_storage_fp16(tmp_path, monkeypatch):
    import main as harness
    from coda_amd import tracking
    p, labels = make_synthetic_task(H=6, N=200, C=4, seed=0)
    os.makedirs(tmp_path / "data")
    torch.save(p.half(), str(tmp_path / "data" / "t16.pt"))
    torch.save(labels, str(tmp_path / "data" / "t16_labels.pt"))
    seen = []
    real_init = Dataset.__init__

    def spy(self, *a, **k):
        real_init(self, *a, **k)
        seen.append(self.preds.dtype)
    monkeypatch.setattr(Dataset, "__init__", spy)
    monkeypatch.chdir(tmp_path)
    tracking._EXPERIMENT = None
    tracking._RUN_STACK.clear()
    harness.main(["--task", "t16", "--data-dir", "data", "--device", "cpu",
                  "--method", "coda", "--iters", "3", "--seeds", "1",
                  "--no-mlflow", "--chunk-size", "64", "--storage", "fp16"])
    assert seen == [F16]


def test_convert_task_fp16_pt_roundtrip(tmp_path):
    p, labels = make_synthetic_task(H=4, N=60, C=6, seed=4)
    os.makedirs(tmp_path / "data")
    torch.save(p, str(tmp_path / "data" / "t.pt"))
    torch.save(labels, str(tmp_path / "data" / "t_labels.pt"))
    r = subprocess.run(
        [sys.executable, os.path.join(REPO, "scripts", "convert_task.py"),
         "--task", "t", "--data-dir", str(tmp_path / "data"),
         "--dtype", "fp16", "--out-dir", str(tmp_path / "data_fp16")],
        capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    out = torch.load(str(tmp_path / "data_fp16" / "t.pt"),
                     weights_only=True)
    assert out.dtype == F16
    assert torch.equal(_bits(out), _bits(p.to(F16)))
    ds = Dataset(str(tmp_path / "data_fp16" / "t.pt"), "cpu",
                 storage_dtype="fp16")
    assert torch.equal(_bits(ds.preds), _bits(out))
    assert torch.equal(ds.labels, labels)
