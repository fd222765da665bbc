"""Sharded low-precision task format + the ingest contract (CPU).

Covers the writer / manifest reader, the convert script and main.py's
task resolution, the loader's host-side bound, and the eager twin of the
fused ingest op against a hand-written loop. The GPU kernel is checked
against the same twin in tests/test_ingest_gpu.py.
"""
import json
import os
import subprocess
import sys

import pytest
import torch

from coda_amd import ops
from coda_amd.datasets import (Dataset, STORAGE_DTYPES, WIRE_DTYPES,
                               make_synthetic_task, read_shard_manifest,
                               resolve_task_path, write_sharded_task,
                               write_synthetic_task)

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bits(t):
    """Bit pattern view, so fp8 / bf16 compare exactly."""
    if t.dtype == torch.float8_e4m3fn:
        return t.view(torch.uint8)
    if t.dtype == torch.bfloat16:
        return t.view(torch.int16)
    return t


def _hand_reference(wire, storage_dt, ens0=None):
    """The contract written out: rounding via torch's CPU conversion, argmax
    as a first-maximum scan, the consensus as an explicit h-ascending loop
    of single fp32 adds."""
    H, N, C = wire.shape
    s = wire.float().to(storage_dt)
    f = s.float()
    classes = torch.empty(H, N, dtype=torch.long)
    for h in range(H):
        for n in range(N):
            row = f[h, n]
            best, at = row[0], 0
            for c in range(1, C):
                if row[c] > best:
                    best, at = row[c], c
            classes[h, n] = at
    ens = torch.zeros(N, C) if ens0 is None else ens0.clone()
    for h in range(H):
        ens = ens + f[h]
    mirror = s.permute(0, 2, 1).contiguous()
    return s, classes, ens, mirror


def _ingest(wire, storage_dt, hc, nc, mirror=True, idxs=None):
    H, N, C = wire.shape
    idxs = list(range(H)) if idxs is None else idxs
    Hl = len(idxs)
    preds = torch.zeros(Hl, N, C).to(storage_dt)
    classes = torch.full((Hl, N), -1, dtype=torch.long)
    ens = torch.zeros(N, C)
    preds_t = torch.zeros(Hl, C, N).to(storage_dt) if mirror else None
    for l0 in range(0, Hl, hc):
        hs = idxs[l0:l0 + hc]
        for n0 in range(0, N, nc):
            ops.ingest_chunk(wire[hs, n0:n0 + nc].contiguous(), l0, n0,
                             preds, classes, ens, preds_t)
    return preds, classes, ens, preds_t


@pytest.mark.parametrize("wire_name", ["fp32", "fp16", "bf16", "fp8"])
@pytest.mark.parametrize("storage", ["fp32", "bf16", "fp8"])
def test_write_read_round_trip(tmp_path, wire_name, storage):
    src, labels = make_synthetic_task(H=5, N=40, C=7, seed=2,
                                      temperature=0.5)
    d = str(tmp_path / "t.shards")
    mpath = write_sharded_task(d, src, wire_name, models_per_shard=2,
                               labels=labels)
    man = read_shard_manifest(d)
    assert (man["H"], man["N"], man["C"]) == (5, 40, 7)
    assert [(s["h0"], s["h1"]) for s in man["shards"]] == \
        [(0, 2), (2, 4), (4, 5)]
    with open(mpath) as f:
        raw = json.load(f)
    assert set(raw) == {"format", "H", "N", "C", "dtype", "shards", "labels"}

    want = src.to(WIRE_DTYPES[wire_name]).float().to(STORAGE_DTYPES[storage])
    for path in (d, mpath):
        ds = Dataset(path, "cpu", storage_dtype=storage)
        assert ds.preds.dtype == STORAGE_DTYPES[storage]
        assert torch.equal(_bits(ds.preds), _bits(want))
        assert torch.equal(ds.labels, labels)
        assert ds.total_models == 5
        assert set(ds.init_stats) == {"classes", "ens_sum", "preds_t"}
        assert torch.equal(ds.init_stats["classes"],
                           want.float().argmax(-1))


def test_writer_accepts_shard_iterator(tmp_path):
    src, _ = make_synthetic_task(H=5, N=20, C=4, seed=1)
    d = str(tmp_path / "it.shards")
    write_sharded_task(d, iter([src[0:3], src[3:5]]), "bf16",
                       models_per_shard=99)
    man = read_shard_manifest(d)
    assert [(s["h0"], s["h1"]) for s in man["shards"]] == [(0, 3), (3, 5)]
    assert man["labels"] is None
    ds = Dataset(d, "cpu", storage_dtype="bf16")
    assert torch.equal(_bits(ds.preds), _bits(src.to(torch.bfloat16)))
    assert ds.labels is None


def _rewrite_manifest(d, edit):
    p = os.path.join(d, "manifest.json")
    with open(p) as f:
        man = json.load(f)
    edit(man)
    with open(p, "w") as f:
        json.dump(man, f)


class TestMalformedManifest:
    @pytest.fixture()
    def task_dir(self, tmp_path):
        src, _ = make_synthetic_task(H=6, N=10, C=3, seed=0)
        d = str(tmp_path / "m.shards")
        write_sharded_task(d, src, "fp16", models_per_shard=2)
        return d

    def test_gap(self, task_dir):
        _rewrite_manifest(task_dir, lambda m: m["shards"].pop(1))
        with pytest.raises(ValueError, match="gap"):
            Dataset(task_dir, "cpu")

    def test_overlap(self, task_dir):
        def edit(m):
            m["shards"][1]["h0"] = 1
        _rewrite_manifest(task_dir, edit)
        with pytest.raises(ValueError, match="overlap"):
            Dataset(task_dir, "cpu")

    def test_short_cover(self, task_dir):
        _rewrite_manifest(task_dir, lambda m: m["shards"].pop())
        with pytest.raises(ValueError, match="H = 6"):
            read_shard_manifest(task_dir)

    def test_bad_dtype(self, task_dir):
        _rewrite_manifest(task_dir, lambda m: m.update(dtype="int8"))
        with pytest.raises(ValueError, match="dtype"):
            Dataset(task_dir, "cpu")

    def test_bad_format(self, task_dir):
        _rewrite_manifest(task_dir,
                          lambda m: m.update(format="coda_amd.shards/9"))
        with pytest.raises(ValueError, match="format"):
            Dataset(task_dir, "cpu")

    def test_shape_mismatch(self, task_dir):
        _rewrite_manifest(task_dir, lambda m: m.update(N=11))
        with pytest.raises(ValueError, match="shape"):
            Dataset(task_dir, "cpu")

    def test_writer_rejects_dtype(self, tmp_path):
        with pytest.raises(ValueError, match="dtype"):
            write_sharded_task(str(tmp_path / "x"), torch.zeros(1, 1, 1),
                               "int8", 1)


def test_convert_script_and_task_resolution(tmp_path):
    data = str(tmp_path / "data")
    out = str(tmp_path / "out")
    write_synthetic_task(data, "syn", H=6, N=50, C=5, seed=4)
    subprocess.run(
        [sys.executable, os.path.join(REPO, "scripts", "convert_task.py"),
         "--task", "syn", "--data-dir", data, "--out-dir", out,
         "--dtype", "fp8", "--shards", "--models-per-shard", "4"],
        check=True, capture_output=True)
    sdir = os.path.join(out, "syn.shards")
    man = read_shard_manifest(sdir)
    assert man["dtype"] == "fp8"
    assert [(s["h0"], s["h1"]) for s in man["shards"]] == [(0, 4), (4, 6)]
    last = torch.load(os.path.join(sdir, man["shards"][-1]["file"]),
                      weights_only=True)
    assert last.shape == (2, 50, 5) and last.dtype == torch.float8_e4m3fn

    src = torch.load(os.path.join(data, "syn.pt"), weights_only=True)
    labels = torch.load(os.path.join(data, "syn_labels.pt"),
                        weights_only=True)
    # only shards present -> the shards; both present -> the .pt
    assert resolve_task_path(out, "syn") == sdir
    ds = Dataset(resolve_task_path(out, "syn"), "cpu", storage_dtype="fp8")
    assert torch.equal(_bits(ds.preds),
                       _bits(src.to(torch.float8_e4m3fn)))
    assert torch.equal(ds.labels, labels)
    os.rename(sdir, os.path.join(data, "syn.shards"))
    assert resolve_task_path(data, "syn") == os.path.join(data, "syn.pt")
    # neither: the .pt path, so the error names the usual file
    assert resolve_task_path(out, "syn") == os.path.join(out, "syn.pt")


def test_main_cli_prefers_pt_then_shards(tmp_path, monkeypatch):
    """main.py --task T: <T>.pt when it exists, <T>.shards only when it
    does not; the sharded task runs the selector end to end."""
    import main as harness
    data = str(tmp_path / "data")
    pt = write_synthetic_task(data, "synthtask", H=6, N=200, C=4, seed=0)
    write_sharded_task(
        os.path.join(data, "synthtask.shards"),
        torch.load(pt, weights_only=True), "bf16", models_per_shard=4,
        labels=torch.load(pt.replace(".pt", "_labels.pt"),
                          weights_only=True))
    opened = []

    class Spy(Dataset):
        def __init__(self, filepath, *a, **k):
            opened.append(filepath)
            super().__init__(filepath, *a, **k)

    monkeypatch.setattr(harness, "Dataset", Spy)
    monkeypatch.chdir(tmp_path)
    argv = ["--task", "synthtask", "--data-dir", "data", "--device", "cpu",
            "--method", "coda", "--iters", "3", "--seeds", "1",
            "--no-mlflow", "--chunk-size", "64"]
    harness.main(argv)
    os.remove(pt)
    harness.main(argv + ["--storage", "bf16"])
    assert opened == [os.path.join("data", "synthtask.pt"),
                      os.path.join("data", "synthtask.shards")]


@pytest.mark.parametrize("wire_name", ["fp32", "fp8"])
def test_host_side_bound(tmp_path, monkeypatch, wire_name):
    """Every chunk reaches the ingest op in the file's dtype, within the
    budget, and the chunks tile [0,H) x [0,N) exactly once."""
    H, N, C = 6, 400, 8
    src, _ = make_synthetic_task(H=H, N=N, C=C, seed=11)
    d = str(tmp_path / "b.shards")
    write_sharded_task(d, src, wire_name, models_per_shard=4)
    esize = torch.empty(0, dtype=WIRE_DTYPES[wire_name]).element_size()
    budget = 150 * C * esize            # < one model (400 points): sub-split
    assert budget < N * C * esize
    calls = []
    real = ops.ingest_chunk

    def spy(wire, h0, n0, *rest):
        calls.append((wire.dtype, tuple(wire.shape),
                      wire.numel() * wire.element_size(), h0, n0))
        return real(wire, h0, n0, *rest)

    monkeypatch.setattr(ops, "ingest_chunk", spy)
    ds = Dataset(d, "cpu", storage_dtype="fp32",
                 stream_chunk_mb=budget / (1 << 20))
    cover = torch.zeros(H, N, dtype=torch.int32)
    assert calls
    for dt, shape, nbytes, h0, n0 in calls:
        assert dt == WIRE_DTYPES[wire_name]
        assert nbytes <= budget
        assert shape[2] == C
        cover[h0:h0 + shape[0], n0:n0 + shape[1]] += 1
    assert any(shape[1] < N for _, shape, _, _, _ in calls)
    assert torch.equal(cover, torch.ones_like(cover))
    assert torch.equal(ds.preds, src.to(WIRE_DTYPES[wire_name]).float())


@pytest.mark.parametrize("wire_name,storage", [
    ("fp32", "fp32"), ("fp32", "bf16"), ("fp32", "fp8"), ("fp16", "fp32"),
    ("bf16", "bf16"), ("fp8", "fp8"), ("bf16", "fp8")])
def test_eager_twin_vs_hand_loop(wire_name, storage):
    src, _ = make_synthetic_task(H=5, N=45, C=9, seed=3, temperature=0.5)
    wire = src.to(WIRE_DTYPES[wire_name])
    sdt = STORAGE_DTYPES[storage]
    s, classes, ens, mirror = _hand_reference(wire, sdt)
    for hc, nc in [(5, 45), (1, 45), (2, 37)]:
        got = _ingest(wire, sdt, hc, nc)
        assert torch.equal(_bits(got[0]), _bits(s))
        assert torch.equal(got[1], classes)
        assert torch.equal(got[2], ens)
        assert torch.equal(_bits(got[3]), _bits(mirror))
    # the mirror is optional; ens_out is advanced, not overwritten
    p2, c2, e2, none = _ingest(wire, sdt, 2, 37, mirror=False)
    assert none is None and torch.equal(c2, classes)
    start = torch.rand(45, 9, generator=torch.Generator().manual_seed(0))
    e3 = start.clone()
    ops.ingest_chunk(wire, 0, 0, torch.empty(5, 45, 9).to(sdt),
                     torch.empty(5, 45, dtype=torch.long), e3)
    assert torch.equal(e3, _hand_reference(wire, sdt, ens0=start)[2])


def test_tie_rule_is_lowest_index():
    wire = torch.tensor([[[0.25, 0.5, 0.5, 0.125], [0.5, 0.25, 0.25, 0.5]]])
    _, classes, _, _ = _ingest(wire, torch.float32, 1, 2)
    assert classes.tolist() == [[1, 0]]


def test_chunking_independence_on_the_loader(tmp_path):
    src, labels = make_synthetic_task(H=6, N=130, C=11, seed=5,
                                      temperature=0.5)
    d = str(tmp_path / "c.shards")
    write_sharded_task(d, src, "bf16", models_per_shard=4, labels=labels)
    per_model = 130 * 11 * 2
    runs = [Dataset(d, "cpu", storage_dtype="fp8",
                    stream_chunk_mb=b / (1 << 20))
            for b in (6 * per_model, per_model, 37 * 11 * 2)]
    for ds in runs[1:]:
        assert torch.equal(_bits(ds.preds), _bits(runs[0].preds))
        for k in ("classes", "ens_sum"):
            assert torch.equal(ds.init_stats[k], runs[0].init_stats[k])


def test_distributed_shard_selection(tmp_path, monkeypatch):
    """shard=(1, 3) ingests exactly models 1 and 4, across shard files."""
    H, N, C = 6, 30, 4
    src, _ = make_synthetic_task(H=H, N=N, C=C, seed=6)
    d = str(tmp_path / "d.shards")
    write_sharded_task(d, src, "fp32", models_per_shard=4)
    seen = []
    real = ops.ingest_chunk

    def spy(wire, h0, n0, *rest):
        seen.append((wire.clone(), h0))
        return real(wire, h0, n0, *rest)

    monkeypatch.setattr(ops, "ingest_chunk", spy)
    ds = Dataset(d, "cpu", shard=(1, 3))
    assert ds.model_idxs.tolist() == [1, 4]
    assert ds.total_models == H
    assert sum(w.shape[0] for w, _ in seen) == 2
    assert torch.equal(ds.preds, src[[1, 4]])
    _, classes, ens, _ = _hand_reference(src[[1, 4]], torch.float32)
    assert torch.equal(ds.init_stats["classes"], classes)
    assert torch.equal(ds.init_stats["ens_sum"], ens)
    # every rank together covers every model once
    all_idx = sorted(sum((Dataset(d, "cpu", shard=(r, 3)).model_idxs.tolist()
                          for r in range(3)), []))
    assert all_idx == list(range(H))


def test_selector_uses_init_stats(tmp_path, monkeypatch):
    """With init_stats present CODA neither recomputes the stats nor differs
    from the legacy route where the consensus order cannot matter (H=2:
    one add either way)."""
    from coda_amd import CODA
    src, labels = make_synthetic_task(H=2, N=60, C=4, seed=7)
    d = str(tmp_path / "s.shards")
    write_sharded_task(d, src, "fp32", models_per_shard=1, labels=labels)
    legacy = CODA(Dataset.from_tensors(src, labels, "cpu"))
    ds = Dataset(d, "cpu")

    def boom(*a, **k):
        raise AssertionError("init_model_stats recomputed")

    monkeypatch.setattr(ops, "init_model_stats", boom)
    sel = CODA(ds)
    assert sel.classes is ds.init_stats["classes"]
    assert torch.equal(sel.classes, legacy.classes)
    assert torch.equal(sel.dirichlets, legacy.dirichlets)
    assert sel._preds_t is None
