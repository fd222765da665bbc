"""Logits tasks on the CPU: the format-2 sharded task, the loader's
temperature plumbing, and the eager twin of the logits ingest
(ops.reference.ingest_chunk with logit_scale) against the fp64 reference
of the contract (tests/ingest_logits_ref.py). The kernel is held to the
same reference, under the same conditions, in
tests/test_ingest_logits_gpu.py.

Conditions on the pool (PARITY.md, L2). Low-precision storage: every
stored element is the storage rounding of the fp64 value or its immediate
neighbour, and at most 1 % of a case's elements differ at all. fp32
storage: relative error at most MARGIN = 16 x E32[case] on the elements
at or above 2^-126, where E32 is the fp32 twin's own error on that case
(re-measured here within a factor 1.5); an element below 2^-126 is 0 or
within the same tolerance x 2^-126, plus one subnormal quantum 2^-149.

Mutation floors: four faults applied to the fp64 reference must each
exceed these tolerances. The partial maximum is the odd one: a softmax
does not depend on what is subtracted before exp2 until exp2 overflows,
which is all the maximum is there to prevent. So that floor runs on
logits whose classes from 64 on are raised by 1000 (x k >= 1024 at T = 1,
the fp64 overflow), where a maximum over the first 64 classes gives
inf / inf; on the N(0, 4^2) input it moves the fp64 result by 1e-15.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from coda_amd import ops
from coda_amd.datasets import (Dataset, SHARD_FORMAT, SHARD_FORMAT_LOGITS,
                               make_synthetic_task, read_shard_manifest,
                               write_sharded_task)
from coda_amd.ops import reference
from tests import ingest_logits_ref as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FEW_PAIRS = [("fp16", "fp32"), ("bf16", "fp8")]
CASES = ([(R.SHAPES[0], (w, s)) for w in R.WIRES for s in R.STORAGES]
         + [(s, p) for s in R.SHAPES[1:] for p in FEW_PAIRS])
IDS = [f"{s[0]}x{s[1]}x{s[2]}-{p[0]}-{p[1]}" for s, p in CASES]


def _bits(t):
    return t if t.dtype == torch.float32 else R.ordinal(t)


def _ingest(x, k, storage, hc, nc, fn=ops.ingest_chunk):
    H, N, C = x.shape
    sdt = R.DT[storage]
    preds = torch.zeros(H, N, C).to(sdt)
    classes = torch.full((H, N), -1, dtype=torch.long)
    ens = torch.zeros(N, C)
    preds_t = torch.zeros(H, C, N).to(sdt)
    for h0 in range(0, H, hc):
        for n0 in range(0, N, nc):
            fn(x[h0:h0 + hc, n0:n0 + nc].contiguous(), h0, n0, preds,
               classes, ens, preds_t, k[h0:h0 + hc])
    return preds, classes, ens, preds_t


def _logit_task(tmp_path, H=6, N=50, C=9, dtype="fp16", **kw):
    g = torch.Generator().manual_seed(4)
    x = torch.randn(H, N, C, generator=g) * 4.0
    labels = torch.randint(0, C, (N,), generator=g)
    d = str(tmp_path / "t.shards")
    write_sharded_task(d, x, dtype, models_per_shard=4, labels=labels,
                       kind="logits", **kw)
    return x.to(R.DT[dtype]), labels, d


# ---------------------------------------------------------------- format

def test_format2_round_trip(tmp_path):
    temps = [0.37, 2.5, 1.0, 0.8, 1.7, 3.0]
    x, labels, d = _logit_task(tmp_path, temperature=temps)
    man = read_shard_manifest(d)
    assert man["format"] == SHARD_FORMAT_LOGITS == "coda_amd.shards/2"
    assert man["kind"] == "logits" and man["temperature"] == temps
    assert man["dtype"] == "fp16" and len(man["shards"]) == 2
    ds = Dataset(d, "cpu", storage_dtype="bf16", stream_chunk_mb=0.001)
    assert ds.kind == "logits" and ds.temperature.tolist() == temps
    assert torch.equal(ds.labels, labels)
    want = _ingest(x, R.logit_scale(temps), "bf16", 6, 50,
                   fn=reference.ingest_chunk)
    assert torch.equal(_bits(ds.preds), _bits(want[0]))
    assert torch.equal(ds.init_stats["classes"], want[1])
    assert torch.equal(ds.init_stats["ens_sum"], want[2])
    soft = torch.softmax(x.float() / torch.tensor(temps).view(6, 1, 1), -1)
    torch.testing.assert_close(ds.preds.float(), soft, rtol=2 ** -7,
                               atol=1e-30)
    # a load-time temperature overrides the manifest's; scalar broadcasts
    ds2 = Dataset(d, "cpu", storage_dtype="bf16", temperature=2.0)
    soft2 = torch.softmax(x.float() / 2.0, -1)
    torch.testing.assert_close(ds2.preds.float(), soft2, rtol=2 ** -7,
                               atol=1e-30)
    # no temperature anywhere means 1
    (tmp_path / "u").mkdir()
    _, _, d1 = _logit_task(tmp_path / "u")
    assert "temperature" not in json.load(open(os.path.join(
        d1, "manifest.json")))
    assert Dataset(d1, "cpu").temperature.tolist() == [1.0] * 6


def test_format2_is_unknown_to_a_format1_reader(tmp_path):
    _, _, d = _logit_task(tmp_path)
    with pytest.raises(ValueError, match="unknown format"):
        read_shard_manifest(d, formats=(SHARD_FORMAT,))


PARENT_MANIFEST = """{
 "format": "coda_amd.shards/1",
 "H": 3,
 "N": 4,
 "C": 5,
 "dtype": "bf16",
 "shards": [
  {
   "file": "h000000-000002.pt",
   "h0": 0,
   "h1": 2
  },
  {
   "file": "h000002-000003.pt",
   "h0": 2,
   "h1": 3
  }
 ],
 "labels": "labels.pt"
}"""


def test_probability_task_bytes_unchanged(tmp_path):
    """What the writer wrote before logits existed: this manifest text
    (json.dump, indent=1, these keys in this order) and, per shard,
    torch.save of the converted contiguous clone."""
    p, labels = make_synthetic_task(H=3, N=4, C=5, seed=1)
    d = str(tmp_path / "p.shards")
    for kw in ({}, {"kind": "probs"}):
        write_sharded_task(d, p, "bf16", models_per_shard=2, labels=labels,
                           **kw)
        assert open(os.path.join(d, "manifest.json")).read() \
            == PARENT_MANIFEST
        for name, a, b in (("h000000-000002.pt", 0, 2),
                           ("h000002-000003.pt", 2, 3)):
            # same file name: torch.save records it inside the archive
            os.makedirs(str(tmp_path / "ref"), exist_ok=True)
            ref = str(tmp_path / "ref" / name)
            torch.save(p[a:b].float().to(torch.bfloat16).contiguous()
                       .clone(), ref)
            got = open(os.path.join(d, name), "rb").read()
            assert got == open(ref, "rb").read(), name
    man = read_shard_manifest(d)
    assert man["kind"] == "probs" and man["temperature"] is None


def test_fp8_logits_refused(tmp_path):
    x = torch.randn(2, 3, 4)
    with pytest.raises(ValueError, match="fp8"):
        write_sharded_task(str(tmp_path / "a.shards"), x, "fp8",
                           kind="logits")
    _, _, d = _logit_task(tmp_path)
    mpath = os.path.join(d, "manifest.json")
    man = json.load(open(mpath))
    man["dtype"] = "fp8"
    json.dump(man, open(mpath, "w"))
    with pytest.raises(ValueError, match="fp8"):
        read_shard_manifest(d)
    with pytest.raises(ValueError, match="fp8"):
        Dataset(d, "cpu")
    with pytest.raises(ValueError, match="wire dtype"):
        z = torch.zeros(1, 2, 3)
        ops.ingest_chunk(z.to(R.F8), 0, 0, z.clone(),
                         torch.zeros(1, 2, dtype=torch.long),
                         torch.zeros(2, 3), None, torch.ones(1))


@pytest.mark.parametrize("bad", ["nan", "+inf", "all -inf row", "fp16 overflow"])
def test_bad_logits_refused_at_write(tmp_path, bad):
    x = torch.randn(5, 6, 7)
    x[0, 0, 0] = float("-inf")               # allowed
    d = str(tmp_path / "ok.shards")
    write_sharded_task(d, x, "fp16", models_per_shard=2, kind="logits")
    assert float(Dataset(d, "cpu").preds[0, 0, 0]) == 0.0
    if bad == "nan":
        x[3, 2, 1] = float("nan")
    elif bad == "+inf":
        x[3, 2, 1] = float("inf")
    elif bad == "fp16 overflow":
        x[3, 2, 1] = 1e6                      # inf once in the wire dtype
    else:
        x[3, 2] = float("-inf")
    with pytest.raises(ValueError, match=r"shard h000002-000004\.pt"):
        write_sharded_task(str(tmp_path / "bad.shards"), x, "fp16",
                           models_per_shard=2, kind="logits")


@pytest.mark.parametrize("bad", [0, -1.0, float("nan"), float("inf"),
                                 [1.0, 2.0], "1", True])
def test_bad_temperature_refused(tmp_path, bad):
    x = torch.randn(3, 4, 5)
    with pytest.raises(ValueError, match="temperature"):
        write_sharded_task(str(tmp_path / "a.shards"), x, "fp32",
                           kind="logits", temperature=bad)
    (tmp_path / "b").mkdir()
    _, _, d = _logit_task(tmp_path / "b", H=3)
    with pytest.raises(ValueError, match="temperature"):
        Dataset(d, "cpu", temperature=bad)
    mpath = os.path.join(d, "manifest.json")
    man = json.load(open(mpath))
    man["temperature"] = bad
    json.dump(man, open(mpath, "w"))
    with pytest.raises(ValueError, match="temperature"):
        read_shard_manifest(d)


def test_temperature_on_a_probability_task_refused(tmp_path):
    p, labels = make_synthetic_task(H=3, N=4, C=5, seed=1)
    d = str(tmp_path / "p.shards")
    write_sharded_task(d, p, "fp16")
    with pytest.raises(ValueError, match="temperature"):
        Dataset(d, "cpu", temperature=2.0)
    with pytest.raises(ValueError, match="temperature"):
        write_sharded_task(d, p, "fp16", temperature=2.0)
    pt = str(tmp_path / "p.pt")
    torch.save(p, pt)
    with pytest.raises(ValueError, match="temperature"):
        Dataset(pt, "cpu", temperature=2.0)
    # and a format-1 manifest cannot smuggle logits in
    mpath = os.path.join(d, "manifest.json")
    man = json.load(open(mpath))
    man["kind"] = "logits"
    json.dump(man, open(mpath, "w"))
    with pytest.raises(ValueError, match="kind"):
        read_shard_manifest(d)


def test_shard_picks_global_temperatures(tmp_path):
    temps = [0.37, 2.5, 1.0, 0.8, 1.7, 3.0]
    _, _, d = _logit_task(tmp_path, temperature=temps)
    full = Dataset(d, "cpu")

    # torch's vectorised exp2 is not the same number in every chunk shape
    def same(a, b):
        return bool(torch.isclose(a, b, rtol=1e-5, atol=1e-30).all())

    for rank in (0, 1):
        part = Dataset(d, "cpu", shard=(rank, 2), stream_chunk_mb=0.002)
        assert part.model_idxs.tolist() == list(range(rank, 6, 2))
        assert part.temperature.tolist() == temps
        assert same(part.preds, full.preds[rank::2])
    # the odd models' temperatures matter: move one and rank 1 changes
    moved = list(temps)
    moved[3] = 5.0
    odd = Dataset(d, "cpu", shard=(1, 2), temperature=moved)
    assert same(odd.preds[0], full.preds[1])
    assert not same(odd.preds[1], full.preds[3])
    assert same(odd.preds[2], full.preds[5])
    even = Dataset(d, "cpu", shard=(0, 2), temperature=moved)
    assert same(even.preds, full.preds[0::2])


def test_loader_refuses_non_finite_probabilities(tmp_path):
    """A file our writer never checked: written as probabilities, then
    relabelled as logits by hand."""
    x = torch.randn(3, 4, 5)
    x[1, 2, 3] = float("nan")
    d = str(tmp_path / "n.shards")
    write_sharded_task(d, x, "fp32")
    mpath = os.path.join(d, "manifest.json")
    man = json.load(open(mpath))
    man["format"], man["kind"] = SHARD_FORMAT_LOGITS, "logits"
    json.dump(man, open(mpath, "w"))
    with pytest.raises(ValueError, match="non-finite probabilities from a "
                                         "logits task"):
        Dataset(d, "cpu")


def test_cli_kind_and_temperature(tmp_path, monkeypatch):
    g = torch.Generator().manual_seed(0)
    x = torch.randn(4, 30, 6, generator=g) * 4
    data = tmp_path / "data"
    data.mkdir()
    torch.save(x, str(data / "zoo.pt"))
    torch.save(torch.randint(0, 6, (30,), generator=g),
               str(data / "zoo_labels.pt"))
    out = tmp_path / "out"
    conv = [sys.executable, os.path.join(REPO, "scripts", "convert_task.py"),
            "--task", "zoo", "--data-dir", str(data), "--out-dir", str(out),
            "--dtype", "fp16"]
    r = subprocess.run(conv + ["--kind", "logits"], capture_output=True,
                       text=True)
    assert r.returncode != 0 and "--shards" in r.stderr
    r = subprocess.run(conv + ["--shards", "--kind", "logits",
                               "--temperature", "2.0"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    man = read_shard_manifest(str(out / "zoo.shards"))
    assert man["kind"] == "logits" and man["temperature"] == 2.0
    ds = Dataset(str(out / "zoo.shards"), "cpu")
    torch.testing.assert_close(ds.preds,
                               torch.softmax(x.half().float() / 2.0, -1),
                               rtol=1e-4, atol=1e-7)
    import main as harness
    monkeypatch.chdir(tmp_path)
    argv = ["--task", "zoo", "--method", "iid", "--iters", "2", "--seeds",
            "1", "--no-mlflow", "--device", "cpu", "--temperature", "0.5"]
    seen = []

    class Spy(Dataset):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            seen.append(self.temperature.tolist())

    monkeypatch.setattr(harness, "Dataset", Spy)
    harness.main(argv + ["--data-dir", str(out)])
    assert seen == [[0.5] * 4]
    # the .pt in `data` holds probabilities as far as anyone can tell
    with pytest.raises(ValueError, match="temperature"):
        harness.main(argv + ["--data-dir", str(data)])


# ------------------------------------------------- eager twin vs fp64

@pytest.mark.parametrize("tset", R.TEMP_SETS)
@pytest.mark.parametrize("shape,pair", CASES, ids=IDS)
def test_eager_twin_matches_fp64(shape, pair, tset):
    wire, storage = pair
    x = R.logits(shape, wire)
    k = R.logit_scale(R.temperatures(shape[0], tset))
    p64 = R.ref64(x, k)
    if storage == "fp8" and shape[2] >= 64:
        s = R.round_storage(p64, storage).float()
        assert ((s > 0) & (s < 2.0 ** -6)).float().mean() > 0.02
        assert (s == 0).float().mean() > 0.25, "tails do not underflow"
    whole = _ingest(x, k, storage, shape[0], shape[1])
    R.check_pool(whole[0], p64, shape, wire, storage, tset, "eager")
    f = whole[0].float()
    assert torch.equal(whole[1], f.argmax(-1))
    ens = torch.zeros(shape[1], shape[2])
    for h in range(shape[0]):
        ens = ens + f[h]
    assert torch.equal(whole[2], ens)
    assert torch.equal(_bits(whole[3]), _bits(whole[0].permute(0, 2, 1)))
    parts = _ingest(x, k, storage, 2, 37)
    R.check_pool(parts[0], p64, shape, wire, storage, tset, "eager 2x37")
    assert torch.equal(parts[1], parts[0].float().argmax(-1))


@pytest.mark.parametrize("case", R.f32_cases(),
                         ids=lambda c: f"{c[0][0]}x{c[0][1]}x{c[0][2]}-"
                                       f"{c[1]}-{c[2]}")
def test_e32_table_re_measured(case):
    e = R.measure_e32(*case)
    print(f"{case}: twin {e:.3e} recorded {R.E32[case]:.3e}")
    assert R.E32[case] / 1.5 <= e <= R.E32[case] * 1.5


def test_fp64_storage_rounding_is_direct():
    """round_storage rounds once; through fp32 a value just above a bf16
    midpoint lands on the midpoint and goes the other way."""
    v = np.array([0.5 + 2.0 ** -9 + 2.0 ** -40])
    assert float(R.round_storage(v, "bf16")) == 0.5 + 2.0 ** -8
    assert float(torch.from_numpy(v).float().to(torch.bfloat16)) == 0.5
    for st in ("fp16", "bf16", "fp8"):
        g = torch.rand(4000, generator=torch.Generator().manual_seed(1)) \
            ** 8
        assert torch.equal(_bits(R.round_storage(g.double().numpy(), st)),
                           _bits(g.to(R.DT[st])))


# ------------------------------------------------------ mutation floors

def _exceeds(p_bad, p64, shape, tset):
    """Would the faulty pool fail the fp32 condition, and the bf16 one?"""
    tol = R.MARGIN * R.E32[(shape, "fp16", tset)]
    rel, sub = R.f32_error(p_bad, p64)
    f32_fails = not (rel <= tol and sub <= tol + 2.0 ** -23)
    if not np.isfinite(p_bad).all():
        return f32_fails, True
    dist, frac = R.lowp_mismatch(
        R.round_storage(np.clip(p_bad, 0, 1), "bf16"), p64, "bf16")
    return f32_fails, not (dist <= 1 and frac <= 0.01)


@pytest.mark.parametrize("shape", R.SHAPES[:4],
                         ids=lambda s: f"{s[0]}x{s[1]}x{s[2]}")
@pytest.mark.parametrize("fault", ["k_model0", "drop_last_z", "shared_tile"])
def test_mutation_floor(shape, fault):
    x = R.logits(shape, "fp16")
    k = R.logit_scale(R.temperatures(shape[0], "vec"))
    p64 = R.ref64(x, k)
    kw = {"k_model0": {"k_model0": True},
          "drop_last_z": {"drop_last_z": True},
          "shared_tile": {"shared_tile": R.tile_points(shape[1], shape[2])},
          }[fault]
    bad = R.ref64(x, k, **kw)
    assert _exceeds(bad, p64, shape, "vec") == (True, True)


@pytest.mark.parametrize("shape", [R.SHAPES[0], R.SHAPES[2]],
                         ids=["5x130x67", "2x65x1001"])
def test_mutation_floor_partial_max(shape):
    """Module docstring: invisible on the N(0, 4^2) input, inf / inf once
    the true maximum is 1000 above the first 64 classes."""
    k = R.logit_scale(R.temperatures(shape[0], "ones"))
    x = R.logits(shape, "fp16")
    moved = np.abs(R.ref64(x, k, max_first=64) / R.ref64(x, k) - 1).max()
    print(f"partial max on the plain input: rel {moved:.2e}")
    assert moved < 1e-12
    x = R.logits(shape, "fp16", offset=1000.0)
    p64 = R.ref64(x, k)
    assert np.isfinite(p64).all()
    bad = R.ref64(x, k, max_first=64)
    assert _exceeds(bad, p64, shape, "ones") == (True, True)
    # the eager twin takes the whole-row maximum; |t| reaches 1443 here,
    # so the tolerance is 16 x the twin's error on this very input
    got = _ingest(x, k, "fp32", shape[0], shape[1])[0]
    rel, sub = R.f32_error(got, p64)
    e32 = R.f32_error(R.twin32(x, k), p64)[0]
    print(f"offset input: eager rel {rel:.3e}, twin {e32:.3e}")
    assert rel <= R.MARGIN * e32 and sub <= R.MARGIN * e32 + 2.0 ** -23


# ------------------------------------------------ ties and -inf entries

@pytest.mark.parametrize("wire,storage", [("fp32", "fp32"), ("fp16", "fp16"),
                                          ("bf16", "fp8")])
@pytest.mark.parametrize("shape", [R.SHAPES[0], R.SHAPES[2]],
                         ids=["5x130x67", "2x65x1001"])
def test_tie_rule_binds(shape, wire, storage):
    x, a, b = R.crafted_ties(shape, wire)
    k = R.logit_scale(R.temperatures(shape[0], "vec"))
    for hc, nc in ((shape[0], shape[1]), (2, 37)):
        preds, classes, _, _ = _ingest(x, k, storage, hc, nc)
        R.check_ties(preds, classes, a, b)


@pytest.mark.parametrize("wire,storage", [("fp32", "fp32"), ("fp16", "bf16"),
                                          ("bf16", "fp8")])
def test_neg_inf_gives_exact_zero(wire, storage):
    shape = R.SHAPES[0]
    x, hole = R.with_neg_inf(shape, wire)
    k = R.logit_scale(R.temperatures(shape[0], "vec"))
    preds, classes, ens, _ = _ingest(x, k, storage, 2, 37)
    assert bool((preds.float()[hole] == 0).all())
    assert bool(torch.isfinite(ens).all())
    assert not bool(hole.gather(2, classes.unsqueeze(-1)).any())
    p64 = R.ref64(x, k)
    assert bool((torch.from_numpy(p64)[hole] == 0).all())
    if storage != "fp32":
        dist, frac = R.lowp_mismatch(preds, p64, storage)
        assert dist <= 1 and frac <= 0.01
