"""GPU tests of the logits ingest kernel (coda_amd/ops/hip/ingest_logits.hip).

What is exact is compared exactly, on the kernel's OWN stored pool: the
classes are its lowest-index argmax, the consensus the h-ascending fp32
sum of its decoded values, the mirror its permutation; two runs and two
chunkings give the same bits. The pool itself is held to the fp64
reference of the contract (tests/ingest_logits_ref.py) under the
conditions of PARITY.md (L2): low-precision storage - the storage
rounding of the fp64 value or its immediate neighbour, at most 1 % of a
case's elements differing at all; fp32 storage - relative error at most
16 x the fp32 twin's own error E32 on the elements >= 2^-126, elements
below stored as 0 or within that tolerance x 2^-126 (+ 2^-149).

E32 per fp32-storage case (twin vs fp64, re-measured on the CPU by
tests/test_ingest_logits.py; tolerance = 16 x), at T = 1 and at
T = (0.37, 2.5, 1.0, 0.8, 1.7)[:H]:

| shape         | wire | E32 T=1  | E32 T vec |
|---------------|------|----------|-----------|
| (5, 130, 67)  | fp32 | 2.28e-06 | 5.20e-06  |
| (5, 130, 67)  | fp16 | 1.40e-06 | 2.74e-06  |
| (5, 130, 67)  | bf16 | 1.37e-06 | 2.70e-06  |
| (3, 70, 3)    | fp16 | 7.04e-07 | 1.31e-06  |
| (2, 65, 1001) | fp16 | 1.53e-06 | 3.80e-06  |
| (4, 128, 64)  | fp16 | 1.43e-06 | 2.76e-06  |
| (1, 1, 5)     | fp16 | 4.78e-07 | 1.19e-06  |

Measured on an MI355X: the kernel's worst relative error equals the
twin's entry to the four digits printed in all 14 cases (the worst
element's error is the fp32 rounding of t = (x - m) * k, which twin and
kernel share; the hardware exp2 adds nothing visible on top), and no
element below 2^-126 was stored non-zero. Low-precision storage: ordinal
distance at most 1, 0 to 0.021 % of a case's elements differing (fp8: 0
in every case).

Shapes are those of tests/test_ingest_gpu.py, for its reasons: odd C
(scalar path) with a ragged last tile; C below a wave; many lane strides
with an odd C; the vector path; a single point.
"""
import random

import pytest
import torch

from tests import ingest_logits_ref as R

pytestmark = pytest.mark.gpu

FEW_PAIRS = [("fp16", "fp32"), ("bf16", "fp8")]
CASES = ([(R.SHAPES[0], (w, s)) for w in R.WIRES for s in R.STORAGES]
         + [(s, p) for s in R.SHAPES[1:] for p in FEW_PAIRS])
IDS = [f"{s[0]}x{s[1]}x{s[2]}-{p[0]}-{p[1]}" for s, p in CASES]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module", autouse=True)
def _require_ext():
    import coda_amd.ops as ops
    assert ops.hip_available(), \
        "HIP extension must be built on GPU boxes (python build_hip.py)"


def _bits(t):
    return t if t.dtype == torch.float32 else R.ordinal(t)


def _ens_start(N, C):
    return torch.rand(N, C, generator=torch.Generator().manual_seed(1))


def _run_gpu(dev, x, k, storage, hc, nc, mirror=True, misalign=False):
    """Ingest logits x on the GPU in (hc, nc) chunks into garbage-filled
    outputs; everything comes back on the CPU."""
    from coda_amd import ops
    H, N, C = x.shape
    sdt = R.DT[storage]
    esz = torch.empty(0, dtype=sdt).element_size()
    preds = torch.full((H * N * C * esz,), 0x55, dtype=torch.uint8,
                       device=dev).view(sdt).view(H, N, C)
    classes = torch.full((H, N), -7, dtype=torch.long, device=dev)
    ens = _ens_start(N, C).to(dev)
    preds_t = (torch.full((H * C * N * esz,), 0x55, dtype=torch.uint8,
                          device=dev).view(sdt).view(H, C, N)
               if mirror else None)
    kd = k.to(dev)
    for h0 in range(0, H, hc):
        for n0 in range(0, N, nc):
            chunk = x[h0:h0 + hc, n0:n0 + nc].contiguous()
            if misalign:
                # contiguous, but starting one element into its buffer
                buf = torch.empty(chunk.numel() + 1, dtype=chunk.dtype,
                                  device=dev)
                buf[1:].copy_(chunk.reshape(-1))
                wire = buf[1:].view(chunk.shape)
                assert wire.data_ptr() % 16 != 0
            else:
                wire = chunk.to(dev)
            ops.ingest_chunk(wire, h0, n0, preds, classes, ens, preds_t,
                             kd[h0:h0 + hc])
    torch.cuda.synchronize(dev)
    return (preds.cpu(), classes.cpu(), ens.cpu(),
            preds_t.cpu() if mirror else None)


def _assert_exact_on_own_pool(got, mirror=True):
    preds, classes, ens, preds_t = got
    H, N, C = preds.shape
    f = preds.float()
    assert bool(torch.isfinite(f).all())
    assert torch.equal(classes, f.argmax(-1)), "classes_out"
    want = _ens_start(N, C)
    for h in range(H):
        want = want + f[h]
    assert torch.equal(ens, want), "ens_out"
    if mirror:
        assert torch.equal(_bits(preds_t),
                           _bits(preds.permute(0, 2, 1).contiguous()))
    else:
        assert preds_t is None


def _assert_same_bits(a, b):
    assert torch.equal(_bits(a[0]), _bits(b[0])), "preds_out"
    assert torch.equal(a[1], b[1]), "classes_out"
    assert torch.equal(a[2], b[2]), "ens_out"
    if a[3] is not None and b[3] is not None:
        assert torch.equal(_bits(a[3]), _bits(b[3])), "preds_t_out"


@pytest.mark.parametrize("tset", R.TEMP_SETS)
@pytest.mark.parametrize("shape,pair", CASES, ids=IDS)
def test_kernel_outputs(dev, shape, pair, tset):
    wire, storage = pair
    x = R.logits(shape, wire)
    k = R.logit_scale(R.temperatures(shape[0], tset))
    whole = _run_gpu(dev, x, k, storage, shape[0], shape[1])
    R.check_pool(whole[0], R.ref64(x, k), shape, wire, storage, tset,
                 "kernel")
    _assert_exact_on_own_pool(whole)
    again = _run_gpu(dev, x, k, storage, shape[0], shape[1])
    _assert_same_bits(whole, again)
    parts = _run_gpu(dev, x, k, storage, 2, 37, mirror=False)
    _assert_exact_on_own_pool(parts, mirror=False)
    _assert_same_bits(whole, parts)


@pytest.mark.parametrize("pair", [("fp32", "bf16"), ("fp16", "fp32")],
                         ids=["fp32-bf16", "fp16-fp32"])
def test_misaligned_wire_takes_the_scalar_path(dev, pair):
    """C % 4 == 0 but the wire buffer is not 16-byte aligned. The sum of
    the exponentials runs in the same lane order on both paths, so the
    scalar path gives the vector path's bits."""
    wire, storage = pair
    shape = R.SHAPES[3]
    x = R.logits(shape, wire)
    k = R.logit_scale(R.temperatures(shape[0], "vec"))
    got = _run_gpu(dev, x, k, storage, 2, 37, misalign=True)
    p64 = R.ref64(x, k)
    if storage == "fp32":
        assert wire == "fp16"            # the E32 table's wire
        R.check_pool(got[0], p64, shape, wire, storage, "vec", "misaligned")
    else:
        dist, frac = R.lowp_mismatch(got[0], p64, storage)
        print(f"misaligned {wire}->{storage}: ordinal distance {dist}, "
              f"differing {frac:.3%}")
        assert dist <= 1 and frac <= 0.01
    _assert_exact_on_own_pool(got)
    _assert_same_bits(got, _run_gpu(dev, x, k, storage, 2, 37))


@pytest.mark.parametrize("wire,storage", [("fp32", "fp32"), ("fp16", "fp16"),
                                          ("bf16", "fp8")])
@pytest.mark.parametrize("shape", [R.SHAPES[0], R.SHAPES[2]],
                         ids=["5x130x67", "2x65x1001"])
def test_tie_rule_binds(dev, shape, wire, storage):
    """Crafted logits, one case per wire dtype: every row has its maximum
    at two or more classes. exp2(0) == 1 at each of them, so the stored
    values tie and the lowest index wins."""
    x, a, b = R.crafted_ties(shape, wire)
    k = R.logit_scale(R.temperatures(shape[0], "vec"))
    for hc, nc in ((shape[0], shape[1]), (2, 37)):
        got = _run_gpu(dev, x, k, storage, hc, nc)
        R.check_ties(got[0], got[1], a, b)
        _assert_exact_on_own_pool(got)


@pytest.mark.parametrize("wire,storage", [("fp32", "fp32"), ("fp16", "bf16"),
                                          ("bf16", "fp8")])
def test_neg_inf_gives_exact_zero(dev, wire, storage):
    shape = R.SHAPES[0]
    x, hole = R.with_neg_inf(shape, wire)
    k = R.logit_scale(R.temperatures(shape[0], "vec"))
    got = _run_gpu(dev, x, k, storage, 2, 37)
    assert bool((got[0].float()[hole] == 0).all())
    _assert_exact_on_own_pool(got)
    if storage != "fp32":
        dist, frac = R.lowp_mismatch(got[0], R.ref64(x, k), storage)
        assert dist <= 1 and frac <= 0.01


@pytest.mark.parametrize("shape", [R.SHAPES[0], R.SHAPES[2]],
                         ids=["5x130x67", "2x65x1001"])
def test_max_spans_every_lane_stride(dev, shape):
    """Classes from 64 on raised by 1000: a maximum taken over the first
    lane stride alone would overflow exp2. |t| reaches 1443 here, so the
    fp32 tolerance is 16 x the twin's error on this very input."""
    x = R.logits(shape, "fp16", offset=1000.0)
    k = R.logit_scale(R.temperatures(shape[0], "ones"))
    p64 = R.ref64(x, k)
    got = _run_gpu(dev, x, k, "fp32", shape[0], shape[1])
    rel, sub = R.f32_error(got[0], p64)
    e32 = R.f32_error(R.twin32(x, k), p64)[0]
    print(f"offset input {shape}: kernel rel {rel:.3e} sub {sub:.3e}, "
          f"twin {e32:.3e}")
    assert rel <= R.MARGIN * e32 and sub <= R.MARGIN * e32 + 2.0 ** -23
    _assert_exact_on_own_pool(got)


def test_rejects_bad_logit_scale(dev):
    """Checked on the host before anything is launched."""
    from coda_amd import ops
    H, N, C = 2, 10, 4
    preds = torch.zeros(H, N, C, device=dev)
    classes = torch.zeros(H, N, dtype=torch.long, device=dev)
    ens = torch.zeros(N, C, device=dev)
    wire = torch.zeros(2, 5, C, device=dev)
    k = torch.ones(2, device=dev)
    for bad in (torch.ones(3, device=dev), torch.ones(2),
                torch.ones(2, device=dev, dtype=torch.float64),
                torch.ones(2, 1, device=dev)):
        with pytest.raises(ValueError, match="logit_scale"):
            ops.ingest_chunk(wire, 0, 0, preds, classes, ens, None, bad)
    with pytest.raises(ValueError, match="wire dtype"):
        ops.ingest_chunk(wire.to(R.F8), 0, 0, preds, classes, ens, None, k)
    for h0, n0 in [(1, 0), (0, 6), (-1, 0)]:
        with pytest.raises(RuntimeError, match="outside"):
            ops.ingest_chunk(wire, h0, n0, preds, classes, ens, None, k)
    torch.cuda.synchronize(dev)
    assert not bool(preds.any()) and not bool(ens.any())


@pytest.fixture(scope="module")
def logit_dirs(tmp_path_factory):
    """Logits whose softmax at T = 1 is make_synthetic_task's pool."""
    from coda_amd.datasets import make_synthetic_task, write_sharded_task
    preds, labels = make_synthetic_task(H=6, N=400, C=8, seed=11)
    x = preds.log()
    root = tmp_path_factory.mktemp("ingest_logits")
    d = str(root / "t.shards")
    write_sharded_task(d, x, "fp16", models_per_shard=4, labels=labels,
                       kind="logits")
    return x.half(), labels, d


@pytest.mark.parametrize("storage", ["bf16", "fp8"])
def test_end_to_end_matches_in_memory_route(dev, logit_dirs, storage,
                                            monkeypatch):
    """CODA on a logits sharded task, init_stats from the ingest, == CODA
    via from_tensors on the pool the loader produced. Assertions and
    tolerances of tests/test_ingest_gpu.py's test of the same name: the
    consensus argmax is first shown to be safe (smallest top-2 margin of
    the fp64 consensus > 100 x the fp32 summation bound), get_pbest is
    compared at rtol=1e-5, atol=1e-7."""
    from coda_amd import CODA, Oracle, ops
    from coda_amd.datasets import Dataset
    from coda_amd.options import LOSS_FNS
    x, labels, d = logit_dirs
    H = x.shape[0]
    budget = 150 * 8 * 2 / (1 << 20)     # sub-splits every model along n
    ds_a = Dataset(d, dev, storage_dtype=storage, stream_chunk_mb=budget)
    assert ds_a.kind == "logits"
    stored = ds_a.preds.cpu()
    dist, frac = R.lowp_mismatch(stored, R.ref64(x, R.logit_scale([1.0] * H)),
                                 storage)
    assert dist <= 1 and frac <= 0.01
    cons = stored.double().sum(0)                       # (N, C) fp64
    top2 = cons.topk(2, dim=-1).values
    margin = float((top2[:, 0] - top2[:, 1]).min())
    bound = 100 * (H - 1) * 2.0 ** -24 * float(cons.abs().max())
    print(f"consensus top-2 margin {margin:.3e} vs bound {bound:.3e}")
    assert margin > bound, "pick another seed: consensus argmax not safe"

    ds_b = Dataset.from_tensors(stored, labels, dev)
    assert torch.equal(_bits(ds_a.preds), _bits(ds_b.preds))
    assert torch.equal(ds_a.labels, ds_b.labels)
    random.seed(0); torch.manual_seed(0)
    sel_b = CODA(ds_b, chunk_size=64)

    def boom(*a, **k):
        raise AssertionError("init_model_stats recomputed")
    monkeypatch.setattr(ops, "init_model_stats", boom)
    random.seed(0); torch.manual_seed(0)
    sel_a = CODA(ds_a, chunk_size=64)
    monkeypatch.undo()

    assert torch.equal(sel_a.classes, sel_b.classes)
    assert torch.equal(sel_a.dirichlets, sel_b.dirichlets)
    assert (sel_a._preds_t is None) == (sel_b._preds_t is None)
    if sel_a._preds_t is not None:
        assert sel_a._preds_t is ds_a.init_stats["preds_t"]
        assert torch.equal(_bits(sel_a._preds_t), _bits(sel_b._preds_t))

    oracle = Oracle(ds_b, LOSS_FNS["acc"])
    for _ in range(3):
        idx, q = sel_b.get_next_item_to_label()
        y = oracle(int(idx))
        sel_b.add_label(idx, y, q)
        sel_a.add_label(idx, y, q)
    torch.testing.assert_close(sel_a.get_pbest(), sel_b.get_pbest(),
                               rtol=1e-5, atol=1e-7)


def test_temperature_reaches_the_selector(dev, logit_dirs):
    """T = 0.37 sharpens every model: another pool, another consensus,
    other Dirichlet priors in the selector."""
    from coda_amd import CODA
    from coda_amd.datasets import Dataset
    _, _, d = logit_dirs
    ds_1 = Dataset(d, dev, storage_dtype="bf16")
    ds_t = Dataset(d, dev, storage_dtype="bf16", temperature=0.37)
    e1, et = ds_1.init_stats["ens_sum"], ds_t.init_stats["ens_sum"]
    assert not torch.equal(e1, et)
    # sharper rows: the consensus' largest entry per point grows
    assert float((et.max(-1).values - e1.max(-1).values).mean()) > 0.1
    torch.testing.assert_close(et.sum(-1), e1.sum(-1), rtol=2e-2, atol=0)
    random.seed(0); torch.manual_seed(0)
    sel_1 = CODA(ds_1, chunk_size=64)
    random.seed(0); torch.manual_seed(0)
    sel_t = CODA(ds_t, chunk_size=64)
    assert not torch.equal(sel_1.dirichlets, sel_t.dirichlets)
