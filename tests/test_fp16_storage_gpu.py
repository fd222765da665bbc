"""GPU tests of fp16 prediction-pool storage: the fp16-storage ingest kernels
(coda_amd/ops/hip/ingest_f16.hip), the fp16 pi_hat_delta kernels
(label.hip) and CODA end to end.

Nothing here is approximate. The ingest contract is bit-level (stored bits
== torch's CPU `wire.float().to(torch.float16)`, lowest-index argmax and an
h-ascending fp32 add chain of the stored values), so the kernel's four
outputs are compared with the eager twin run on the CPU from identical
start buffers. fp16 -> fp32 is exact, so everything computed from an fp16
pool is compared with torch.equal against the same computation on
`pool.float()`.
"""
import random

import pytest
import torch

pytestmark = pytest.mark.gpu

F16 = torch.float16
DT = {"fp32": torch.float32, "fp16": F16, "bf16": torch.bfloat16,
      "fp8": torch.float8_e4m3fn}
# two models, 101 points (ragged against every tile size, 64 down to 8);
# C=3: scalar width, odd rows; C=8 and C=1000: vector width, one tile of
# 64 points and thirteen of 8
INGEST_SHAPES = [(2, 101, 3), (2, 101, 8), (2, 101, 1000)]
H0, N0 = 1, 4          # chunk offsets inside the (H0 + 2, N0 + 101 + 3) pool


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
    return t.view(torch.int16) if t.dtype == F16 else t


def _crafted_values(full):
    """fp32 values at the places where an fp32 -> fp16 encoder can go
    wrong. `full` walks every fp16 subnormal; the short list (for the 606
    elements of the C=3 shape) keeps the ends and the middle."""
    f64 = torch.float64
    if full:
        k = torch.arange(0, 1025, dtype=f64)
    else:
        k = torch.tensor([0, 1, 2, 3, 4, 5, 6, 7, 255, 256, 511, 512, 513,
                          767, 1021, 1022, 1023, 1024], dtype=f64)
    sub = (k * 2.0 ** -24).float()                  # k * 2^-24, exact
    half = ((k[:-1] + 0.5) * 2.0 ** -24).float()    # subnormal RNE ties
    inf = torch.tensor(float("inf"))
    zero = torch.tensor(0.0)
    parts = [sub, half, torch.nextafter(half, inf), torch.nextafter(half, zero)]
    # 2^-25 (ties to zero) and its neighbours
    t25 = torch.tensor([2.0 ** -25])
    parts += [t25, torch.nextafter(t25, inf), torch.nextafter(t25, zero),
              torch.tensor([2.0 ** -26, 1.5 * 2.0 ** -25, 2.0 ** -30,
                            1e-40])]                # 1e-40: fp32 subnormal
    # RNE ties in the normal range, mantissa even / odd / carrying
    m = torch.tensor([0.0, 1.0, 2.0, 511.0, 1022.0, 1023.0], dtype=f64)
    for e in (-14, -3, 0, 10, 15):
        tie = ((1.0 + (m + 0.5) / 1024.0) * 2.0 ** e).float()
        parts += [tie, torch.nextafter(tie, inf), torch.nextafter(tie, zero)]
    # the overflow boundary: 65504 is the largest finite fp16, 65520 the
    # tie that rounds to infinity (positive only: -inf + inf in the
    # consensus would be a NaN, which is outside the contract)
    top = torch.tensor([65504.0, 65520.0, 65536.0, 1e5])
    parts += [top, torch.nextafter(top[:2], inf), torch.nextafter(top[:2], zero)]
    small = torch.cat([sub[:8], half[:8], t25])
    parts += [torch.tensor([0.0, -0.0]), -small]
    return torch.cat(parts)


_INPUTS = {}
_REFS = {}


def _input(shape, wire, kind):
    """(H, N, C) wire tensor on the CPU, built once per case."""
    key = (shape, wire, kind)
    if key not in _INPUTS:
        H, N, C = shape
        if kind == "softmax":
            # peaked rows, as real classifiers give: at C=1000 most of a
            # row lies below 2^-14
            g = torch.Generator().manual_seed(3)
            x = torch.softmax(4.0 * torch.randn(H, N, C, generator=g), -1)
        else:
            total = H * N * C
            vals = _crafted_values(full=total >= 8192)
            assert total >= vals.numel()
            g = torch.Generator().manual_seed(7)
            x = vals[torch.arange(total) % vals.numel()]
            x = x[torch.randperm(total, generator=g)].view(H, N, C)
        _INPUTS[key] = x.to(DT[wire])
    return _INPUTS[key]


def _start_buffers(shape, mirror):
    """Garbage-filled pool, mirror and classes, a random consensus."""
    H, N, C = shape
    Hl, Np = H0 + H, N0 + N + 3
    preds = torch.full((Hl * Np * C * 2,), 0x55,
                       dtype=torch.uint8).view(F16).view(Hl, Np, C)
    classes = torch.full((Hl, Np), -7, dtype=torch.long)
    ens = torch.rand(Np, C, generator=torch.Generator().manual_seed(1))
    preds_t = (torch.full((Hl * C * Np * 2,), 0x55,
                          dtype=torch.uint8).view(F16).view(Hl, C, Np)
               if mirror else None)
    return preds, classes, ens, preds_t


def _reference(shape, wire, kind, mirror):
    """The eager twin on the CPU; computed once per case, never modified."""
    from coda_amd.ops import reference
    key = (shape, wire, kind, mirror)
    if key not in _REFS:
        out = _start_buffers(shape, mirror)
        reference.ingest_chunk(_input(shape, wire, kind), H0, N0, *out)
        _REFS[key] = out
    return _REFS[key]


def _check_input_claims(shape, wire, kind):
    """What each input is claimed to exercise, asserted on the CPU before
    the GPU is touched."""
    w = _input(shape, wire, kind)
    s = w.float().to(F16)
    f = s.float()
    sub = (f.abs() > 0) & (f.abs() < 2.0 ** -14)
    if kind == "softmax":
        if shape[2] == 1000 and wire != "fp8":
            # (fp8 has flushed these to zero or its own 2^-9 grid already)
            assert sub.float().mean() > 0.25, "fp16 subnormals missing"
        return
    assert not bool(torch.isnan(f).any())
    assert int(sub.sum()) > 0
    if wire == "fp32":
        x = w.flatten()
        bits = _bits(s).flatten()
        assert int(torch.isinf(f).sum()) > 0 and bool((f == 65504.0).any())
        assert bool((x == 2.0 ** -25).any()) and bool((x == 65520.0).any())
        assert bits[x == 2.0 ** -25].eq(0).all()          # tie -> even = 0
        assert bits[x == 1.5 * 2.0 ** -24].eq(2).all()    # tie -> even = 2
        assert bits[x == 2.5 * 2.0 ** -24].eq(2).all()
        assert bits[x == 65520.0].eq(0x7c00).all()        # tie -> inf
        assert bool((bits == -0x8000).any()), "-0 missing"


# softmax rows from every wire dtype; the crafted fp32 set as it is, and
# rounded to the two 16-bit wires (e4m3 holds none of it: 65504 is a NaN
# there, outside the contract)
INGEST_CASES = ([(s, w, "softmax") for s in INGEST_SHAPES
                 for w in ("fp32", "fp16", "bf16", "fp8")]
                + [(s, w, "crafted") for s in INGEST_SHAPES
                   for w in ("fp32", "fp16", "bf16")])


@pytest.mark.parametrize("shape,wire,kind", INGEST_CASES,
                         ids=[f"{s[0]}x{s[1]}x{s[2]}-{w}-{k}"
                              for s, w, k in INGEST_CASES])
def test_ingest_into_fp16_matches_eager_twin(dev, shape, wire, kind):
    """All four outputs, and everything around the chunk, bit for bit."""
    from coda_amd import ops
    _check_input_claims(shape, wire, kind)
    w = _input(shape, wire, kind)
    for mirror in (True, False):
        want = _reference(shape, wire, kind, mirror)
        got = [None if t is None else t.to(dev)
               for t in _start_buffers(shape, mirror)]
        ops.ingest_chunk(w.to(dev), H0, N0, *got)
        torch.cuda.synchronize(dev)
        assert got[0].dtype == F16
        assert torch.equal(_bits(got[0].cpu()), _bits(want[0])), "preds_out"
        assert torch.equal(got[1].cpu(), want[1]), "classes_out"
        assert torch.equal(got[2].cpu(), want[2]), "ens_out"
        if mirror:
            assert torch.equal(_bits(got[3].cpu()), _bits(want[3])), \
                "preds_t_out"


def test_fp16_wire_to_fp16_storage_is_a_bit_copy(dev):
    """Every finite fp16 bit pattern and both infinities come through."""
    from coda_amd import ops
    bits = torch.arange(-32768, 32768, dtype=torch.int32).to(torch.int16)
    w = bits.view(F16)
    w = w[~torch.isnan(w.float())]
    C = 8
    w = torch.cat([w, torch.zeros(-w.numel() % C, dtype=F16)])
    n = w.numel() // C
    w = w.view(1, n, C)
    assert bool((w == 65504.0).any()) and int(torch.isinf(w).sum()) == 2
    preds = torch.zeros(1, n, C, dtype=F16, device=dev)
    classes = torch.zeros(1, n, dtype=torch.long, device=dev)
    ens = torch.zeros(n, C, device=dev)
    ops.ingest_chunk(w.to(dev), 0, 0, preds, classes, ens)
    assert torch.equal(_bits(preds.cpu()), _bits(w))
    # the kernel's own fp16 -> fp32 decode, over every subnormal too
    assert torch.equal(ens.cpu(), 0.0 + w[0].float())
    assert torch.equal(classes.cpu(), w.float().argmax(-1))


# ---------------------------------------------------------------------------
# pi_hat_delta
# ---------------------------------------------------------------------------

def _pool16(H, N, C, seed):
    """An fp16 pool with some points scaled into the fp16 subnormal
    range, so that the kernels' fp16 -> fp32 up-cast meets denormals."""
    from coda_amd.datasets import make_synthetic_task
    p, labels = make_synthetic_task(H=H, N=N, C=C, seed=seed)
    p[:, ::17] *= 2.0 ** -13
    p16 = p.half()
    f = p16.float()
    assert int(((f > 0) & (f < 2.0 ** -14)).sum()) > 0
    return p16, labels


@pytest.mark.parametrize("shape,route", [((5, 300, 7), "single_chain"),
                                         ((6, 70000, 3), "part"),
                                         ((6, 70000, 3), "mirror_part")],
                         ids=["5x300x7", "6x70000x3", "6x70000x3-mirror"])
def test_pi_hat_delta_fp16_equals_fp32_kernels(dev, shape, route,
                                               monkeypatch):
    from coda_amd import ops
    H, N, C = shape
    # the route ops.pi_hat_delta takes at this shape
    bx = (N + 255) // 256
    kh = -(-512 // bx)
    assert (kh > 1 and H >= 2 * kh) == (route != "single_chain")
    p16, _ = _pool16(H, N, C, seed=21)
    cls = torch.randint(0, C, (H,),
                        generator=torch.Generator().manual_seed(5))
    want_eager = ops.reference.pi_hat_delta(p16.float(), cls)

    d16 = p16.to(dev)
    d32 = d16.float()
    t16 = t32 = None
    if route == "mirror_part":
        t16 = d16.permute(0, 2, 1).contiguous()
        t32 = d32.permute(0, 2, 1).contiguous()
    got32 = ops.pi_hat_delta(d32, cls.to(dev), preds_t=t32)

    def boom(*a, **k):
        raise AssertionError("fp16 pool fell back to the eager op")
    monkeypatch.setattr(ops.reference, "pi_hat_delta", boom)
    got16 = ops.pi_hat_delta(d16, cls.to(dev), preds_t=t16)
    monkeypatch.undo()

    assert got16.dtype == torch.float32
    assert torch.equal(got16, got32)
    # the tolerance tests/test_gpu.py holds the fp32 kernel to
    torch.testing.assert_close(got16.cpu(), want_eager, rtol=1e-5, atol=1e-6)


# ---------------------------------------------------------------------------
# end to end
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("shape", [(8, 300, 5), (6, 70000, 3)],
                         ids=["8x300x5", "6x70000x3"])
def test_coda_on_fp16_storage_equals_fp32_storage(dev, shape, tmp_path):
    """An fp16-wire sharded task loaded as fp16 and as fp32: same init
    statistics, and over 10 teacher-forced CODA steps the same chosen
    index, selection value and P(best), bit for bit."""
    import bench
    from coda_amd import CODA
    from coda_amd.datasets import (Dataset, make_synthetic_task,
                                   write_sharded_task)
    H, N, C = shape
    p, labels = make_synthetic_task(H=H, N=N, C=C, seed=13)
    p16 = p.half()
    d = str(tmp_path / "t.shards")
    write_sharded_task(d, p16, "fp16", models_per_shard=3, labels=labels)
    ds16 = Dataset(d, dev, storage_dtype="fp16")
    ds32 = Dataset(d, dev, storage_dtype="fp32")

    # pool footprint: half of fp32, mirror included
    assert ds16.preds.dtype == F16 and ds16.preds.element_size() == 2
    assert ds32.preds.element_size() == 4
    assert torch.equal(_bits(ds16.preds.cpu()), _bits(p16))
    t16, t32 = ds16.init_stats["preds_t"], ds32.init_stats["preds_t"]
    assert (t16 is None) == (t32 is None)
    if t16 is not None:
        assert t16.dtype == F16 and t16.shape == (H, C, N)
        assert torch.equal(t16.float(), t32)
    assert torch.equal(ds16.init_stats["classes"],
                       ds32.init_stats["classes"])
    assert torch.equal(ds16.init_stats["ens_sum"],
                       ds32.init_stats["ens_sum"])

    # (the wide pool's candidates in chunks that keep the step short)
    chunk = 64 if N <= 1000 else 8192
    # torch's float index_add_ (the confusion prior) sums with atomics on
    # the GPU; like the benchmark, build the selectors with its
    # deterministic accumulation so that two constructions can be compared
    # bit for bit at all
    sels = []
    for ds in (ds16, ds32):
        random.seed(0)
        torch.manual_seed(0)
        with bench.reproducible_setup():
            sels.append(CODA(ds, chunk_size=chunk))
    s16, s32 = sels
    assert s16._preds_t is t16
    assert torch.equal(s16.get_pbest(), s32.get_pbest())
    for step in range(10):
        picks = []
        for sel in (s16, s32):
            random.seed(step)
            torch.manual_seed(step)
            idx, q = sel.get_next_item_to_label()
            picks.append((int(idx), float(q)))
        assert picks[0] == picks[1], (step, picks)
        idx, q = picks[1]
        y = int(labels[idx])
        s16.add_label(idx, y, q)
        s32.add_label(idx, y, q)
        assert torch.equal(s16.get_pbest(), s32.get_pbest()), step


def test_legacy_fp16_pt_stays_fp16_on_the_wire(dev, tmp_path, monkeypatch):
    """An fp16 .pt bound for fp16 storage is never up-cast: not on the
    host, not in the pinned staging buffers, not on the device - through
    the one-copy route, the pinned route and the streamed route."""
    from coda_amd.datasets import Dataset, make_synthetic_task
    # 600 KB per model: the 1 MB streamed route takes one model a chunk
    p, _ = make_synthetic_task(H=3, N=60000, C=5, seed=8)
    p16 = p.half()
    path = str(tmp_path / "t.pt")
    torch.save(p16, path)

    staged = []
    real_pin = torch.Tensor.pin_memory

    def spy_pin(self, *a, **k):
        staged.append(self.dtype)
        return real_pin(self, *a, **k)
    monkeypatch.setattr(torch.Tensor, "pin_memory", spy_pin)

    def no_float(self, *a, **k):
        raise AssertionError("fp16 pool up-cast on the way to the device")
    monkeypatch.setattr(torch.Tensor, "float", no_float)
    loaded = [Dataset(path, dev, storage_dtype="fp16"),
              Dataset(path, dev, storage_dtype="fp16", pin=True),
              Dataset(path, dev, storage_dtype="fp16", stream_chunk_mb=1)]
    monkeypatch.undo()
    assert len(staged) == 3 and all(dt == F16 for dt in staged)
    for ds in loaded:
        assert ds.preds.dtype == F16 and ds.preds.is_cuda
        assert torch.equal(_bits(ds.preds.cpu()), _bits(p16))


# ---------------------------------------------------------------------------
# pi marginal: what makes "bit for bit" above possible at C = 5 and C = 3
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("N,C", [(300, 5), (70000, 3), (30000, 182),
                                 (500, 1500)],
                         ids=["300x5", "70000x3", "30000x182", "500x1500"])
def test_pi_marginal_scalar_route_is_deterministic(dev, N, C):
    """The class counts the vector kernels do not take (C % 4 != 0, or
    C > 1024) sum their slab partials in a fixed order: equal bits from
    call to call, and the fp64 value within the fp32 chain's bound - at
    most 46/2 + 2 slab adds, 96/2 + 2 and 16 reduce adds and 3 roundings
    per term at these shapes, i.e. 94 * 2^-24 = 5.6e-6 relative on sums
    of positive terms; 1e-5 is asserted."""
    from coda_amd import ops
    assert C % 4 != 0 or C > 1024
    assert -(-N // 1536) <= 46
    g = torch.Generator().manual_seed(N + C)
    adjusted = (torch.rand(N, C, generator=g) + 0.05)
    row_sums = adjusted.sum(-1) * (0.5 + torch.rand(N, generator=g))
    want = ((1.0 / row_sums.double()) @ adjusted.double())
    a, r = adjusted.to(dev), row_sums.to(dev)
    first = ops._ext.pi_marginal(a, r)
    assert first.shape == (C,) and first.dtype == torch.float32
    for _ in range(4):
        assert torch.equal(ops._ext.pi_marginal(a, r), first)
    rel = ((first.cpu().double() - want).abs() / want).max()
    print(f"pi_marginal {N}x{C}: max rel err {float(rel):.3e}")
    assert float(rel) <= 1e-5
