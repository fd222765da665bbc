"""GPU tests of the fused ingest kernel (coda_amd/ops/hip/ingest.hip).

The kernel is compared with the eager twin (ops.reference.ingest_chunk) run
on the CPU, on inputs built on the CPU. Nothing in the contract is
approximate - storage rounding is torch's CPU conversion, the argmax has a
tie rule, the consensus is a fixed chain of fp32 adds - so every output is
compared with torch.equal (fp8 / bf16 through their bit patterns).

Shapes (H, N, C) are the smallest that reach each way the kernel can go
wrong: odd C (unaligned 1- and 2-byte rows, the scalar path) with N off
the tile size; C below one wave; C over many lane strides plus a tail
(and, in fp8, a tile past 64 KB of LDS); the fully aligned vector path;
the degenerate single element.
"""
import random

import pytest
import torch

pytestmark = pytest.mark.gpu

F8 = torch.float8_e4m3fn
DT = {"fp32": torch.float32, "fp16": torch.float16, "bf16": torch.bfloat16,
      "fp8": F8}
ALL_PAIRS = [("fp32", "fp32"), ("fp32", "bf16"), ("fp32", "fp8"),
             ("fp16", "fp32"), ("bf16", "bf16"), ("fp8", "fp8"),
             ("bf16", "fp8")]
FEW_PAIRS = [("fp8", "fp8"), ("fp32", "bf16")]
SHAPES = [(5, 130, 67), (3, 70, 3), (2, 65, 1001), (4, 128, 64), (1, 1, 5)]
CASES = ([(SHAPES[0], p) for p in ALL_PAIRS]
         + [(s, p) for s in SHAPES[1:] for p in FEW_PAIRS])


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
    if t.dtype == F8:
        return t.view(torch.uint8)
    if t.dtype == torch.bfloat16:
        return t.view(torch.int16)
    return t


def _tie_rows(f):
    """Rows whose maximum is attained at two or more positions."""
    return ((f == f.max(-1, keepdim=True).values).sum(-1) >= 2)


def _crafted(shape, wire_dt):
    """Every row has its maximum (0.75, exact in every dtype here) at two
    or more positions and everything else below 0.5, so only the tie rule
    decides each class. Row (0, 0) has its first maximum in the last
    lane-stride's tail (columns C-2, C-1); row (0, 1) spans the whole row;
    row (0, 2) straddles the 64-column stride boundary."""
    from coda_amd.datasets import make_synthetic_task
    H, N, C = shape
    assert C >= 3 and N >= 3
    base, _ = make_synthetic_task(H=H, N=N, C=C, seed=9, temperature=0.5)
    x = base * 0.5
    g = torch.Generator().manual_seed(5)
    a = torch.randint(0, C - 1, (H, N), generator=g)
    b = a + 1 + (torch.rand(H, N, generator=g) * (C - 1 - a)).long()
    b = b.clamp(max=C - 1)
    a[0, 0], b[0, 0] = C - 2, C - 1
    a[0, 1], b[0, 1] = 0, C - 1
    if C > 64:
        a[0, 2], b[0, 2] = 63, 64
    assert bool((a < b).all())
    x.scatter_(2, a.unsqueeze(-1), 0.75)
    x.scatter_(2, b.unsqueeze(-1), 0.75)
    return x.to(wire_dt), a


_INPUTS = {}
_REFS = {}


def _input(shape, wire, crafted=False):
    from coda_amd.datasets import make_synthetic_task
    key = (shape, wire, crafted)
    if key not in _INPUTS:
        if crafted:
            _INPUTS[key] = _crafted(shape, DT[wire])[0]
        else:
            H, N, C = shape
            p, _ = make_synthetic_task(H=H, N=N, C=C, seed=3,
                                       temperature=0.5)
            _INPUTS[key] = p.to(DT[wire])
    return _INPUTS[key]


def _ens_start(shape):
    _, N, C = shape
    return torch.rand(N, C, generator=torch.Generator().manual_seed(1))


def _reference(shape, wire, storage, crafted=False):
    """The eager twin on the CPU, one whole-pool call; computed once per
    case and shared (never modified)."""
    from coda_amd.ops import reference
    key = (shape, wire, storage, crafted)
    if key not in _REFS:
        H, N, C = shape
        w = _input(shape, wire, crafted)
        preds = torch.zeros(H, N, C).to(DT[storage])
        classes = torch.empty(H, N, dtype=torch.long)
        ens = _ens_start(shape)
        preds_t = torch.zeros(H, C, N).to(DT[storage])
        reference.ingest_chunk(w, 0, 0, preds, classes, ens, preds_t)
        _REFS[key] = (preds, classes, ens, preds_t)
    return _REFS[key]


def _run_gpu(dev, w, storage, hc, nc, mirror, misalign=False):
    """Ingest w on the GPU in (hc, nc) chunks into garbage-filled outputs."""
    from coda_amd import ops
    H, N, C = w.shape
    sdt = DT[storage]
    esz = torch.empty(0, dtype=sdt).element_size()
    preds = torch.full((H * N * C * esz,), 0x55, dtype=torch.uint8,
                       device=dev).view(sdt).view(H, N, C)
    classes = torch.full((H, N), -7, dtype=torch.long, device=dev)
    ens = _ens_start((H, N, C)).to(dev)
    preds_t = (torch.full((H * C * N * esz,), 0x55, dtype=torch.uint8,
                          device=dev).view(sdt).view(H, C, N)
               if mirror else None)
    for h0 in range(0, H, hc):
        for n0 in range(0, N, nc):
            chunk = w[h0:h0 + hc, n0:n0 + nc].contiguous()
            if misalign:
                # contiguous, but starting one element into its buffer
                buf = torch.empty(chunk.numel() + 1, dtype=chunk.dtype,
                                  device=dev)
                buf[1:].copy_(chunk.reshape(-1))
                wire = buf[1:].view(chunk.shape)
                assert wire.data_ptr() % 16 != 0
            else:
                wire = chunk.to(dev)
            ops.ingest_chunk(wire, h0, n0, preds, classes, ens, preds_t)
    torch.cuda.synchronize(dev)
    return preds, classes, ens, preds_t


def _assert_same(got, want, mirror):
    assert torch.equal(_bits(got[0].cpu()), _bits(want[0])), "preds_out"
    assert torch.equal(got[1].cpu(), want[1]), "classes_out"
    assert torch.equal(got[2].cpu(), want[2]), "ens_out"
    if mirror:
        assert torch.equal(_bits(got[3].cpu()), _bits(want[3])), "preds_t_out"
    else:
        assert got[3] is None


def _check_input_claims(shape, wire, storage):
    """What the synthetic input is claimed to exercise, asserted on the
    CPU before the GPU is touched."""
    H, N, C = shape
    f = _input(shape, wire).float().to(DT[storage]).float()
    if storage == "fp8" and C >= 64:
        sub = (f > 0) & (f < 2.0 ** -6)
        assert sub.float().mean() > 0.25, "fp8 subnormals missing"
        assert int(_tie_rows(f).sum()) > 0, "no tie rows in the fp8 input"


@pytest.mark.parametrize("chunks", ["whole", "hc2_nc37"])
@pytest.mark.parametrize("shape,pair", CASES,
                         ids=[f"{s[0]}x{s[1]}x{s[2]}-{p[0]}-{p[1]}"
                              for s, p in CASES])
def test_kernel_matches_eager_twin(dev, shape, pair, chunks):
    wire, storage = pair
    _check_input_claims(shape, wire, storage)
    want = _reference(shape, wire, storage)
    hc, nc = (shape[0], shape[1]) if chunks == "whole" else (2, 37)
    for mirror in (True, False):
        got = _run_gpu(dev, _input(shape, wire), storage, hc, nc, mirror)
        _assert_same(got, want, mirror)


@pytest.mark.parametrize("chunks", ["whole", "hc2_nc37"])
@pytest.mark.parametrize("shape", [SHAPES[0], SHAPES[2]],
                         ids=["5x130x67", "2x65x1001"])
@pytest.mark.parametrize("wire,storage",
                         [("fp32", "fp32"), ("fp16", "fp32"),
                          ("bf16", "bf16"), ("fp8", "fp8")])
def test_tie_rule_binds(dev, shape, wire, storage, chunks):
    """Crafted input, one per wire dtype: every row ties at its maximum,
    so classes are decided by the lowest-index rule alone."""
    w, first = _crafted(shape, DT[wire])
    f = w.float().to(DT[storage]).float()
    assert bool(_tie_rows(f).all())
    assert bool((f.max(-1).values == 0.75).all())
    assert int(first[0, 0]) == shape[2] - 2      # first max in the tail
    _INPUTS.setdefault((shape, wire, True), w)
    want = _reference(shape, wire, storage, crafted=True)
    assert torch.equal(want[1], first)
    hc, nc = (shape[0], shape[1]) if chunks == "whole" else (2, 37)
    for mirror in (True, False):
        got = _run_gpu(dev, w, storage, hc, nc, mirror)
        _assert_same(got, want, mirror)


@pytest.mark.parametrize("pair", FEW_PAIRS, ids=["fp8-fp8", "fp32-bf16"])
def test_misaligned_wire_takes_the_scalar_path(dev, pair):
    """C % 4 == 0 but the wire buffer is not 16-byte aligned."""
    wire, storage = pair
    shape = SHAPES[3]
    want = _reference(shape, wire, storage)
    got = _run_gpu(dev, _input(shape, wire), storage, 2, 37, True,
                   misalign=True)
    _assert_same(got, want, True)


def test_offsets_past_2_31(dev):
    """A small chunk written at the far end of a pool of 3.08e9 elements:
    its pool, mirror and classes offsets only exist in 64-bit arithmetic.
    The outputs are allocated, never filled by the host (fp8: 2 x 3.1 GB +
    3.1 GB of consensus); everything outside the chunk must stay untouched."""
    from coda_amd import ops
    from coda_amd.ops import reference
    Hl, N, C = 4, 1_100_000, 700
    hc, nc, h0, n0 = 1, 50, 3, N - 50
    assert (h0 * N + n0) * C > 2 ** 31 and h0 * C * N > 2 ** 31
    w = _input((hc, nc, C), "fp8")
    want = (torch.zeros(hc, nc, C).to(F8),
            torch.empty(hc, nc, dtype=torch.long), torch.zeros(nc, C),
            torch.zeros(hc, C, nc).to(F8))
    reference.ingest_chunk(w, 0, 0, *want)

    preds = torch.full((Hl, N, C), 0x55, dtype=torch.uint8, device=dev)
    preds_t = torch.full((Hl, C, N), 0x55, dtype=torch.uint8, device=dev)
    classes = torch.full((Hl, N), -7, dtype=torch.long, device=dev)
    ens = torch.zeros(N, C, device=dev)
    ops.ingest_chunk(w.to(dev), h0, n0, preds.view(F8), classes, ens,
                     preds_t.view(F8))
    torch.cuda.synchronize(dev)
    assert torch.equal(preds[h0:, n0:].cpu(), want[0].view(torch.uint8))
    assert torch.equal(classes[h0:, n0:].cpu(), want[1])
    assert torch.equal(ens[n0:].cpu(), want[2])
    assert torch.equal(preds_t[h0:, :, n0:].cpu(), want[3].view(torch.uint8))
    # put the chunk's region back: nothing else may have changed
    preds[h0:, n0:] = 0x55
    preds_t[h0:, :, n0:] = 0x55
    classes[h0:, n0:] = -7
    ens[n0:] = 0
    assert bool((preds == 0x55).all()) and bool((preds_t == 0x55).all())
    assert bool((classes == -7).all()) and not bool(ens.any())


def test_rejects_out_of_range_chunk(dev):
    """Bounds are checked on the host before anything is launched."""
    from coda_amd import ops
    H, N, C = 2, 10, 4
    preds = torch.zeros(H, N, C, device=dev)
    classes = torch.zeros(H, N, dtype=torch.long, device=dev)
    ens = torch.zeros(N, C, device=dev)
    wire = torch.zeros(2, 5, C, device=dev)
    for h0, n0 in [(1, 0), (0, 6), (-1, 0)]:
        with pytest.raises(RuntimeError, match="outside"):
            ops.ingest_chunk(wire, h0, n0, preds, classes, ens)
    with pytest.raises(RuntimeError, match="preds_t_out"):
        ops.ingest_chunk(wire, 0, 0, preds, classes, ens,
                         torch.zeros(H, N, C, device=dev))
    with pytest.raises(RuntimeError, match="wire dtype"):
        ops.ingest_chunk(wire.to(torch.float64), 0, 0, preds, classes, ens)


@pytest.fixture(scope="module")
def shard_dirs(tmp_path_factory):
    from coda_amd.datasets import make_synthetic_task, write_sharded_task
    preds, labels = make_synthetic_task(H=6, N=400, C=8, seed=11)
    root = tmp_path_factory.mktemp("ingest")
    dirs = {}
    for name in ("bf16", "fp8"):
        dirs[name] = str(root / f"t_{name}.shards")
        write_sharded_task(dirs[name], preds, name, models_per_shard=4,
                           labels=labels)
    return preds, labels, dirs


@pytest.mark.parametrize("storage", ["bf16", "fp8"])
def test_run_to_run_bit_identical(dev, shard_dirs, storage):
    from coda_amd.datasets import Dataset
    _, _, dirs = shard_dirs
    budget = 150 * 8 / (1 << 20)        # sub-splits every model along n
    a = Dataset(dirs[storage], dev, storage_dtype=storage,
                stream_chunk_mb=budget)
    b = Dataset(dirs[storage], dev, storage_dtype=storage,
                stream_chunk_mb=budget)
    c = Dataset(dirs[storage], dev, storage_dtype=storage)  # one chunk/shard
    for other in (b, c):
        assert torch.equal(_bits(a.preds), _bits(other.preds))
        assert torch.equal(a.init_stats["classes"],
                           other.init_stats["classes"])
        assert torch.equal(a.init_stats["ens_sum"],
                           other.init_stats["ens_sum"])
        assert torch.equal(_bits(a.init_stats["preds_t"]),
                           _bits(other.init_stats["preds_t"]))


@pytest.mark.parametrize("storage", ["bf16", "fp8"])
def test_end_to_end_matches_in_memory_route(dev, shard_dirs, storage,
                                            monkeypatch):
    """CODA on a sharded task == CODA on the same pool from tensors.

    The two routes sum the consensus in different orders (h-ascending adds
    vs torch's chunked sum), which can only matter through the pseudo-label
    argmax; the input is first shown to be safe: the smallest top-2 margin
    of the fp64 consensus must exceed 100 x the fp32 summation error bound
    (H-1) * 2^-24 * max sum|x|. get_pbest is compared at the tolerance
    tests/test_gpu.py uses for two routes on one GPU (graph vs eager
    replay: rtol=1e-5, atol=1e-7)."""
    from coda_amd import CODA, Oracle, ops
    from coda_amd.datasets import Dataset
    from coda_amd.options import LOSS_FNS
    preds, labels, dirs = shard_dirs
    sdt = DT[storage]
    H = preds.shape[0]
    stored = preds.to(sdt)
    cons = stored.double().sum(0)                       # (N, C) fp64
    top2 = cons.topk(2, dim=-1).values
    margin = float((top2[:, 0] - top2[:, 1]).min())
    bound = 100 * (H - 1) * 2.0 ** -24 * float(cons.abs().max())
    print(f"consensus top-2 margin {margin:.3e} vs bound {bound:.3e}")
    assert margin > bound, "pick another seed: consensus argmax not safe"

    ds_a = Dataset(dirs[storage], dev, storage_dtype=storage)
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
