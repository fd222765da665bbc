"""References for the logits ingest (ops.ingest_chunk with logit_scale,
coda_amd/ops/hip/ingest_logits.hip), shared by tests/test_ingest_logits.py
(CPU) and tests/test_ingest_logits_gpu.py.

  ref64   the contract in fp64 on the wire-rounded logits and the fp32
          k_h = float32(log2(e) / T_h):  exp2((x - max x) * k_h) / Z.
  twin32  the same with every operation rounded to fp32 in the kernel's
          order - class c on lane c % 64, ascending per lane, the 64
          partial sums combined by the xor butterfly 32, 16, .., 1 - and
          a correctly rounded exp2. Emulated in fp64 (PARITY.md: a torch
          fp32 sum is not the same number on two hosts): the sum,
          product and quotient of two fp32 values rounded to fp64 and
          then to fp32 equal the fp32 operation (53 >= 2 * 24 + 2).

Storage rounding of an fp64 value goes straight from fp64 (torch would
round through fp32 first); stored values are compared as ordinals of
their bit patterns, which for non-negative values is the order of the
format, so "the immediate neighbour" is an ordinal distance of 1.
"""
import math

import numpy as np
import torch

F8 = torch.float8_e4m3fn
DT = {"fp32": torch.float32, "fp16": torch.float16, "bf16": torch.bfloat16,
      "fp8": F8}
WIRES = ("fp32", "fp16", "bf16")
STORAGES = ("fp32", "fp16", "bf16", "fp8")
SHAPES = [(5, 130, 67), (3, 70, 3), (2, 65, 1001), (4, 128, 64), (1, 1, 5)]
# (mantissa bits, exponent of the smallest normal)
FORMATS = {"fp32": (23, -126), "fp16": (10, -14), "bf16": (7, -126),
           "fp8": (3, -6)}
TINY = 2.0 ** -126
TEMP_SETS = ("ones", "vec")
_VEC = (0.37, 2.5, 1.0, 0.8, 1.7)


def temperatures(H, tset):
    """All ones, or a per-model vector that starts 0.37, 2.5."""
    return [1.0] * H if tset == "ones" else list(_VEC[:H])


def logit_scale(temps):
    """k_h = float32(log2(e) / T_h), rounded once from fp64 (the loader's
    formula)."""
    t = torch.tensor(temps, dtype=torch.float64)
    return (math.log2(math.e) / t).to(torch.float32)


_LOGITS = {}


def logits(shape, wire, offset=0.0):
    """N(0, 4^2) logits rounded to the wire dtype, so |t| reaches the
    range where the tails underflow storage. offset raises the classes
    from 64 on: the row maximum then lies outside the first lane stride,
    far enough (offset * k > 1024) that a maximum taken over the first 64
    classes overflows exp2 even in fp64."""
    key = (shape, wire, offset)
    if key not in _LOGITS:
        g = torch.Generator().manual_seed(7)
        x = torch.randn(shape, generator=g) * 4.0
        if offset:
            x[..., 64:] += offset
        _LOGITS[key] = x.to(DT[wire])
    return _LOGITS[key]


def _np64(x):
    return x.float().double().numpy()


def ref64(x, k, *, max_first=None, drop_last_z=False, shared_tile=0,
          k_model0=False):
    """(H, N, C) fp64 softmax of the contract. The keyword arguments apply
    one fault each (mutation floors): the max over the first `max_first`
    classes only; the last class left out of Z; the last point of every
    `shared_tile`-point tile using its neighbour's m and Z; model 0's k
    for every model."""
    x = _np64(x)
    k = k.double().numpy()
    if k_model0:
        k = np.full_like(k, k[0])
    with np.errstate(over="ignore", invalid="ignore"):
        m = (x[..., :max_first] if max_first else x).max(-1, keepdims=True)
        if shared_tile:
            m = m.copy()
            last = [n for n in range(1, x.shape[1])
                    if n % shared_tile == shared_tile - 1
                    or n == x.shape[1] - 1]
            m[:, last] = m[:, [n - 1 for n in last]]
        e = np.exp2((x - m) * k[:, None, None])
        z = (e[..., :-1] if drop_last_z else e).sum(-1, keepdims=True)
        if shared_tile:
            z = z.copy()
            z[:, last] = z[:, [n - 1 for n in last]]
        return e / z


def _f32(a):
    return a.astype(np.float32).astype(np.float64)


def twin32(x, k):
    """The fp32 twin (module docstring), as fp64 values that are fp32
    numbers."""
    x = _np64(x)
    k = k.double().numpy()[:, None, None]
    H, N, C = x.shape
    m = x.max(-1, keepdims=True)
    e = _f32(np.exp2(_f32(_f32(x - m) * k)))
    strides = -(-C // 64)
    pad = np.zeros((H, N, strides * 64))
    pad[..., :C] = e                     # z + 0 == z: absent classes
    pad = pad.reshape(H, N, strides, 64)
    acc = np.zeros((H, N, 64))
    for i in range(strides):
        acc = _f32(acc + pad[:, :, i])
    lanes = np.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        acc = _f32(acc + acc[..., lanes ^ off])
    return _f32(e / acc[..., :1])


def round_storage(p64, storage):
    """fp64 array in [0, 1] -> torch tensor in the storage dtype, rounded
    to nearest even straight from fp64."""
    mant, emin = FORMATS[storage]
    _, ex = np.frexp(p64)
    q = np.ldexp(1.0, np.maximum(ex - 1, emin) - mant)
    r = np.rint(p64 / q) * q
    return torch.from_numpy(r).float().to(DT[storage])


def ordinal(t):
    """Bit patterns as int64 (the format's order for non-negative values)."""
    if t.dtype == torch.float32:
        return t.view(torch.int32).long()
    if t.dtype == F8:
        return t.view(torch.uint8).long()
    return t.view(torch.int16).long()


def lowp_mismatch(got, p64, storage):
    """(largest ordinal distance, fraction of elements that differ) of a
    stored pool against the storage rounding of the fp64 value."""
    d = (ordinal(got) - ordinal(round_storage(p64, storage))).abs()
    return int(d.max()), float((d != 0).double().mean())


def f32_error(got, p64):
    """(worst relative error over the elements with p64 >= 2^-126, worst
    |error| / 2^-126 over the elements below that are not stored as 0).
    A NaN anywhere gives inf."""
    g = got.double().numpy() if isinstance(got, torch.Tensor) else got
    if not np.isfinite(g).all() or not np.isfinite(p64).all():
        return math.inf, math.inf
    big = p64 >= TINY
    rel = float((np.abs(g - p64)[big] / p64[big]).max()) if big.any() else 0.0
    small = ~big & (g != 0)
    sub = float((np.abs(g - p64)[small]).max() / TINY) if small.any() else 0.0
    return rel, sub


def tile_points(nc, C):
    """The kernel's tile: the largest power of two <= 64 (and < 2 * nc)
    whose consensus + stage + Z rows fit 80 KB."""
    rb = (C * 4 + 15) & ~15
    if (rb // 16) % 2 == 0:
        rb += 16
    tn = 64
    while tn > 1 and ((tn >> 1) >= nc
                      or ((tn * C * 4 + 15) & ~15) + tn * rb + tn * 4
                      > 80 * 1024):
        tn >>= 1
    return tn


# Worst relative error of twin32 against ref64 over the elements >= 2^-126,
# per (shape, wire, temperature set): the fp32-storage cases of the GPU
# test. The tolerance on the kernel's fp32 pool is MARGIN x the entry
# (1-ulp hardware exp2, and headroom for another order and the divide).
MARGIN = 16.0
E32 = {
    ((5, 130, 67), "fp32", "ones"): 2.279e-06,
    ((5, 130, 67), "fp32", "vec"): 5.196e-06,
    ((5, 130, 67), "fp16", "ones"): 1.397e-06,
    ((5, 130, 67), "fp16", "vec"): 2.739e-06,
    ((5, 130, 67), "bf16", "ones"): 1.370e-06,
    ((5, 130, 67), "bf16", "vec"): 2.697e-06,
    ((3, 70, 3), "fp16", "ones"): 7.038e-07,
    ((3, 70, 3), "fp16", "vec"): 1.311e-06,
    ((2, 65, 1001), "fp16", "ones"): 1.528e-06,
    ((2, 65, 1001), "fp16", "vec"): 3.797e-06,
    ((4, 128, 64), "fp16", "ones"): 1.427e-06,
    ((4, 128, 64), "fp16", "vec"): 2.758e-06,
    ((1, 1, 5), "fp16", "ones"): 4.779e-07,
    ((1, 1, 5), "fp16", "vec"): 1.194e-06,
}


def f32_cases():
    return ([(SHAPES[0], w, t) for w in WIRES for t in TEMP_SETS]
            + [(s, "fp16", t) for s in SHAPES[1:] for t in TEMP_SETS])


def measure_e32(shape, wire, tset):
    x = logits(shape, wire)
    k = logit_scale(temperatures(shape[0], tset))
    return f32_error(twin32(x, k), ref64(x, k))[0]


def crafted_ties(shape, wire):
    """Every row has its maximum logit (24, exact in every wire dtype, 6
    sigma above the rest) at two or more classes; rows (0, 0..2) as in
    tests/test_ingest_gpu.py: the tail of the last lane stride, the whole
    row, the stride boundary."""
    H, N, C = shape
    x = logits(shape, wire).float().clone()
    assert float(x.max()) < 23.0
    g = torch.Generator().manual_seed(5)
    a = torch.randint(0, C - 1, (H, N), generator=g)
    b = (a + 1 + (torch.rand(H, N, generator=g) * (C - 1 - a)).long()) \
        .clamp(max=C - 1)
    a[0, 0], b[0, 0] = C - 2, C - 1
    a[0, 1], b[0, 1] = 0, C - 1
    if C > 64:
        a[0, 2], b[0, 2] = 63, 64
    assert bool((a < b).all())
    x.scatter_(2, a.unsqueeze(-1), 24.0)
    x.scatter_(2, b.unsqueeze(-1), 24.0)
    return x.to(DT[wire]), a, b


def check_ties(preds, classes, a, b):
    f = preds.float()
    fa = f.gather(2, a.unsqueeze(-1))
    assert torch.equal(fa, f.gather(2, b.unsqueeze(-1))), "tied s differ"
    assert torch.equal(fa.squeeze(-1), f.max(-1).values)
    assert torch.equal(classes, a), "lowest index must win"


def with_neg_inf(shape, wire):
    """A fifth of the entries -inf, column 1 of every row kept finite."""
    x = logits(shape, wire).clone()
    g = torch.Generator().manual_seed(8)
    hole = torch.rand(shape, generator=g) < 0.2
    hole[..., min(1, shape[2] - 1)] = False
    x[hole] = float("-inf")
    return x, hole


def check_pool(got, p64, shape, wire, storage, tset, what):
    """The conditions on a stored pool (PARITY.md, L2; spelled out in
    tests/test_ingest_logits.py); prints before asserting."""
    if storage == "fp32":
        e32 = E32[(shape, wire, tset)]
        tol = MARGIN * e32
        rel, sub = f32_error(got, p64)
        print(f"{what} {shape} {wire}->fp32 {tset}: rel {rel:.3e} "
              f"sub {sub:.3e} (E32 {e32:.3e}, tol {tol:.3e})")
        assert rel <= tol and sub <= tol + 2.0 ** -23
    else:
        dist, frac = lowp_mismatch(got, p64, storage)
        print(f"{what} {shape} {wire}->{storage} {tset}: ordinal distance "
              f"{dist}, differing {frac:.3%}")
        assert dist <= 1 and frac <= 0.01
