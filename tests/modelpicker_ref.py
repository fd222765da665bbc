"""fp64 reference and fp32 twin of the hit-sparse ModelPicker entropy
(not itself a test).

`dev64` is the CONTRACT of ops.modelpicker_dev: the dense formula of
ModelPicker.compute_entropies, clamp(min=1e-12) included, on the fp32
posterior up-cast to fp64, as dev64[n] = C * (entropies64[n] - e0_64). A
class no model predicts on n gives exactly e0_64, so only the hit
classes are evaluated and C = 32767 stays cheap.

`closed_dev` is the kernel's formulation (coda_amd/ops/hip/modelpicker.hip:
sorted segments, S / T' sums of the fp64 prologue's p_h and centred q_h,
closed-form epilogue with log1p). With
f32=True every operation is rounded to fp32 in one fixed order -
sequential along the sorted positions; numpy's
elementwise float32 +, *, / are correctly rounded and the fused
multiply-adds and log1p / log2 are evaluated in fp64 and rounded once -
so all hosts agree. That twin against dev64 is how the tolerances are
measured (never from kernel output). With f32=False the same code runs
in fp64 and takes the faults of the mutation-floor tests.
"""
from __future__ import annotations

import functools

import numpy as np
import torch

from coda_amd import ops

MARGIN = 16.0                      # the project's margin over the twin's error
POSTERIOR_STEPS = {"uniform": 0, "spread3": 3, "spread60": 60,
                   "conc400": 400, "conc2000": 2000}
FAULTS = ("drop_class", "drop_last_model", "ignore_pos64", "drop_T")


def gamma_of(eps: float) -> float:
    return (1.0 - eps) / eps


@functools.lru_cache(maxsize=None)
def make_posterior(H: int, kind: str, eps: float = 0.45,
                   seed: int = 0) -> np.ndarray:
    """(H,) float32 posterior after POSTERIOR_STEPS[kind] label updates
    of models with accuracies in [0.3, 0.9], kept in fp32 between steps
    as the selector keeps it: conc2000 underflows most entries to 0."""
    rng = np.random.default_rng(1000 * seed + H)
    acc = 0.3 + 0.6 * rng.random(H)
    g = gamma_of(eps)
    post = np.full(H, 1.0 / H, dtype=np.float32)
    for _ in range(POSTERIOR_STEPS[kind]):
        agree = rng.random(H) < acc
        nxt = post.astype(np.float64) * np.where(agree, g, 1.0)
        post = (nxt / nxt.sum()).astype(np.float32)
        # round-to-nearest parks a dying entry on the smallest denormal
        # for good; flush it as a denormal-flushing device would, so the
        # concentrated posteriors hold exact zeros (the 0 log 0 path)
        post[post < np.float32(2.0 ** -126)] = 0
    post.setflags(write=False)
    return post


@functools.lru_cache(maxsize=None)
def make_rows(H: int, C: int, N: int = 257, seed: int = 0):
    """(N, H) int64 class rows and an (N,) bool active mask.

    Row 0 and rows >= 7 draw from a per-point set of 1..8 classes (few
    distinct classes keep dev64 cheap at H = 1024). Rows 1..6:
      1  all models agree (dev is exactly 0)
      2  all models distinct where H <= C, else as many classes as exist
      3  a class boundary between sorted positions 63 and 64 (H > 64;
         the middle of the row otherwise)
      4  H >= 1000: one class holds 900 models; else uniform classes
      5  uniform classes, inactive
      6  uniform classes
    About a quarter of the rows >= 7 are inactive.
    """
    rng = np.random.default_rng(7919 * seed + 131 * H + C)
    rows = np.empty((N, H), dtype=np.int64)
    for n in range(N):
        k = int(rng.integers(1, min(8, C) + 1))
        cand = rng.choice(C, size=k, replace=False)
        rows[n] = cand[rng.integers(0, k, H)]
    active = rng.random(N) >= 0.25
    active[:5] = True
    if N > 1:
        rows[1] = C - 1
    if N > 2:
        rows[2] = (rng.permutation(C)[:H] if H <= C
                   else rng.permutation(H) % C)
    if N > 3:
        cut = 64 if H > 64 else max(1, H // 2)
        lo, hi = sorted(rng.choice(C, size=2, replace=False).tolist())
        rows[3] = hi
        rows[3, rng.permutation(H)[:cut]] = lo
    if N > 4:
        rows[4] = rng.integers(0, C, H)
        if H >= 1000:
            rows[4, rng.permutation(H)[:900]] = int(rng.integers(0, C))
    if N > 5:
        rows[5] = rng.integers(0, C, H)
        active[5] = False
    if N > 6:
        rows[6] = rng.integers(0, C, H)
        active[6] = True
    rows.setflags(write=False)
    active.setflags(write=False)
    return rows, active


@functools.lru_cache(maxsize=None)
def uniform_rows(H: int, C: int, N: int = 64, seed: int = 0) -> np.ndarray:
    """(N, H) rows of independent uniform classes (the floor tests)."""
    rng = np.random.default_rng(104729 * seed + 131 * H + C)
    rows = rng.integers(0, C, (N, H))
    rows.setflags(write=False)
    return rows


def build(rows: np.ndarray):
    """ops.modelpicker_build on the CPU -> (packed (N, H) int16, nseg)."""
    st = ops.modelpicker_build(torch.from_numpy(np.array(rows)))
    return st.packed.numpy(), st.nseg.numpy()


# ---------------------------------------------------------------------
# the contract
# ---------------------------------------------------------------------

def dense_e0_64(post32: np.ndarray) -> float:
    post = post32.astype(np.float64)
    p = np.maximum(post / post.sum(), 1e-12)
    return float(-(p * np.log2(p)).sum())


def dev64(rows: np.ndarray, post32: np.ndarray, gamma: float) -> np.ndarray:
    """C * (dense fp64 entropies - e0_64) per row, hit classes only."""
    post = post32.astype(np.float64)
    N, H = rows.shape
    e0 = dense_e0_64(post32)
    uniq = [np.unique(r) for r in rows]
    K = np.array([len(u) for u in uniq])
    order = np.argsort(-K, kind="stable")
    out = np.zeros(N, dtype=np.float64)
    i = 0
    while i < N:
        kmax = int(K[order[i]])
        cn = max(1, (1 << 22) // (kmax * H))
        idx = order[i:i + cn]
        i += cn
        cls = np.full((len(idx), kmax), -1, dtype=np.int64)
        for a, r in enumerate(idx):
            cls[a, :K[r]] = uniq[r]
        agree = rows[idx][:, None, :] == cls[:, :, None]      # (cn, kmax, H)
        new = post * np.where(agree, gamma, 1.0)
        new = new / new.sum(axis=-1, keepdims=True)
        p = np.maximum(new, 1e-12)
        ent = -(p * np.log2(p)).sum(axis=-1)
        out[idx] = np.where(cls >= 0, ent - e0, 0.0).sum(axis=1)
    return out


# ---------------------------------------------------------------------
# the kernel's formulation
# ---------------------------------------------------------------------

def _fma(a, b, c, dt):
    return (a.astype(np.float64) * np.float64(b)
            + c.astype(np.float64)).astype(dt)


def closed_dev(packed: np.ndarray, nseg: np.ndarray, post32: np.ndarray,
               gamma: float, f32: bool = True,
               fault: str = None) -> np.ndarray:
    """dev per row by sorted segments and the closed form.

    f32=True rounds every operation to fp32 (the twin); faults are for
    f32=False runs: drop_class (the first segment contributes nothing),
    drop_last_model (the first segment loses its last model),
    ignore_pos64 (sorted positions >= 64 carry no mass), drop_T (the
    (g-1) T term, T = sum_A p_h log2 p_h, is left out of T' = S E0 + T).
    """
    assert fault is None or fault in FAULTS
    dt = np.float32 if f32 else np.float64
    pk = packed.astype(np.int32) & 0xffff
    m = pk & 0x7fff
    head = (pk >> 15).astype(bool)
    N, H = m.shape

    # prologue (reference.modelpicker_prologue): fp64, rounded once
    p64 = post32.astype(np.float64)
    p64 = p64 / p64.sum()
    lp = np.log2(np.where(p64 > 0, p64, 1.0))
    e0 = -(p64 * lp).sum()
    p = p64.astype(dt)
    q = np.where(p64 > 0, p64 * (lp + e0), 0.0).astype(dt)
    gm1 = dt(gamma - 1.0)
    glg = dt(gamma * np.log2(gamma))
    inv_ln2 = dt(1.0 / np.log(2.0))

    P, Q = p[m], q[m]                                         # (N, H)
    if fault in ("drop_class", "drop_last_model"):
        first_len = np.where(head.any(axis=1), head.argmax(axis=1), H)
        pos = np.arange(H)[None, :]
        hit = (pos < first_len[:, None] if fault == "drop_class"
               else pos == first_len[:, None] - 1)
        P, Q = np.where(hit, 0, P).astype(dt), np.where(hit, 0, Q).astype(dt)
    if fault == "ignore_pos64":
        P, Q = P.copy(), Q.copy()
        P[:, 64:] = 0
        Q[:, 64:] = 0

    def closed(S, T):
        x = (gm1 * S).astype(dt)
        # T' = S E0 + T: without the (g-1) T term only S E0 is left
        t_term = (S * dt(e0)).astype(dt) if fault == "drop_T" else T
        num = _fma(S, glg, (gm1 * t_term).astype(dt), dt)
        lg = (np.log1p(x.astype(np.float64)).astype(dt) * inv_ln2).astype(dt)
        return (lg - (num / (dt(1) + x).astype(dt)).astype(dt)).astype(dt)

    S = np.zeros(N, dtype=dt)
    T = np.zeros(N, dtype=dt)
    dev = np.zeros(N, dtype=dt)
    for j in range(H):
        h = head[:, j]
        if h.any():
            dev = np.where(h, (dev + closed(S, T)).astype(dt), dev)
            S = np.where(h, dt(0), S)
            T = np.where(h, dt(0), T)
        S = (S + P[:, j]).astype(dt)
        T = (T + Q[:, j]).astype(dt)
    dev = np.where(nseg > 1, (dev + closed(S, T)).astype(dt), dev)
    return dev.astype(np.float64)


# ---------------------------------------------------------------------
# tolerances
# ---------------------------------------------------------------------

GPU_H = (3, 64, 65, 128, 1000, 1024)
GPU_C = (2, 10, 1000, 32767)
GPU_EPS = (0.36, 0.49)
GPU_POSTERIORS = ("uniform", "spread60", "conc2000")
# (H, C, posterior) of the mutation floors and the share of rows a
# dropped hit class must move past the tolerance
FLOOR_SHAPES = (
    (64, 10, "uniform", 0.90),
    (65, 1000, "spread3", 0.90),
    (128, 1000, "uniform", 0.90),
    (128, 1000, "spread60", 0.90),
    (1024, 300, "spread60", 0.70),
)


@functools.lru_cache(maxsize=None)
def twin_error(H: int, C: int, kind: str, eps: float) -> float:
    """max over the active make_rows rows of |fp32 twin - dev64|."""
    rows, active = make_rows(H, C)
    post = make_posterior(H, kind, eps)
    packed, nseg = build(rows)
    twin = closed_dev(packed, nseg, post, gamma_of(eps), f32=True)
    ref = dev64_cached(H, C, kind, eps)
    return float(np.abs(twin - ref)[active].max())


@functools.lru_cache(maxsize=None)
def dev64_cached(H: int, C: int, kind: str, eps: float) -> np.ndarray:
    rows, _ = make_rows(H, C)
    out = dev64(rows, make_posterior(H, kind, eps), gamma_of(eps))
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def measured_tolerance(H: int, C: int) -> float:
    """MARGIN x the twin's worst error on the shape, over the GPU test's
    posteriors and epsilons."""
    return MARGIN * max(twin_error(H, C, kind, eps)
                        for kind in GPU_POSTERIORS for eps in GPU_EPS)


@functools.lru_cache(maxsize=None)
def measured_floor_tolerance(H: int, C: int, kind: str,
                             eps: float = 0.45) -> float:
    """MARGIN x the twin's worst error on the floor problem itself."""
    rows = uniform_rows(H, C)
    post = make_posterior(H, kind, eps)
    packed, nseg = build(rows)
    twin = closed_dev(packed, nseg, post, gamma_of(eps), f32=True)
    return MARGIN * float(np.abs(twin - dev64(rows, post,
                                              gamma_of(eps))).max())
