"""fp64 tests of the label-update HIP kernels (GPU,
coda_amd/ops/hip/label.hip): pi_hat_delta and
its two H-windowed variants, pi_marginal (both routes), mixture_entropy,
col_add and dirichlet_add, each called on its own with CPU-built
inputs. They run inside the captured label-update graph on every label.

These kernels are plain fp32 sums, so the reference is the fp64 sum of
the same fp32 (or exactly up-cast) inputs and every bound below is
REASONED, NOT MEASURED. With u = 2^-24 (half an fp32 ulp, the relative
error of one rounding) and non-negative terms, a sum in which no term
passes through more than d roundings is within d * u * (1 + d * u) of
the exact sum, relative, whatever the order:

  pi_hat_delta*   the up-cast is exact and each term is added as it is:
                  H adds in the plain kernel; in the windowed kernels at
                  most Hc adds and one combine per window, then KH adds
                  of the partials: d <= H + KH, KH = ceil(H / hc) (KH = 1
                  for the plain kernel). `part` and `t_part` share the
                  accumulation pattern and must be BIT-equal.
  pi_marginal     per term one correctly rounded reciprocal and one
                  multiply (2), the block's slab of rows_per_block rows
                  plus the merge of its two accumulators, then the
                  16-way reduce over ceil(G / 16) slabs (+ 1) and the
                  final 16 (+ 1): d <= 2 + rpb + 1 + ceil(G / 16) + 1 +
                  16 + 1.
  mixture0        one multiply, the slab of ceil(C / 64) rows, then the
                  combine's 16 adds per accumulator and 3 to merge the
                  four: d <= 1 + ceil(C / 64) + 16 + 3.
  col_add,        one fp32 add per touched element: bit-equal to the
  dirichlet_add   same add in torch; every other element untouched.

h0 (the mixture's log2 entropy) goes through log2 and a 256-thread
tree: it gets MARGIN = 16 times the spread of an fp32 twin of the
reference against fp64, computed on the test's own inputs when the
test runs (never from kernel output). No spread counts for less than
one fp32 ulp of 1 (E_ULP, the convention of tests/test_table_kernels.py
for entropies): h0 lies in [1, 10], where its own fp32 spacing is 1 to
8 ulps of 1, and at H = 4 the twin's four terms happen to round almost
exactly (spread 1.4e-8, a ninth of h0's spacing).

TestFaultFloors (CPU, not marked gpu) shows that the pi_hat_delta
inputs make a dropped tail model, and cls[h + 1] used for model h, move
the sum by more than 10 bounds.
"""
from __future__ import annotations

import functools

import pytest
import torch

from tests.pair_ref import _f32c, _r32, _sum32

U = 2.0 ** -24
MARGIN = 16.0
E_ULP = 2.0 ** -23
BLOCK = 256

DTYPES = {"fp32": torch.float32, "fp16": torch.float16,
          "bf16": torch.bfloat16, "fp8": torch.float8_e4m3fn}
PI_N = (1, 255, 257, 513)
PI_C = (1, 7)
# (H, hc): window tails of 1, 3 and 1 models, hc > H, and no tail
PI_WINDOWS = ((9, 4), (11, 7), (6, 5), (5, 8), (8, 4))


def sum_bound(d: int) -> float:
    return d * U * (1 + d * U)


# ---------------------------------------------------------------------
# CPU inputs and references
# ---------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def pi_inputs(H: int, N: int, C: int, dt: str):
    """preds (H, N, C) in [0.05, 1] rounded to the storage dtype on the
    CPU (so the kernel's up-cast is exact; every value is a normal
    number of every dtype), and cls (H,) int32 that picks class 0 and
    class C - 1 and changes from every model to the next."""
    g = torch.Generator().manual_seed(100 + 7 * H + N + 1000 * C)
    preds = (0.05 + 0.95 * torch.rand(H, N, C, generator=g)).to(DTYPES[dt])
    cls = (torch.arange(H) * (C - 1)) % C if C > 1 else torch.zeros(H)
    cls = cls.to(torch.int32)
    if C > 1:
        assert 0 in cls.tolist() and C - 1 in cls.tolist()
    return preds, cls


def pi_ref(preds, cls, h0=0, h1=None, *, drop_tail=False, next_cls=False):
    """(N,) fp64 sum over models h0 <= h < h1 of preds[h, :, cls[h]].
    Faults: drop_tail leaves the window's last model out; next_cls reads
    cls[h + 1] for model h (the last model keeps its own)."""
    H = preds.shape[0]
    h1 = H if h1 is None else min(h1, H)
    c = cls.long()
    if next_cls:
        c = torch.cat([c[1:], c[-1:]])
    hs = torch.arange(h0, h1 - 1 if drop_tail else h1)
    return preds.double()[hs, :, c[hs]].sum(0)


def marginal_inputs(N: int, C: int):
    """adjusted (N, C) in [0.1, 1.1), row_sums NOT the row sums (a
    kernel that recomputed them would differ); rows 0 and N // 2 have
    row_sums 0 and 1e-13, below the 1e-12 clamp, and entries scaled so
    that they still matter (about 0.1 after the clamped division)."""
    g = torch.Generator().manual_seed(200 + N + 31 * C)
    adjusted = torch.rand(N, C, generator=g) + 0.1
    row_sums = adjusted.sum(-1) * (0.9 + 0.2 * torch.rand(N, generator=g))
    small = {0: 0.0, N // 2: 1e-13} if N > 1 else {0: 0.0}
    for n, rs in small.items():
        adjusted[n] *= 1e-13
        row_sums[n] = rs
    return adjusted.contiguous(), row_sums.contiguous()


def marginal_ref(adjusted, row_sums):
    inv = 1.0 / row_sums.double().clamp_min(_f32c(1e-12, torch.float64))
    return (adjusted.double() * inv.unsqueeze(1)).sum(0)


def marginal_route(N: int, C: int):
    """(vector route?, G, rows per block) as the binding chooses them."""
    if C % 4 == 0 and C <= 4 * BLOCK:
        awpb = (C // 4 + 63) // 64
        G = min(1024, max(256, 1024 // awpb))
        return True, G, -(-N // G)
    return False, 1536, -(-N // 1536)


def mix_inputs(H: int, C: int, tiny: bool = False):
    """P(best)-like rows (C, H) summing to 1 and a pi (C,) summing to 1;
    tiny puts every entry of model 0 near 1e-14, below the 1e-12 clamp
    of the entropy."""
    g = torch.Generator().manual_seed(300 + H + 31 * C)
    rows = torch.rand(C, H, generator=g) ** 4 + 1e-4
    rows /= rows.sum(-1, keepdim=True)
    if tiny:
        rows[:, 0] = 1e-14 * (1 + torch.rand(C, generator=g))
    pi = torch.rand(C, generator=g) + 0.2
    pi /= pi.sum()
    return rows.contiguous(), pi


def mix_ref(rows, pi, *, f32=False):
    """(mixture0 (H,), h0) fp64; f32: every operation rounded to fp32
    (64 strided accumulators over the classes, 256 over the models)."""
    prod = rows.double().t() * pi.double()                      # (H, C)
    mix = _sum32(_r32(prod), 64) if f32 else prod.sum(-1)
    m = mix.clamp_min(_f32c(1e-12, torch.float64))
    if not f32:
        return mix, -(m * torch.log2(m)).sum()
    return mix, -_sum32(_r32(m * _r32(torch.log2(m))), 256)


# ---------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------

@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ext():
    import coda_amd.ops as ops
    assert ops.hip_available(), \
        "HIP extension must be built on GPU boxes (python build_hip.py)"
    return ops._ext


def _rel(got, ref) -> float:
    return float(((got.double() - ref).abs() / ref).max())


@pytest.mark.gpu
class TestPiHatDelta:
    @pytest.mark.parametrize("dt", list(DTYPES))
    @pytest.mark.parametrize("H,hc", PI_WINDOWS)
    def test_three_kernels_vs_fp64(self, ext, dev, H, hc, dt):
        """pi_hat_delta, pi_hat_delta_part and pi_hat_delta_t_part on
        every (N, C): the sum, each window's partial, and part == t_part
        bit for bit."""
        KH = -(-H // min(hc, H))
        worst = [0.0, 0.0, 0.0]
        for N in PI_N:
            for C in PI_C:
                preds, cls = pi_inputs(H, N, C, dt)
                ref = pi_ref(preds, cls)
                p_d, c_d = preds.to(dev), cls.to(dev)
                t_d = preds.permute(0, 2, 1).contiguous().to(dev)
                plain = ext.pi_hat_delta(p_d, c_d)
                part = ext.pi_hat_delta_part(p_d, c_d, hc)
                t_part = ext.pi_hat_delta_t_part(t_d, c_d, hc)
                assert plain.shape == (N,) and plain.dtype == torch.float32
                assert part.shape == (KH, N) == t_part.shape
                assert torch.equal(part, t_part), (N, C)
                e = _rel(plain.cpu(), ref)
                assert e <= sum_bound(H + 1), (N, C, e)
                e_sum = _rel(part.sum(0).cpu(), ref)
                assert e_sum <= sum_bound(H + KH), (N, C, e_sum)
                e_win = 0.0
                for k in range(KH):
                    h0 = k * min(hc, H)
                    win = pi_ref(preds, cls, h0, h0 + hc)
                    e_win = max(e_win, _rel(part[k].cpu(), win))
                assert e_win <= sum_bound(min(hc, H) + 1), (N, C, e_win)
                worst = [max(w, x) for w, x in zip(worst,
                                                   (e, e_sum, e_win))]
        print(f"pi_hat_delta {(H, hc, dt)}: plain {worst[0]:.3g} (bound "
              f"{sum_bound(H + 1):.3g}) part sum {worst[1]:.3g} (bound "
              f"{sum_bound(H + KH):.3g}) window {worst[2]:.3g} (bound "
              f"{sum_bound(min(hc, H) + 1):.3g})")


VECTOR_SHAPES = [(1, 4), (7, 8), (9219, 4), (2307, 1024)]
SLAB_SHAPES = [(1, 1), (9, 3), (4609, 5), (300, 255), (300, 1028),
               (4609, 2048), (33, 2047)]


@pytest.mark.gpu
class TestPiMarginal:
    @pytest.mark.parametrize("N,C", VECTOR_SHAPES + SLAB_SHAPES)
    def test_vs_fp64(self, ext, dev, N, C):
        """Both routes: the 8-row (vector) and 2-row (slab) unrolls with
        their tails, C in (1024, 2048], rows below the 1e-12 clamp, and
        two calls bit-equal."""
        vector, G, rpb = marginal_route(N, C)
        assert vector == ((N, C) in VECTOR_SHAPES)
        adjusted, row_sums = marginal_inputs(N, C)
        assert float(row_sums.min()) == 0.0
        ref = marginal_ref(adjusted, row_sums)
        a_d, r_d = adjusted.to(dev), row_sums.to(dev)
        got = ext.pi_marginal(a_d, r_d)
        again = ext.pi_marginal(a_d, r_d)
        assert got.shape == (C,) and bool(torch.isfinite(got).all())
        assert torch.equal(got, again), "second call differs"
        d = 2 + rpb + 1 + -(-G // 16) + 1 + 16 + 1
        err = _rel(got.cpu(), ref)
        print(f"pi_marginal {(N, C)} {'vector' if vector else 'slab'} "
              f"G={G} rpb={rpb}: rel err {err:.3g} bound "
              f"{sum_bound(d):.3g}")
        assert err <= sum_bound(d), (N, C, err)


MIX_H = (4, 8, 252, 256, 260, 1024)
MIX_C = (1, 63, 64, 65, 1000)


@pytest.mark.gpu
class TestMixtureEntropy:
    @pytest.mark.parametrize("C", MIX_C)
    @pytest.mark.parametrize("H", MIX_H)
    def test_vs_fp64(self, dev, H, C):
        """ops.mixture_entropy on the kernel route (H % 4 == 0, H <=
        1024): empty class slabs (C < 64), one- and two-row slabs."""
        self._check(dev, H, C, False)

    def test_entries_below_the_clamp(self, dev):
        self._check(dev, 8, 65, True)

    @staticmethod
    def _check(dev, H, C, tiny):
        import coda_amd.ops as ops
        assert ops.hip_available()
        rows, pi = mix_inputs(H, C, tiny)
        mix64, h64 = mix_ref(rows, pi)
        _, h32 = mix_ref(rows, pi, f32=True)
        spread = float((h32 - h64).abs())
        if tiny:
            assert bool((mix64 < 1e-12).any())
        m0, h0 = ops.mixture_entropy(rows.to(dev), pi.to(dev))
        assert m0.shape == (H,) and h0.shape == ()
        e_mix = _rel(m0.cpu(), mix64)
        bound = sum_bound(1 + -(-C // 64) + 16 + 3)
        e_h = abs(float(h0) - float(h64))
        tol = MARGIN * max(spread, E_ULP)
        print(f"mixture_entropy {(H, C)}{' tiny' if tiny else ''}: "
              f"mixture0 rel {e_mix:.3g} (bound {bound:.3g}) h0 err "
              f"{e_h:.3g} (tol {tol:.3g}, twin {spread:.3g})")
        assert e_mix <= bound, (H, C, e_mix)
        assert e_h <= tol, (H, C, e_h)


@pytest.mark.gpu
class TestScatterAdds:
    @pytest.mark.parametrize("last", [False, True])
    @pytest.mark.parametrize("N", [1, 255, 257])
    def test_col_add(self, ext, dev, N, last):
        C = 5
        y = C - 1 if last else 0
        g = torch.Generator().manual_seed(400 + N)
        adjusted = torch.rand(N, C, generator=g)
        row_sums = torch.rand(N, generator=g) + 1
        delta = torch.rand(N, generator=g)
        want_a = adjusted.clone()
        want_a[:, y] = adjusted[:, y] + delta
        a_d, r_d = adjusted.to(dev), row_sums.to(dev)
        ext.col_add(a_d, r_d, torch.tensor([y], device=dev), delta.to(dev))
        assert torch.equal(a_d.cpu(), want_a)
        assert torch.equal(r_d.cpu(), row_sums + delta)

    @pytest.mark.parametrize("last", [False, True])
    @pytest.mark.parametrize("H", [1, 255, 257])
    def test_dirichlet_add(self, ext, dev, H, last):
        C = 4
        y = C - 1 if last else 0
        g = torch.Generator().manual_seed(500 + H)
        dirs = torch.rand(H, C, C, generator=g) + 0.5
        cls = torch.randint(0, C, (H,), generator=g)
        cls[0] = C - 1 if last else 0
        if H > 1:
            cls[0], cls[-1] = 0, C - 1
        lr = 0.3
        want = dirs.clone()
        want[torch.arange(H), y, cls] = dirs[torch.arange(H), y, cls] \
            + torch.tensor(lr, dtype=torch.float32)
        d_d = dirs.to(dev)
        ext.dirichlet_add(d_d, torch.tensor([y], device=dev), cls.to(dev),
                          lr)
        assert torch.equal(d_d.cpu(), want)


# ---------------------------------------------------------------------
# CPU: what the pi_hat_delta bound can see
# ---------------------------------------------------------------------

class TestFaultFloors:
    FLOOR = 10.0

    @pytest.mark.parametrize("dt", list(DTYPES))
    @pytest.mark.parametrize("H,hc", PI_WINDOWS)
    def test_dropped_tail_model_and_shifted_class(self, H, hc, dt):
        """A 4-way unroll that loses its tail drops the last model of a
        window; an off-by-one class index reads cls[h + 1]. Every term
        is >= 0.05 of a sum <= H, so the first moves EVERY point by >=
        0.05 / 11; the second is checked on the worst point, as the GPU
        test sees it, and needs more than one class."""
        KH = -(-H // min(hc, H))
        for N in PI_N:
            for C in PI_C:
                preds, cls = pi_inputs(H, N, C, dt)
                ref = pi_ref(preds, cls)
                lost = pi_ref(preds, cls, drop_tail=True)
                moved = ((lost - ref).abs() / ref).min()
                assert float(moved) >= self.FLOOR * sum_bound(H + KH)
                if C > 1:
                    off = pi_ref(preds, cls, next_cls=True)
                    moved = ((off - ref).abs() / ref).max()
                    assert float(moved) >= self.FLOOR * sum_bound(H + KH)
