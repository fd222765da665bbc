// gfx950 kernels of the per-label posterior update: what add_label moves
// besides the table rows (table.hip).
//
// Kernel inventory (host bindings at the bottom):
//   pi_hat_delta_kernel    rank-1 posterior-marginal increment
//   pi_hat_delta_part      H-chunked variant for wide pools (blockIdx.y)
//   pi_hat_delta_t_part    its class-major (H, C, N) twin
//   dirichlet_add_kernel   dir[h, y, cls_h] += lr posterior scatter
//   col_add_kernel         fused adjusted[:, y] += delta; row_sums += delta
//   pi_marginal[_part]     streaming scaled column sum for pi_hat: slab
//                          partials, then pi_marginal_reduce_kernel twice
//   mix_part/combine       weighted column sum + mixture entropy

#include "host_util.h"
#include <algorithm>
#include <vector>

namespace {

// Rank-1 pi_hat increment: out[n] = sum_h preds[h, n, cls[h]] - the exact
// per-label posterior-marginal change (only Dirichlet row true_class
// moves; coda/coda.py:316-317). One thread per point; consecutive
// threads read consecutive n (coalesced); the class index is
// wave-uniform per model. fp32, fp16, bf16 and fp8 prediction storage;
// every dtype up-casts exactly, so fp16 storage of an fp16-representable
// pool sums the very fp32 values the fp32 kernel does.
template <typename T>
__global__ void __launch_bounds__(BLOCK)
pi_hat_delta_kernel(const T* __restrict__ preds,  // (H, N, C)
                    const int* __restrict__ cls,  // (H,)
                    float* __restrict__ out,      // (N,)
                    int H, long long N, int C) {
    const long long n = (long long)blockIdx.x * BLOCK + threadIdx.x;
    if (n >= N) return;
    float acc = 0.f;
    for (int h = 0; h < H; ++h)
        acc += (float)preds[((long long)h * N + n) * C + cls[h]];
    out[n] = acc;
}

// Dirichlet posterior update: dir[h, y, cls_h] += lr for every model h.
// The torch formulation (one_hot -> index_add_ over dim 1 of (H,C,C))
// routes to indexFuncLargeIndex at ~914 us/call despite only H real
// nonzeros; this is an H-thread scatter.
__global__ void __launch_bounds__(BLOCK, 4)
dirichlet_add_kernel(float* __restrict__ dir,      // (H, C, C)
                     const long* __restrict__ y,   // (1,)
                     const long* __restrict__ cls, // (H,) argmax class
                     float lr, int H, int C) {
    const int h = blockIdx.x * BLOCK + threadIdx.x;
    if (h >= H) return;
    dir[((size_t)h * C + y[0]) * C + cls[h]] += lr;
}

// Fused posterior-marginal column update: adjusted[n, y] += delta[n] and
// row_sums[n] += delta[n] in one pass. torch's index_add_ over dim 1
// with a single index parallelizes over the 1-element index list
// (indexFuncLargeIndex: 916 us/call at N=50k - the largest per-step
// kernel in the profiled hot loop); this is a ~10 us elementwise pass.
// y stays a device tensor so the op is hipGraph-replay safe.
__global__ void __launch_bounds__(BLOCK, 4)
col_add_kernel(float* __restrict__ adjusted,       // (N, C)
               float* __restrict__ row_sums,       // (N,)
               const long* __restrict__ y,         // (1,)
               const float* __restrict__ delta,    // (N,)
               long long N, int C) {
    const long long n = (long long)blockIdx.x * BLOCK + threadIdx.x;
    if (n >= N) return;
    const float d = delta[n];
    adjusted[n * C + y[0]] += d;
    row_sums[n] += d;
}

// H-chunked variant for wide model pools: with only N threads the plain
// kernel cannot fill 256 CUs (N=5k, H=10k left it 13x slower than its
// memory floor). blockIdx.y sums an H window into partial[(k, n)]; the
// host reduces partials with a deterministic torch sum (no atomics, so
// trajectories stay bit-reproducible).
template <typename T>
__global__ void __launch_bounds__(BLOCK, 4)
pi_hat_delta_part_kernel(const T* __restrict__ preds,   // (H, N, C)
                         const int* __restrict__ cls,   // (H,)
                         float* __restrict__ partial,   // (KH, N)
                         int H, long long N, int C, int Hc) {
    const int hbeg = blockIdx.y * Hc;
    const int hend = min(H, hbeg + Hc);
    const long long n = (long long)blockIdx.x * BLOCK + threadIdx.x;
    if (n >= N) return;
    // 4 accumulators: the single-chain form serializes ~H/KH scattered
    // loads per thread (wide pools: 1.24 ms at 10k models, 3x floor)
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
    int h = hbeg;
    for (; h + 3 < hend; h += 4) {
        a0 += (float)preds[((long long)h * N + n) * C + cls[h]];
        a1 += (float)preds[((long long)(h + 1) * N + n) * C + cls[h + 1]];
        a2 += (float)preds[((long long)(h + 2) * N + n) * C + cls[h + 2]];
        a3 += (float)preds[((long long)(h + 3) * N + n) * C + cls[h + 3]];
    }
    for (; h < hend; ++h)
        a0 += (float)preds[((long long)h * N + n) * C + cls[h]];
    partial[(size_t)blockIdx.y * N + n] = (a0 + a1) + (a2 + a3);
}


// Class-major twin: preds_t (H, C, N) makes the per-label gather
// preds_t[h, cls_h, :] CONTIGUOUS over n (the row-major layout reads
// one 4-B element per 64-B sector: 150 us at the headline shape and
// 1.2 ms at 10k models, both AT the random-sector floor - the mirror
// turns the same op into a 25 MB coalesced stream).  Accumulation
// pattern matches pi_hat_delta_part_kernel exactly, so routing through
// the mirror is bitwise-neutral.
template <typename T>
__global__ void __launch_bounds__(BLOCK)
pi_hat_delta_t_part_kernel(const T* __restrict__ preds_t, // (H, C, N)
                           const int* __restrict__ cls,   // (H,)
                           float* __restrict__ partial,   // (KH, N)
                           int H, long long N, int C, int Hc) {
    const int hbeg = blockIdx.y * Hc;
    const int hend = min(H, hbeg + Hc);
    const long long n = (long long)blockIdx.x * BLOCK + threadIdx.x;
    if (n >= N) return;
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
    int h = hbeg;
    for (; h + 3 < hend; h += 4) {
        a0 += (float)preds_t[((long long)h * C + cls[h]) * N + n];
        a1 += (float)preds_t[((long long)(h + 1) * C + cls[h + 1]) * N + n];
        a2 += (float)preds_t[((long long)(h + 2) * C + cls[h + 2]) * N + n];
        a3 += (float)preds_t[((long long)(h + 3) * C + cls[h + 3]) * N + n];
    }
    for (; h < hend; ++h)
        a0 += (float)preds_t[((long long)h * C + cls[h]) * N + n];
    partial[(size_t)blockIdx.y * N + n] = (a0 + a1) + (a2 + a3);
}

// pi marginal: out[c] = sum_n adjusted[n, c] / max(row_sums[n], 1e-12)
// (reference coda/coda.py:229-233 without materializing the normalized
// (N, C) matrix). Slab partials for every shape the vector kernel below
// does not take (C % 4 != 0, or 1024 < C <= 2048): each thread owns fixed
// columns c = tid + k*BLOCK (register accumulators, no LDS), a block
// streams its row slab and stores one partial row (G, Cpad), pad columns
// zeroed; pi_marginal_reduce_kernel sums the slabs in a fixed order. The
// earlier schedule ended in one atomicAdd per (block, column), whose
// order - and with it the low bits of pi_hat and of everything computed
// from it - changed from run to run.
__global__ void __launch_bounds__(BLOCK)
pi_marginal_kernel(const float* __restrict__ adjusted,  // (N, C)
                   const float* __restrict__ row_sums,  // (N,)
                   float* __restrict__ partial,         // (G, Cpad)
                   long long N, int C, int Cpad) {
    const int tid = threadIdx.x;
    const long long rows_per_block =
        (N + gridDim.x - 1) / gridDim.x;
    const long long n0 = (long long)blockIdx.x * rows_per_block;
    const long long n1 = min(n0 + rows_per_block, N);
    const int ncols = (Cpad + BLOCK - 1) / BLOCK;
    float acc[8];  // supports C <= 8*BLOCK = 2048
    for (int k = 0; k < ncols && k < 8; ++k) acc[k] = 0.f;
    long long n = n0;
    for (; n + 1 < n1; n += 2) {  // 2-row unroll: 2x loads in flight
        const float inv0 = 1.0f / fmaxf(row_sums[n], 1e-12f);
        const float inv1 = 1.0f / fmaxf(row_sums[n + 1], 1e-12f);
        const float* r0 = adjusted + n * C;
        const float* r1 = r0 + C;
        for (int k = 0; k < ncols && k < 8; ++k) {
            const int c = tid + k * BLOCK;
            if (c < C) acc[k] += r0[c] * inv0 + r1[c] * inv1;
        }
    }
    for (; n < n1; ++n) {
        const float inv = 1.0f / fmaxf(row_sums[n], 1e-12f);
        const float* row = adjusted + n * C;
        for (int k = 0; k < ncols && k < 8; ++k) {
            const int c = tid + k * BLOCK;
            if (c < C) acc[k] += row[c] * inv;
        }
    }
    // an empty slab (more blocks than rows) stores its zeros too
    float* prow = partial + (long long)blockIdx.x * Cpad;
    for (int k = 0; k < ncols && k < 8; ++k) {
        const int c = tid + k * BLOCK;
        if (c < Cpad) prow[c] = acc[k];
    }
}


// pi marginal, vector shapes (C % 4 == 0, C <= 1024): the single-kernel
// schedule above is ATOMIC-bound at the headline shape (1536 blocks x
// 250 lanes x 4 atomicAdds onto 1000 floats = 165 us measured vs a
// ~25 us streaming floor; scripts/pi_marginal_probe.py has the sweep).
// Three-kernel deterministic replacement, 36 us measured:
//   1. slab partials  (G, Cpad)  - thread tid owns one float4 of
//      columns, 8-row-unrolled stream over the block's row slab,
//      plain coalesced float4 stores (no atomics);
//   2. 16-way G-reduce (16, Cpad) - fixed slab boundaries;
//   3. final 16-row sum -> out    - fixed order, so the whole chain is
//      run-to-run DETERMINISTIC (the atomic schedule was not).
__global__ void __launch_bounds__(BLOCK)
pi_marginal_part_kernel(const float* __restrict__ adjusted,  // (N, C)
                        const float* __restrict__ row_sums,  // (N,)
                        float* __restrict__ partial,         // (G, Cpad)
                        long long N, int C, int Cpad) {
    const int tid = threadIdx.x;
    const long long rows_per_block = (N + gridDim.x - 1) / gridDim.x;
    const long long n0 = (long long)blockIdx.x * rows_per_block;
    const long long n1 = min(n0 + rows_per_block, N);
    const int c4 = tid * 4;
    if (c4 >= C) return;
    float4 acc = {0.f, 0.f, 0.f, 0.f};
    float4 acc2 = {0.f, 0.f, 0.f, 0.f};
    long long n = n0;
    for (; n + 7 < n1; n += 8) {
        float inv[8];
        float4 v[8];
#pragma unroll
        for (int r = 0; r < 8; ++r)
            inv[r] = 1.0f / fmaxf(row_sums[n + r], 1e-12f);
#pragma unroll
        for (int r = 0; r < 8; ++r)
            v[r] = *reinterpret_cast<const float4*>(
                adjusted + (n + r) * C + c4);
#pragma unroll
        for (int r = 0; r < 8; r += 2) {
            acc.x += v[r].x * inv[r];  acc2.x += v[r + 1].x * inv[r + 1];
            acc.y += v[r].y * inv[r];  acc2.y += v[r + 1].y * inv[r + 1];
            acc.z += v[r].z * inv[r];  acc2.z += v[r + 1].z * inv[r + 1];
            acc.w += v[r].w * inv[r];  acc2.w += v[r + 1].w * inv[r + 1];
        }
    }
    for (; n < n1; ++n) {
        const float inv = 1.0f / fmaxf(row_sums[n], 1e-12f);
        const float4 v = *reinterpret_cast<const float4*>(
            adjusted + n * C + c4);
        acc.x += v.x * inv; acc.y += v.y * inv;
        acc.z += v.z * inv; acc.w += v.w * inv;
    }
    acc.x += acc2.x; acc.y += acc2.y; acc.z += acc2.z; acc.w += acc2.w;
    *reinterpret_cast<float4*>(
        partial + (long long)blockIdx.x * Cpad + c4) = acc;
}

// Weighted column sum + mixture entropy:
//   mixture0[h] = sum_c pi[c] * rows[c, h];  H0 = -sum_h m log2 m,
//   m = clamp(mixture0, 1e-12)   (ops/reference.py mixture_entropy).
// torch reduces the (C, H) column sum with a 32-thread launch (~22 us
// measured at C=1000, H=128 - twice per step).  Two kernels, fixed
// order (deterministic): G-block row-slab partials, then one block
// combines and does the entropy contraction.
__global__ void __launch_bounds__(BLOCK)
mix_part_kernel(const float* __restrict__ rows,  // (C, H)
                const float* __restrict__ pi,    // (C,)
                float* __restrict__ partial,     // (G, H)
                int C, int H) {
    const int tid = threadIdx.x;
    const int per = (C + gridDim.x - 1) / gridDim.x;
    const int c0 = blockIdx.x * per, c1 = min(c0 + per, C);
    const int h4 = tid * 4;
    if (h4 >= H) return;
    float4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int c = c0; c < c1; ++c) {
        const float w = pi[c];
        const float4 v = *reinterpret_cast<const float4*>(
            rows + (size_t)c * H + h4);
        acc.x += v.x * w; acc.y += v.y * w;
        acc.z += v.z * w; acc.w += v.w * w;
    }
    *reinterpret_cast<float4*>(partial + (size_t)blockIdx.x * H + h4) = acc;
}

__global__ void __launch_bounds__(BLOCK)
mix_combine_kernel(const float* __restrict__ partial,  // (G, H)
                   float* __restrict__ mixture0,       // (H,)
                   float* __restrict__ h0,             // (1,)
                   int G, int H) {
    const int tid = threadIdx.x;
    const int h4 = tid * 4;
    float ent = 0.f;
    if (h4 < H) {
        // 4-way G unroll: at H=128 only 32 threads are active and the
        // serial strided walk was ~17 us latency-bound; independent
        // accumulators keep 4 loads in flight
        float4 acc = {0.f, 0.f, 0.f, 0.f};
        float4 a1 = {0.f, 0.f, 0.f, 0.f};
        float4 a2 = {0.f, 0.f, 0.f, 0.f};
        float4 a3 = {0.f, 0.f, 0.f, 0.f};
        int g = 0;
        for (; g + 3 < G; g += 4) {
            const float4 v0 = *reinterpret_cast<const float4*>(
                partial + (size_t)g * H + h4);
            const float4 v1 = *reinterpret_cast<const float4*>(
                partial + (size_t)(g + 1) * H + h4);
            const float4 v2 = *reinterpret_cast<const float4*>(
                partial + (size_t)(g + 2) * H + h4);
            const float4 v3 = *reinterpret_cast<const float4*>(
                partial + (size_t)(g + 3) * H + h4);
            acc.x += v0.x; acc.y += v0.y; acc.z += v0.z; acc.w += v0.w;
            a1.x += v1.x; a1.y += v1.y; a1.z += v1.z; a1.w += v1.w;
            a2.x += v2.x; a2.y += v2.y; a2.z += v2.z; a2.w += v2.w;
            a3.x += v3.x; a3.y += v3.y; a3.z += v3.z; a3.w += v3.w;
        }
        for (; g < G; ++g) {
            const float4 v = *reinterpret_cast<const float4*>(
                partial + (size_t)g * H + h4);
            acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w;
        }
        acc.x += a1.x + a2.x + a3.x; acc.y += a1.y + a2.y + a3.y;
        acc.z += a1.z + a2.z + a3.z; acc.w += a1.w + a2.w + a3.w;
        *reinterpret_cast<float4*>(mixture0 + h4) = acc;
        const float m[4] = {fmaxf(acc.x, 1e-12f), fmaxf(acc.y, 1e-12f),
                            fmaxf(acc.z, 1e-12f), fmaxf(acc.w, 1e-12f)};
#pragma unroll
        for (int j = 0; j < 4; ++j) ent -= m[j] * __log2f(m[j]);
    }
    __shared__ float se[BLOCK];
    se[tid] = ent;
    __syncthreads();
    for (int s = BLOCK / 2; s > 0; s >>= 1) {
        if (tid < s) se[tid] += se[tid + s];
        __syncthreads();
    }
    if (tid == 0) h0[0] = se[0];
}

// rows-reduce: out[oy, c] = sum over this block.y's fixed slice of
// in[g, c].  Used twice: (G -> 16 slices) then (16 -> 1, oy = 0).
__global__ void __launch_bounds__(BLOCK)
pi_marginal_reduce_kernel(const float* __restrict__ in,   // (G, Cpad)
                          float* __restrict__ out,        // (gridDim.y, ostride)
                          int G, int C, int Cpad, int ostride) {
    const int c4 = (blockIdx.x * BLOCK + threadIdx.x) * 4;
    if (c4 >= C) return;
    const int gs = (G + gridDim.y - 1) / gridDim.y;
    const int g0 = blockIdx.y * gs, g1 = min(g0 + gs, G);
    float4 acc = {0.f, 0.f, 0.f, 0.f};
    float4 acc2 = {0.f, 0.f, 0.f, 0.f};
    int g = g0;
    for (; g + 1 < g1; g += 2) {
        const float4 a = *reinterpret_cast<const float4*>(
            in + (long long)g * Cpad + c4);
        const float4 b = *reinterpret_cast<const float4*>(
            in + (long long)(g + 1) * Cpad + c4);
        acc.x += a.x; acc.y += a.y; acc.z += a.z; acc.w += a.w;
        acc2.x += b.x; acc2.y += b.y; acc2.z += b.z; acc2.w += b.w;
    }
    if (g < g1) {
        const float4 a = *reinterpret_cast<const float4*>(
            in + (long long)g * Cpad + c4);
        acc.x += a.x; acc.y += a.y; acc.z += a.z; acc.w += a.w;
    }
    *reinterpret_cast<float4*>(out + (long long)blockIdx.y * ostride + c4) =
        {acc.x + acc2.x, acc.y + acc2.y, acc.z + acc2.z, acc.w + acc2.w};
}

}  // namespace

// ---------------------------------------------------------------------------
// Host bindings
// ---------------------------------------------------------------------------

static const char* const kPiHatDtypes =
    "pi_hat_delta kernel supports fp32/fp16/bf16/fp8";

torch::Tensor pi_hat_delta(torch::Tensor preds, torch::Tensor cls) {
    TORCH_CHECK(preds.is_cuda() && preds.is_contiguous(),
                "preds must be contiguous on a ROCm device");
    TORCH_CHECK(cls.scalar_type() == torch::kInt32, "cls must be int32");
    const int H = preds.size(0), C = preds.size(2);
    const long long N = preds.size(1);
    auto out = torch::empty({N}, preds.options().dtype(torch::kFloat32));
    const int blocks = (int)((N + BLOCK - 1) / BLOCK);
    dispatch_storage(preds, kPiHatDtypes, [&](auto* p) {
        launch(pi_hat_delta_kernel<elem_t<decltype(p)>>, dim3(blocks), 0,
               p, cls.data_ptr<int>(), out.data_ptr<float>(), H, N, C);
    });
    return out;
}


torch::Tensor pi_hat_delta_part(torch::Tensor preds, torch::Tensor cls,
                                int64_t hc) {
    TORCH_CHECK(preds.is_cuda() && preds.is_contiguous(),
                "preds must be contiguous on a ROCm device");
    TORCH_CHECK(cls.scalar_type() == torch::kInt32, "cls must be int32");
    const int H = preds.size(0), C = preds.size(2);
    const long long N = preds.size(1);
    const int Hc = (int)std::min<int64_t>(hc, H);
    const int KH = (H + Hc - 1) / Hc;
    auto partial = torch::empty({KH, N},
                                preds.options().dtype(torch::kFloat32));
    const int bx = (int)((N + BLOCK - 1) / BLOCK);
    dispatch_storage(preds, kPiHatDtypes, [&](auto* p) {
        launch(pi_hat_delta_part_kernel<elem_t<decltype(p)>>, dim3(bx, KH),
               0, p, cls.data_ptr<int>(), partial.data_ptr<float>(),
               H, N, C, Hc);
    });
    return partial;
}


torch::Tensor pi_hat_delta_t_part(torch::Tensor preds_t,
                                  torch::Tensor cls, int64_t hc) {
    TORCH_CHECK(preds_t.is_cuda() && preds_t.is_contiguous(),
                "preds_t must be contiguous on a ROCm device");
    TORCH_CHECK(cls.scalar_type() == torch::kInt32, "cls must be int32");
    const int H = preds_t.size(0), C = preds_t.size(1);
    const long long N = preds_t.size(2);
    const int Hc = (int)std::min<int64_t>(hc, H);
    const int KH = (H + Hc - 1) / Hc;
    auto partial = torch::empty({KH, N},
                                preds_t.options()
                                .dtype(torch::kFloat32));
    const int bx = (int)((N + BLOCK - 1) / BLOCK);
    dispatch_storage(preds_t, kPiHatDtypes, [&](auto* p) {
        launch(pi_hat_delta_t_part_kernel<elem_t<decltype(p)>>,
               dim3(bx, KH), 0, p, cls.data_ptr<int>(),
               partial.data_ptr<float>(), H, N, C, Hc);
    });
    return partial;
}


void dirichlet_add(torch::Tensor dir, torch::Tensor y, torch::Tensor cls,
                   double lr) {
    check_f32_cuda(dir, "dirichlets");
    TORCH_CHECK(y.scalar_type() == torch::kInt64 && y.numel() == 1, "y");
    TORCH_CHECK(cls.scalar_type() == torch::kInt64, "cls");
    const int H = dir.size(0), C = dir.size(1);
    launch(dirichlet_add_kernel, dim3((H + BLOCK - 1) / BLOCK), 0,
           dir.data_ptr<float>(), y.data_ptr<long>(), cls.data_ptr<long>(),
           (float)lr, H, C);
}

void col_add(torch::Tensor adjusted, torch::Tensor row_sums,
             torch::Tensor y, torch::Tensor delta) {
    check_f32_cuda(adjusted, "adjusted");
    check_f32_cuda(row_sums, "row_sums");
    check_f32_cuda(delta, "delta");
    TORCH_CHECK(y.scalar_type() == torch::kInt64 && y.numel() == 1, "y");
    const long long N = adjusted.size(0);
    const int C = adjusted.size(1);
    launch(col_add_kernel, dim3((int)((N + BLOCK - 1) / BLOCK)), 0,
           adjusted.data_ptr<float>(), row_sums.data_ptr<float>(),
           y.data_ptr<long>(), delta.data_ptr<float>(), N, C);
}

std::vector<torch::Tensor> mixture_entropy(torch::Tensor rows,
                                           torch::Tensor pi) {
    check_f32_cuda(rows, "rows");
    check_f32_cuda(pi, "pi");
    const int C = rows.size(0), H = rows.size(1);
    TORCH_CHECK((H & 3) == 0 && H <= 4 * BLOCK,
                "mixture_entropy kernel needs H % 4 == 0, H <= 1024");
    TORCH_CHECK(pi.numel() == C);
    const int G = 64;
    auto partial = torch::empty({G, H}, rows.options());
    auto mixture0 = torch::empty({H}, rows.options());
    auto h0 = torch::empty({1}, rows.options());
    launch(mix_part_kernel, dim3(G), 0, rows.data_ptr<float>(),
           pi.data_ptr<float>(), partial.data_ptr<float>(), C, H);
    launch(mix_combine_kernel, dim3(1), 0, partial.data_ptr<float>(),
           mixture0.data_ptr<float>(), h0.data_ptr<float>(), G, H);
    return {mixture0, h0};
}

torch::Tensor pi_marginal(torch::Tensor adjusted, torch::Tensor row_sums) {
    check_f32_cuda(adjusted, "adjusted");
    check_f32_cuda(row_sums, "row_sums");
    const long long N = adjusted.size(0);
    const int C = adjusted.size(1);
    TORCH_CHECK(C <= 8 * BLOCK, "C too large for pi_marginal kernel");
    // Vector shapes take the float4 slab kernel (probe: 36 us vs 165 us
    // for the atomic single-kernel at N=50k, C=1000), G sized so the
    // partial stage keeps ~1024 ACTIVE waves streaming: a block covers
    // ceil(C/4) lanes = awpb active waves. Every other C: scalar slab
    // partials on columns padded to a multiple of 4, G = 1536 (6
    // blocks/CU: enough row-slabs in flight to cover HBM latency; 512 ran
    // at 1 TB/s). Both end in the same fixed-order two-stage reduce.
    const bool vec = (C & 3) == 0 && C <= 4 * BLOCK;
    const int Cpad = (C + 3) & ~3;
    const int awpb = (C / 4 + 63) / 64;
    const int G = vec ? std::min(1024, std::max(256, 1024 / awpb)) : 1536;
    constexpr int S = 16;  // G-reduce split
    auto out = torch::empty({Cpad}, adjusted.options());
    auto work = torch::empty({G + S, Cpad}, adjusted.options());
    float* partial = work.data_ptr<float>();
    float* part2 = partial + (long long)G * Cpad;
    const int cblocks = (Cpad + 4 * BLOCK - 1) / (4 * BLOCK);
    launch(vec ? pi_marginal_part_kernel : pi_marginal_kernel, dim3(G), 0,
           adjusted.data_ptr<float>(), row_sums.data_ptr<float>(), partial,
           N, C, Cpad);
    launch(pi_marginal_reduce_kernel, dim3(cblocks, S), 0, partial, part2,
           G, Cpad, Cpad, Cpad);
    launch(pi_marginal_reduce_kernel, dim3(cblocks, 1), 0, part2,
           out.data_ptr<float>(), S, Cpad, Cpad, Cpad);
    return out.narrow(0, 0, C);
}

void register_label_ops(pybind11::module_& m) {
    m.def("pi_hat_delta", &pi_hat_delta,
          "rank-1 pi_hat increment: sum_h preds[h, :, cls_h]");
    m.def("pi_hat_delta_part", &pi_hat_delta_part,
          "H-chunked rank-1 pi_hat increment partials (KH, N)");
    m.def("pi_hat_delta_t_part", &pi_hat_delta_t_part,
          "class-major (H, C, N) rank-1 pi_hat gather partials");
    m.def("col_add", &col_add,
          "fused adjusted[:, y] += delta; row_sums += delta");
    m.def("dirichlet_add", &dirichlet_add,
          "dir[h, y, cls_h] += lr scatter (the posterior label update)");
    m.def("mixture_entropy", &mixture_entropy,
          "mixture0 (H,) = sum_c pi[c]*rows[c,h] + fused log2 entropy");
    m.def("pi_marginal", &pi_marginal,
          "pi[c] = sum_n adjusted[n,c]/clamp(rowsum[n]) in one pass");
}
