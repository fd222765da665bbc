// Fused CDNA4 (gfx950) kernels for the CODA hot path.
//
// The acquisition hot loop (reference: coda/coda.py:77-119 + :235-281) is,
// per candidate row, a Beta-grid P(best) integral coupled over the model
// axis H:
//   p_h = integral pdf_h(x) * prod_{h'!=h} cdf_{h'}(x) dx  on a P=256 grid,
// followed by a log2-entropy EIG assembly. The reference materializes six
// (R, H, P) fp32 tensors per chunk and runs a SEQUENTIAL Python loop over P
// for the trapezoid CDF.
//
// Kernel shape (wave-per-row): one 64-lane wave owns one row; each lane
// owns 4 consecutive grid points (P = 256 = 64 x 4). The trapezoid CDF is
// a lane-local running sum + one wave shfl-scan - NO block barriers and no
// LDS traffic in the hot loop (the first design used thread<->point with a
// 3-barrier LDS scan per model per pass; this one is barrier-free after
// staging). The H-coupling (sum_h log cdf) lives in 4 per-lane registers;
// the EIG entropy epilogue is fused into the hypothetical-update kernel.
// Global traffic: 2*R*H floats in, R*H (or B*C) floats out - three orders
// of magnitude below the eager formulation.
//
// Numerics: log-pdf evaluated in f64 (2 FMA per point; f32 cancellation at
// large Beta counts is the reference's main error source there), exp/log
// in f32, the reference's clamp ladder preserved exactly (cdf clamp 1e-30,
// log-space clamp +-80, entropy clamp 1e-12).
//
// Workgroup = 256 threads = 4 waves = 4 independent rows.
//
// This file holds the v1 engine; the v2 table engine is table.hip, the
// per-label posterior update label.hip. The grid geometry and per-lane
// grid state shared with table.hip are beta_grid.h, the cross-lane
// primitives wave.h.
//
// Kernel inventory (host bindings at the bottom):
//   pbest_kernel           fused P(best) over (R, H) rows
//   pbest_row_kernel       one row, the model axis windowed over the
//                          workgroup's 4 waves
//   eig_hyp_kernel         fused hypothetical P(best) + entropy (v1 EIG)
//   pbest/eig_phase1/2     two-phase variants with the model-axis
//                          all-reduce seam between passes (sharded v1)
//   pbest_phase1/2_wide    wide-H (> 2048 models): the two-pass split with
//                          LDS column windows as the "ranks", coupled
//                          through global memory on one device

#include "host_util.h"
#include <algorithm>
#include <vector>

namespace {

// Per-row P(best) core. The wave loops over models h twice:
//   pass A accumulates the cdf product PI_h cdf_h(p_j) per lane point as a
//   (mantissa, exponent) pair - one multiply + a native v_frexp per model
//   instead of a log (base-2 log taken ONCE at the end);
//   pass B integrates pdf_h * exp2(clamp(slog2 - log2 cdf_h)) and leaves
//   the UNNORMALIZED per-model masses in s_pb[0..H).
// All transcendentals are the native base-2 ops (v_exp_f32/v_log_f32);
// log-pdf arguments are prepared in f64 as base-2 logs (s_lnB holds
// log2 B(a,b)). Returns 1/sum_h mass. s_a/s_b/s_lnB/s_pb are this row's
// staged LDS arrays.

// Pass A: slog2[j] = log2 PROD_h clamp(cdf_h(p_j), 1e-30), accumulated as
// a (mantissa, exponent) pair - one multiply + native v_frexp per model
// instead of a per-model v_log (base-2 log taken once at the end).
__device__ void pbest_pass_a(const float* s_a, const float* s_b,
                             const double* s_lnB, int H,
                             const LaneGrid& g, int lane,
                             float (&slog2)[PTS_PER_LANE]) {
    float pm[PTS_PER_LANE] = {1.f, 1.f, 1.f, 1.f};
    int pe_[PTS_PER_LANE] = {0, 0, 0, 0};
    for (int h = 0; h < H; ++h) {
        float pdf[PTS_PER_LANE], cdf[PTS_PER_LANE];
        g.pdf4(s_a[h], s_b[h], s_lnB[h], pdf);
        g.cdf4(pdf, lane, cdf);
        // renormalize every model: one clamped factor can be 1e-30, so a
        // second multiply would underflow f32.
#pragma unroll
        for (int j = 0; j < PTS_PER_LANE; ++j) {
            int ex;
            pm[j] = frexpf(pm[j] * fmaxf(cdf[j], kEps), &ex);
            pe_[j] += ex;
        }
    }
#pragma unroll
    for (int j = 0; j < PTS_PER_LANE; ++j)
        slog2[j] = __log2f(pm[j]) + (float)pe_[j];
}

// Pass B: unnormalized per-model masses
//   pb_h = trapz pdf_h * exp2(clamp(slog2 - log2 cdf_h, +-115.4))
// left in s_pb[0..H); returns the wave-local sum over H (the normalizer
// partial - globally reduced by the caller when H is sharded).
__device__ float pbest_pass_b(const float* s_a, const float* s_b,
                              const double* s_lnB, float* s_pb, int H,
                              const LaneGrid& g, int lane,
                              const float (&slog2)[PTS_PER_LANE]) {
    float w[PTS_PER_LANE] = {1.f, 1.f, 1.f, 1.f};
    if (lane == 0) w[0] = 0.5f;                 // trapz endpoint p == 0
    if (lane == 63) w[PTS_PER_LANE - 1] = 0.5f;  // and p == P-1
    for (int h = 0; h < H; ++h) {
        float pdf[PTS_PER_LANE], cdf[PTS_PER_LANE];
        g.pdf4(s_a[h], s_b[h], s_lnB[h], pdf);
        g.cdf4(pdf, lane, cdf);
        float acc = 0.f;
#pragma unroll
        for (int j = 0; j < PTS_PER_LANE; ++j) {
            float lc = __log2f(fmaxf(cdf[j], kEps));
            float pe = exp2f(
                fminf(fmaxf(slog2[j] - lc, -kLog2Clamp), kLog2Clamp));
            acc += pdf[j] * pe * w[j];
        }
        float mass = wave_reduce_sum(acc * g.dxf);
        if (lane == (h & 63)) s_pb[h] = mass;
    }
    // all lanes of the wave executed the stores above in program order;
    // wave-internal LDS visibility needs no barrier.
    float part = 0.f;
    for (int h = lane; h < H; h += 64) part += s_pb[h];
    return wave_reduce_sum(part);
}

// Fused single-device core: both passes; returns 1/total.
__device__ float pbest_row_core(const float* s_a, const float* s_b,
                                const double* s_lnB, float* s_pb, int H) {
    const int lane = threadIdx.x & 63;
    LaneGrid g;
    g.init(lane);
    float slog2[PTS_PER_LANE];
    pbest_pass_a(s_a, s_b, s_lnB, H, g, lane, slog2);
    float total = pbest_pass_b(s_a, s_b, s_lnB, s_pb, H, g, lane, slog2);
    return 1.0f / fmaxf(total, kEps);
}

// Cooperative LDS staging of up to ROWS_PER_BLOCK rows of Beta params
// (+ the f64 log2-Beta-normalizer, computed once per (row, model)).
__device__ void stage_plain(const float* alpha, const float* beta, int R,
                            int H, int row0, double* lnB_all, float* f_all) {
    for (int idx = threadIdx.x; idx < ROWS_PER_BLOCK * H; idx += BLOCK) {
        const int rl = idx / H, h = idx - rl * H;
        const int r = row0 + rl;
        if (r >= R) continue;
        float a = alpha[(size_t)r * H + h];
        float b = beta[(size_t)r * H + h];
        f_all[rl * 3 * H + h] = a;
        f_all[rl * 3 * H + H + h] = b;
        lnB_all[rl * H + h] = (lgamma((double)a) + lgamma((double)b)
                            - lgamma((double)a + (double)b))
                            * 1.4426950408889634;
    }
    __syncthreads();
}

// Staging with the hypothetical update applied on the fly:
// row r = (candidate b, hypothesized class c); model h gets alpha+w if its
// argmax class on b equals c, else beta+w (reference coda/coda.py:150-168).
__device__ void stage_hyp(const float* alpha_t, const float* beta_t,
                          const int* cls, float update_weight, int B, int C,
                          int H, int row0, double* lnB_all, float* f_all) {
    const int R = B * C;
    for (int idx = threadIdx.x; idx < ROWS_PER_BLOCK * H; idx += BLOCK) {
        const int rl = idx / H, h = idx - rl * H;
        const int r = row0 + rl;
        if (r >= R) continue;
        const int b = r / C, c = r - b * C;
        const int cl = cls[(size_t)b * H + h];
        const float add = (cl == c) ? update_weight : 0.f;
        float a = alpha_t[(size_t)c * H + h] + add;
        float bb = beta_t[(size_t)c * H + h] + (update_weight - add);
        f_all[rl * 3 * H + h] = a;
        f_all[rl * 3 * H + H + h] = bb;
        lnB_all[rl * H + h] = (lgamma((double)a) + lgamma((double)bb)
                            - lgamma((double)a + (double)bb))
                            * 1.4426950408889634;
    }
    __syncthreads();
}

// ---------------------------------------------------------------------------
// Kernel 1: generic P(best). alpha/beta: (R, H) -> out: (R, H).
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(BLOCK, 4)
pbest_kernel(const float* __restrict__ alpha, const float* __restrict__ beta,
             float* __restrict__ out, int R, int H) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    double* lnB_all = reinterpret_cast<double*>(smem_raw);
    float* f_all = reinterpret_cast<float*>(lnB_all + ROWS_PER_BLOCK * H);

    const int tid = threadIdx.x;
    const int row0 = blockIdx.x * ROWS_PER_BLOCK;
    stage_plain(alpha, beta, R, H, row0, lnB_all, f_all);

    const int rl = tid >> 6;
    const int r = row0 + rl;
    if (r >= R) return;
    float* s_a = f_all + rl * 3 * H;
    float* s_b = s_a + H;
    float* s_pb = s_b + H;
    double* s_lnB = lnB_all + rl * H;

    float inv = pbest_row_core(s_a, s_b, s_lnB, s_pb, H);

    const int lane = tid & 63;
    for (int h = lane; h < H; h += 64)
        out[(size_t)r * H + h] = s_pb[h] * inv;
}

// Single-row P(best): R = 1 gives the generic kernel ONE wave (one
// workgroup, 92 us at H=128 - the per-label incremental posterior-row
// refresh is exactly this shape).  Here all ROWS_PER_BLOCK waves
// cooperate on the one row by windowing the model axis: wave w owns
// models [w*Hc, w*Hc+Hc), pass-A slog2 partials combine through LDS
// (the in-workgroup analogue of the phase1/phase2 global coupling),
// pass B integrates each window against the combined term.  Identical
// math to the two-pass split, one launch.
__global__ void __launch_bounds__(BLOCK, 4)
pbest_row_kernel(const float* __restrict__ alpha,  // (H,)
                 const float* __restrict__ beta,   // (H,)
                 float* __restrict__ out,          // (H,)
                 int H) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    const int Hc = (H + ROWS_PER_BLOCK - 1) / ROWS_PER_BLOCK;
    double* lnB_all = reinterpret_cast<double*>(smem_raw);
    float* f_all = reinterpret_cast<float*>(lnB_all + ROWS_PER_BLOCK * Hc);
    float* slds = f_all + ROWS_PER_BLOCK * 3 * Hc;     // (4, P) partials
    float* tot_lds = slds + ROWS_PER_BLOCK * P_POINTS; // (4,)

    for (int idx = threadIdx.x; idx < ROWS_PER_BLOCK * Hc; idx += BLOCK) {
        const int w = idx / Hc, h = idx - w * Hc;
        const int hg = w * Hc + h;
        if (hg >= H) continue;
        float a = alpha[hg], b = beta[hg];
        f_all[w * 3 * Hc + h] = a;
        f_all[w * 3 * Hc + Hc + h] = b;
        lnB_all[w * Hc + h] = (lgamma((double)a) + lgamma((double)b)
                            - lgamma((double)a + (double)b))
                            * 1.4426950408889634;
    }
    __syncthreads();

    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int Hcur = max(0, min(Hc, H - w * Hc));
    LaneGrid g;
    g.init(lane);
    float slog2[PTS_PER_LANE];
    // empty window: pass A leaves the identity (log2 1 = 0) partial
    pbest_pass_a(f_all + w * 3 * Hc, f_all + w * 3 * Hc + Hc,
                 lnB_all + w * Hc, Hcur, g, lane, slog2);
#pragma unroll
    for (int j = 0; j < PTS_PER_LANE; ++j)
        slds[w * P_POINTS + lane * PTS_PER_LANE + j] = slog2[j];
    __syncthreads();
#pragma unroll
    for (int j = 0; j < PTS_PER_LANE; ++j) {
        float s = 0.f;
        for (int q = 0; q < ROWS_PER_BLOCK; ++q)
            s += slds[q * P_POINTS + lane * PTS_PER_LANE + j];
        slog2[j] = s;
    }
    float* s_pb = f_all + w * 3 * Hc + 2 * Hc;
    const float part = pbest_pass_b(f_all + w * 3 * Hc,
                                    f_all + w * 3 * Hc + Hc,
                                    lnB_all + w * Hc, s_pb,
                                    Hcur, g, lane, slog2);
    if (lane == 0) tot_lds[w] = part;
    __syncthreads();
    const float total = tot_lds[0] + tot_lds[1] + tot_lds[2] + tot_lds[3];
    const float inv = 1.0f / fmaxf(total, kEps);
    for (int h = lane; h < Hcur; h += 64)
        out[w * Hc + h] = s_pb[h] * inv;
}

// ---------------------------------------------------------------------------
// Kernel 2: fused hypothetical-update P(best) + entropy epilogue for EIG.
// One wave per (candidate b, hypothesized class c) row:
//   a_h = alpha_t[c,h] + w*[cls[b,h]==c];  b_h = beta_t[c,h] + w*[else]
//   pb = pbest(a, b)  (normalized over H)
//   H_after[b,c] = -sum_h m log2 m,  m = clamp(mixture0[h]
//                  + pi_hat[c]*(pb_h - pbest_before[c,h]), 1e-12)
// (reference: coda/coda.py:150-168 + :267-276). The final EIG contraction
// over (B, C) is done by the host.
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(BLOCK, 4)
eig_hyp_kernel(const float* __restrict__ alpha_t,       // (C, H)
               const float* __restrict__ beta_t,        // (C, H)
               const int* __restrict__ cls,             // (B, H)
               const float* __restrict__ pbest_before,  // (C, H)
               const float* __restrict__ pi_hat,        // (C,)
               const float* __restrict__ mixture0,      // (H,)
               float* __restrict__ h_after,             // (B, C)
               float update_weight, int B, int C, int H) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    double* lnB_all = reinterpret_cast<double*>(smem_raw);
    float* f_all = reinterpret_cast<float*>(lnB_all + ROWS_PER_BLOCK * H);

    const int tid = threadIdx.x;
    const int row0 = blockIdx.x * ROWS_PER_BLOCK;
    const int R = B * C;
    stage_hyp(alpha_t, beta_t, cls, update_weight, B, C, H, row0,
              lnB_all, f_all);

    const int rl = tid >> 6;
    const int r = row0 + rl;
    if (r >= R) return;
    const int b = r / C, c = r - b * C;
    float* s_a = f_all + rl * 3 * H;
    float* s_b = s_a + H;
    float* s_pb = s_b + H;
    double* s_lnB = lnB_all + rl * H;

    float inv = pbest_row_core(s_a, s_b, s_lnB, s_pb, H);

    const int lane = tid & 63;
    const float pi_c = pi_hat[c];
    float ent = 0.f;
    for (int h = lane; h < H; h += 64) {
        float pb = s_pb[h] * inv;
        float m = mixture0[h] + pi_c * (pb - pbest_before[(size_t)c * H + h]);
        m = fmaxf(m, 1e-12f);
        ent += -m * __log2f(m);
    }
    float ent_total = wave_reduce_sum(ent);
    if (lane == 0) h_after[r] = ent_total;
}


// ---------------------------------------------------------------------------
// Two-phase (model-axis-sharded) kernels. When H shards across ranks, the
// coupling term sum_h log2 cdf_h(p) is all-reduced between pass A and
// pass B (SURVEY.md section 2.4 - the latency-critical collective of the
// EIG loop). Phase 1 writes each row's slog2 partial (R, P) coalesced
// (lane l owns points 4l..4l+3); after the all-reduce, phase 2 reads the
// GLOBAL slog2, integrates, and emits UNNORMALIZED per-model masses plus
// the local normalizer partial (second, tiny all-reduce done by the host).
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(BLOCK, 4)
pbest_phase1_kernel(const float* __restrict__ alpha,
                    const float* __restrict__ beta,
                    float* __restrict__ slog2_out,  // (R, P)
                    int R, int H) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    double* lnB_all = reinterpret_cast<double*>(smem_raw);
    float* f_all = reinterpret_cast<float*>(lnB_all + ROWS_PER_BLOCK * H);
    const int row0 = blockIdx.x * ROWS_PER_BLOCK;
    stage_plain(alpha, beta, R, H, row0, lnB_all, f_all);
    const int rl = threadIdx.x >> 6;
    const int r = row0 + rl;
    if (r >= R) return;
    const int lane = threadIdx.x & 63;
    LaneGrid g;
    g.init(lane);
    float slog2[PTS_PER_LANE];
    pbest_pass_a(f_all + rl * 3 * H, f_all + rl * 3 * H + H,
                 lnB_all + rl * H, H, g, lane, slog2);
#pragma unroll
    for (int j = 0; j < PTS_PER_LANE; ++j)
        slog2_out[(size_t)r * P_POINTS + lane * PTS_PER_LANE + j] = slog2[j];
}

__global__ void __launch_bounds__(BLOCK, 4)
pbest_phase2_kernel(const float* __restrict__ alpha,
                    const float* __restrict__ beta,
                    const float* __restrict__ slog2_in,  // (R, P) global
                    float* __restrict__ pb_out,          // (R, H) unnorm
                    float* __restrict__ tot_out,         // (R,) partial
                    int R, int H) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    double* lnB_all = reinterpret_cast<double*>(smem_raw);
    float* f_all = reinterpret_cast<float*>(lnB_all + ROWS_PER_BLOCK * H);
    const int row0 = blockIdx.x * ROWS_PER_BLOCK;
    stage_plain(alpha, beta, R, H, row0, lnB_all, f_all);
    const int rl = threadIdx.x >> 6;
    const int r = row0 + rl;
    if (r >= R) return;
    const int lane = threadIdx.x & 63;
    LaneGrid g;
    g.init(lane);
    float slog2[PTS_PER_LANE];
#pragma unroll
    for (int j = 0; j < PTS_PER_LANE; ++j)
        slog2[j] = slog2_in[(size_t)r * P_POINTS + lane * PTS_PER_LANE + j];
    float* s_pb = f_all + rl * 3 * H + 2 * H;
    float total = pbest_pass_b(f_all + rl * 3 * H, f_all + rl * 3 * H + H,
                               lnB_all + rl * H, s_pb, H, g, lane, slog2);
    for (int h = lane; h < H; h += 64)
        pb_out[(size_t)r * H + h] = s_pb[h];
    if (lane == 0) tot_out[r] = total;
}

// ---------------------------------------------------------------------------
// Wide-H single-device variants: the same two-pass split, but the "shards"
// are LDS-sized column windows of one (R, Htot) matrix processed by
// blockIdx.y, coupled through global memory instead of RCCL. Lifts the
// H <= 2048 LDS ceiling of the fused kernel (model pools of 10k+) while
// keeping every pass in LDS and the whole op at two launches + two tiny
// sums (vs the chunked eager fallback's ~1 GB log-cdf intermediates).
// ---------------------------------------------------------------------------
__device__ void stage_window(const float* alpha, const float* beta, int R,
                             int Htot, int h0, int Hc, int row0,
                             double* lnB_all, float* f_all) {
    for (int idx = threadIdx.x; idx < ROWS_PER_BLOCK * Hc; idx += BLOCK) {
        const int rl = idx / Hc, h = idx - rl * Hc;
        const int r = row0 + rl;
        if (r >= R || h0 + h >= Htot) continue;
        float a = alpha[(size_t)r * Htot + h0 + h];
        float b = beta[(size_t)r * Htot + h0 + h];
        f_all[rl * 3 * Hc + h] = a;
        f_all[rl * 3 * Hc + Hc + h] = b;
        lnB_all[rl * Hc + h] = (lgamma((double)a) + lgamma((double)b)
                             - lgamma((double)a + (double)b))
                             * 1.4426950408889634;
    }
    __syncthreads();
}

__global__ void __launch_bounds__(BLOCK, 4)
pbest_phase1_wide_kernel(const float* __restrict__ alpha,
                         const float* __restrict__ beta,
                         float* __restrict__ slog2_part,  // (KH, R, P)
                         int R, int Htot, int Hc) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    double* lnB_all = reinterpret_cast<double*>(smem_raw);
    float* f_all = reinterpret_cast<float*>(lnB_all + ROWS_PER_BLOCK * Hc);
    const int k = blockIdx.y, h0 = k * Hc;
    const int Hcur = min(Hc, Htot - h0);
    const int row0 = blockIdx.x * ROWS_PER_BLOCK;
    stage_window(alpha, beta, R, Htot, h0, Hc, row0, lnB_all, f_all);
    const int rl = threadIdx.x >> 6;
    const int r = row0 + rl;
    if (r >= R) return;
    const int lane = threadIdx.x & 63;
    LaneGrid g;
    g.init(lane);
    float slog2[PTS_PER_LANE];
    // stage_window packs the window at stride Hc, so pass A sees a dense
    // Hcur-model row exactly like a shard's local slice
    pbest_pass_a(f_all + rl * 3 * Hc, f_all + rl * 3 * Hc + Hc,
                 lnB_all + rl * Hc, Hcur, g, lane, slog2);
#pragma unroll
    for (int j = 0; j < PTS_PER_LANE; ++j)
        slog2_part[((size_t)k * R + r) * P_POINTS
                   + lane * PTS_PER_LANE + j] = slog2[j];
}

__global__ void __launch_bounds__(BLOCK, 4)
pbest_phase2_wide_kernel(const float* __restrict__ alpha,
                         const float* __restrict__ beta,
                         const float* __restrict__ slog2_in,  // (R, P) global
                         float* __restrict__ pb_out,          // (R, Htot)
                         float* __restrict__ tot_part,        // (KH, R)
                         int R, int Htot, int Hc) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    double* lnB_all = reinterpret_cast<double*>(smem_raw);
    float* f_all = reinterpret_cast<float*>(lnB_all + ROWS_PER_BLOCK * Hc);
    const int k = blockIdx.y, h0 = k * Hc;
    const int Hcur = min(Hc, Htot - h0);
    const int row0 = blockIdx.x * ROWS_PER_BLOCK;
    stage_window(alpha, beta, R, Htot, h0, Hc, row0, lnB_all, f_all);
    const int rl = threadIdx.x >> 6;
    const int r = row0 + rl;
    if (r >= R) return;
    const int lane = threadIdx.x & 63;
    LaneGrid g;
    g.init(lane);
    float slog2[PTS_PER_LANE];
#pragma unroll
    for (int j = 0; j < PTS_PER_LANE; ++j)
        slog2[j] = slog2_in[(size_t)r * P_POINTS + lane * PTS_PER_LANE + j];
    float* s_pb = f_all + rl * 3 * Hc + 2 * Hc;
    float total = pbest_pass_b(f_all + rl * 3 * Hc, f_all + rl * 3 * Hc + Hc,
                               lnB_all + rl * Hc, s_pb, Hcur, g, lane, slog2);
    for (int h = lane; h < Hcur; h += 64)
        pb_out[(size_t)r * Htot + h0 + h] = s_pb[h];
    if (lane == 0) tot_part[(size_t)k * R + r] = total;
}

__global__ void __launch_bounds__(BLOCK, 4)
eig_phase1_kernel(const float* __restrict__ alpha_t,
                  const float* __restrict__ beta_t,
                  const int* __restrict__ cls,
                  float* __restrict__ slog2_out,  // (B*C, P)
                  float update_weight, int B, int C, int H) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    double* lnB_all = reinterpret_cast<double*>(smem_raw);
    float* f_all = reinterpret_cast<float*>(lnB_all + ROWS_PER_BLOCK * H);
    const int row0 = blockIdx.x * ROWS_PER_BLOCK;
    stage_hyp(alpha_t, beta_t, cls, update_weight, B, C, H, row0,
              lnB_all, f_all);
    const int rl = threadIdx.x >> 6;
    const int r = row0 + rl;
    if (r >= B * C) return;
    const int lane = threadIdx.x & 63;
    LaneGrid g;
    g.init(lane);
    float slog2[PTS_PER_LANE];
    pbest_pass_a(f_all + rl * 3 * H, f_all + rl * 3 * H + H,
                 lnB_all + rl * H, H, g, lane, slog2);
#pragma unroll
    for (int j = 0; j < PTS_PER_LANE; ++j)
        slog2_out[(size_t)r * P_POINTS + lane * PTS_PER_LANE + j] = slog2[j];
}

__global__ void __launch_bounds__(BLOCK, 4)
eig_phase2_kernel(const float* __restrict__ alpha_t,
                  const float* __restrict__ beta_t,
                  const int* __restrict__ cls,
                  const float* __restrict__ slog2_in,  // (B*C, P) global
                  float* __restrict__ pb_out,          // (B*C, H) unnorm
                  float* __restrict__ tot_out,         // (B*C,) partial
                  float update_weight, int B, int C, int H) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    double* lnB_all = reinterpret_cast<double*>(smem_raw);
    float* f_all = reinterpret_cast<float*>(lnB_all + ROWS_PER_BLOCK * H);
    const int row0 = blockIdx.x * ROWS_PER_BLOCK;
    stage_hyp(alpha_t, beta_t, cls, update_weight, B, C, H, row0,
              lnB_all, f_all);
    const int rl = threadIdx.x >> 6;
    const int r = row0 + rl;
    if (r >= B * C) return;
    const int lane = threadIdx.x & 63;
    LaneGrid g;
    g.init(lane);
    float slog2[PTS_PER_LANE];
#pragma unroll
    for (int j = 0; j < PTS_PER_LANE; ++j)
        slog2[j] = slog2_in[(size_t)r * P_POINTS + lane * PTS_PER_LANE + j];
    float* s_pb = f_all + rl * 3 * H + 2 * H;
    float total = pbest_pass_b(f_all + rl * 3 * H, f_all + rl * 3 * H + H,
                               lnB_all + rl * H, s_pb, H, g, lane, slog2);
    for (int h = lane; h < H; h += 64)
        pb_out[(size_t)r * H + h] = s_pb[h];
    if (lane == 0) tot_out[r] = total;
}

}  // namespace

// ---------------------------------------------------------------------------
// Host bindings
// ---------------------------------------------------------------------------

torch::Tensor pbest_from_beta(torch::Tensor alpha, torch::Tensor beta,
                              int64_t num_points) {
    check_f32_cuda(alpha, "alpha");
    check_f32_cuda(beta, "beta");
    TORCH_CHECK(num_points == P_POINTS,
                "HIP pbest kernel is compiled for P=256");
    TORCH_CHECK(alpha.dim() == 2 && alpha.sizes() == beta.sizes(),
                "alpha/beta must be (R, H)");
    const int R = alpha.size(0), H = alpha.size(1);
    auto out = torch::empty_like(alpha);
    if (R == 0) return out;
    if (R == 1) {
        // one row would give the generic kernel a single wave; the row
        // kernel windows the model axis across the whole workgroup
        const int Hc = (H + ROWS_PER_BLOCK - 1) / ROWS_PER_BLOCK;
        const size_t smem = lds_bytes(Hc)
            + (ROWS_PER_BLOCK * P_POINTS + ROWS_PER_BLOCK) * sizeof(float);
        TORCH_CHECK(smem <= 160 * 1024, "H too large for LDS: ", H);
        launch(pbest_row_kernel, dim3(1), smem, alpha.data_ptr<float>(),
               beta.data_ptr<float>(), out.data_ptr<float>(), H);
        return out;
    }
    const auto g = v1_geometry(R, H);
    launch(pbest_kernel, dim3(g.blocks), g.smem, alpha.data_ptr<float>(),
           beta.data_ptr<float>(), out.data_ptr<float>(), R, H);
    return out;
}

torch::Tensor eig_chunk(torch::Tensor alpha_cc, torch::Tensor beta_cc,
                        torch::Tensor chunk_classes,
                        torch::Tensor pbest_before, torch::Tensor pi_hat,
                        torch::Tensor pi_hat_xi, torch::Tensor mixture0,
                        double h_before, double update_weight,
                        int64_t num_points) {
    check_f32_cuda(pbest_before, "pbest_before");
    check_f32_cuda(pi_hat, "pi_hat");
    check_f32_cuda(pi_hat_xi, "pi_hat_xi");
    check_f32_cuda(mixture0, "mixture0");
    check_hyp_inputs(alpha_cc, beta_cc, chunk_classes);
    TORCH_CHECK(num_points == P_POINTS,
                "HIP eig kernel is compiled for P=256");
    const int H = alpha_cc.size(0), C = alpha_cc.size(1);
    const int B = chunk_classes.size(0);
    TORCH_CHECK(pbest_before.dim() == 2 && pbest_before.size(0) == C &&
                pbest_before.size(1) == H, "pbest_before must be (C, H)");
    TORCH_CHECK(pi_hat.numel() == C, "pi_hat must be (C,)");
    TORCH_CHECK(mixture0.numel() == H, "mixture0 must be (H,)");
    TORCH_CHECK(pi_hat_xi.dim() == 2 && pi_hat_xi.size(0) == B &&
                pi_hat_xi.size(1) == C, "pi_hat_xi must be (B, C)");
    // (H, C) -> (C, H) contiguous rows for per-class streaming
    auto alpha_t = alpha_cc.t().contiguous();
    auto beta_t = beta_cc.t().contiguous();
    check_f32_cuda(alpha_t, "alpha_cc");
    check_f32_cuda(beta_t, "beta_cc");

    auto h_after = torch::empty({B, C}, alpha_t.options());
    const auto g = v1_geometry(B * C, H);
    launch(eig_hyp_kernel, dim3(g.blocks), g.smem,
           alpha_t.data_ptr<float>(), beta_t.data_ptr<float>(),
           chunk_classes.data_ptr<int>(), pbest_before.data_ptr<float>(),
           pi_hat.data_ptr<float>(), mixture0.data_ptr<float>(),
           h_after.data_ptr<float>(), (float)update_weight, B, C, H);
    // EIG = H_before - sum_c pi_hat_xi[b,c] * H_after[b,c]
    return h_before - (pi_hat_xi * h_after).sum(-1);
}


// ---- Two-phase (sharded) host bindings ----

torch::Tensor pbest_phase1(torch::Tensor alpha, torch::Tensor beta) {
    check_beta_rows(alpha, beta);
    const int R = alpha.size(0), H = alpha.size(1);
    auto slog2 = torch::empty({R, P_POINTS}, alpha.options());
    if (R == 0) return slog2;
    const auto g = v1_geometry(R, H);
    launch(pbest_phase1_kernel, dim3(g.blocks), g.smem,
           alpha.data_ptr<float>(), beta.data_ptr<float>(),
           slog2.data_ptr<float>(), R, H);
    return slog2;
}

std::vector<torch::Tensor> pbest_phase2(torch::Tensor alpha,
                                        torch::Tensor beta,
                                        torch::Tensor slog2) {
    check_beta_rows(alpha, beta);
    check_slog2(slog2, alpha.size(0));
    const int R = alpha.size(0), H = alpha.size(1);
    auto pb = torch::empty({R, H}, alpha.options());
    auto tot = torch::empty({R}, alpha.options());
    if (R == 0) return {pb, tot};
    const auto g = v1_geometry(R, H);
    launch(pbest_phase2_kernel, dim3(g.blocks), g.smem,
           alpha.data_ptr<float>(), beta.data_ptr<float>(),
           slog2.data_ptr<float>(), pb.data_ptr<float>(),
           tot.data_ptr<float>(), R, H);
    return {pb, tot};
}

torch::Tensor pbest_phase1_wide(torch::Tensor alpha, torch::Tensor beta,
                                int64_t hc) {
    check_beta_rows(alpha, beta);
    TORCH_CHECK(hc >= 1, "hc must be >= 1");
    const int R = alpha.size(0), Htot = alpha.size(1);
    const int Hc = std::min<int64_t>(hc, Htot);
    const int KH = (Htot + Hc - 1) / Hc;
    auto part = torch::empty({KH, R, P_POINTS}, alpha.options());
    if (R == 0) return part;
    const auto g = v1_geometry(R, Hc, "Hc");
    launch(pbest_phase1_wide_kernel, dim3(g.blocks, KH), g.smem,
           alpha.data_ptr<float>(), beta.data_ptr<float>(),
           part.data_ptr<float>(), R, Htot, Hc);
    return part;
}

std::vector<torch::Tensor> pbest_phase2_wide(torch::Tensor alpha,
                                             torch::Tensor beta,
                                             torch::Tensor slog2,
                                             int64_t hc) {
    check_beta_rows(alpha, beta);
    check_slog2(slog2, alpha.size(0));
    TORCH_CHECK(hc >= 1, "hc must be >= 1");
    const int R = alpha.size(0), Htot = alpha.size(1);
    const int Hc = std::min<int64_t>(hc, Htot);
    const int KH = (Htot + Hc - 1) / Hc;
    auto pb = torch::empty({R, Htot}, alpha.options());
    auto tot_part = torch::empty({KH, R}, alpha.options());
    if (R == 0) return {pb, tot_part};
    const auto g = v1_geometry(R, Hc, "Hc");
    launch(pbest_phase2_wide_kernel, dim3(g.blocks, KH), g.smem,
           alpha.data_ptr<float>(), beta.data_ptr<float>(),
           slog2.data_ptr<float>(), pb.data_ptr<float>(),
           tot_part.data_ptr<float>(), R, Htot, Hc);
    return {pb, tot_part};
}

torch::Tensor eig_phase1(torch::Tensor alpha_cc, torch::Tensor beta_cc,
                         torch::Tensor chunk_classes, double update_weight) {
    check_hyp_inputs(alpha_cc, beta_cc, chunk_classes);
    const int H = alpha_cc.size(0), C = alpha_cc.size(1);
    const int B = chunk_classes.size(0);
    auto alpha_t = alpha_cc.t().contiguous();
    auto beta_t = beta_cc.t().contiguous();
    auto slog2 = torch::empty({(int64_t)B * C, P_POINTS}, alpha_t.options());
    const auto g = v1_geometry(B * C, H);
    launch(eig_phase1_kernel, dim3(g.blocks), g.smem,
           alpha_t.data_ptr<float>(), beta_t.data_ptr<float>(),
           chunk_classes.data_ptr<int>(), slog2.data_ptr<float>(),
           (float)update_weight, B, C, H);
    return slog2;
}

std::vector<torch::Tensor> eig_phase2(torch::Tensor alpha_cc,
                                      torch::Tensor beta_cc,
                                      torch::Tensor chunk_classes,
                                      torch::Tensor slog2,
                                      double update_weight) {
    check_hyp_inputs(alpha_cc, beta_cc, chunk_classes);
    const int H = alpha_cc.size(0), C = alpha_cc.size(1);
    const int B = chunk_classes.size(0);
    check_slog2(slog2, (int64_t)B * C);
    auto alpha_t = alpha_cc.t().contiguous();
    auto beta_t = beta_cc.t().contiguous();
    auto pb = torch::empty({(int64_t)B * C, H}, alpha_t.options());
    auto tot = torch::empty({(int64_t)B * C}, alpha_t.options());
    const auto g = v1_geometry(B * C, H);
    launch(eig_phase2_kernel, dim3(g.blocks), g.smem,
           alpha_t.data_ptr<float>(), beta_t.data_ptr<float>(),
           chunk_classes.data_ptr<int>(), slog2.data_ptr<float>(),
           pb.data_ptr<float>(), tot.data_ptr<float>(),
           (float)update_weight, B, C, H);
    return {pb, tot};
}

void register_pbest_ops(pybind11::module_& m) {
    m.def("pbest_from_beta", &pbest_from_beta,
          "Beta-grid P(best) per row: (R,H),(R,H) -> (R,H)");
    m.def("eig_chunk", &eig_chunk,
          "Fused hypothetical P(best) + entropy EIG for a candidate chunk");
    m.def("pbest_phase1", &pbest_phase1,
          "Sharded pass A: local sum_h log2 cdf partials (R, P)");
    m.def("pbest_phase2", &pbest_phase2,
          "Sharded pass B: unnormalized masses + normalizer partial");
    m.def("pbest_phase1_wide", &pbest_phase1_wide,
          "Wide-H pass A: per-window slog2 partials (KH, R, P)");
    m.def("pbest_phase2_wide", &pbest_phase2_wide,
          "Wide-H pass B: unnormalized (R, Htot) masses + (KH, R) totals");
    m.def("eig_phase1", &eig_phase1,
          "Sharded hypothetical pass A: slog2 partials (B*C, P)");
    m.def("eig_phase2", &eig_phase2,
          "Sharded hypothetical pass B: unnorm masses + totals");
}
