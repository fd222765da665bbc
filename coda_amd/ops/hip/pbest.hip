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
// Kernel inventory (host bindings at the bottom):
//   pbest_kernel           fused P(best) over (R, H) rows (v1)
//   eig_hyp_kernel         fused hypothetical P(best) + entropy (v1 EIG)
//   pbest/eig_phase1/2     two-phase variants with the model-axis
//                          all-reduce seam between passes (sharded v1)
//   es_build[_gathered]    v2: CSR-bucketed log-cdf scatter + exp2 +
//                          trapz weights -> the GEMM B operand (bf16/f32)
//   eig_assemble_kernel    v2: variant select + normalize + log2 entropy
//   eig_totals/entropy     v2 sharded split around the normalizer
//                          all-reduce
//   beta_row_tables_kernel v2: per-class incremental table refresh
//   pbest_phase1/2_wide    wide-H (> 2048 models): the two-pass split with
//                          LDS column windows as the "ranks", coupled
//                          through global memory on one device
//   pi_hat_delta_kernel    rank-1 posterior-marginal increment
//   pi_hat_delta_part      H-chunked variant for wide pools (blockIdx.y)
//   pi_marginal_kernel     streaming scaled column sum for pi_hat
//   col_add_kernel         fused adjusted[:, y] += delta; row_sums += delta
//   dirichlet_add_kernel   dir[h, y, cls_h] += lr posterior scatter

#include <torch/extension.h>
#include <hip/hip_runtime.h>
#include <c10/hip/HIPStream.h>
#include <hip/hip_bfloat16.h>
#include <hip/hip_fp8.h>  // __hip_fp8_e4m3 (OCP = torch.float8_e4m3fn)
#include <algorithm>
#include <vector>

#define P_POINTS 256
#define BLOCK 256

// Tuning hooks (scripts/build_variants.py): CODA_MIN_WAVES forces the
// register allocator toward higher occupancy; CODA_UNROLL_H software-
// pipelines the model loop (independent pdf math overlaps the scan's
// dependent shfl chain).
#ifdef CODA_MIN_WAVES
#define CODA_LB __launch_bounds__(BLOCK, CODA_MIN_WAVES)
#else
#define CODA_LB __launch_bounds__(BLOCK)
#endif
#define CODA_STR2(x) #x
#define CODA_STR(x) CODA_STR2(x)
#ifdef CODA_UNROLL_H
#define CODA_HLOOP _Pragma(CODA_STR(unroll CODA_UNROLL_H))
#else
#define CODA_HLOOP
#endif
#define ROWS_PER_BLOCK 4
#define PTS_PER_LANE 4
#define ES_LONG_ROW 512

namespace {

constexpr double kGridLo = 1e-6;
constexpr double kGridHi = 1.0 - 1e-6;
constexpr float kEps = 1e-30f;
constexpr float kLogClamp = 80.0f;               // natural-log clamp (reference)
constexpr float kLog2Clamp = 115.41560327111707f; // same clamp in base 2

#ifdef CODA_DPP_SCAN
// DPP cross-lane add: moved-in value (0 where no source / masked), added.
// dpp_ctrl: row_shr:N = 0x110|N, row_bcast15 = 0x142, row_bcast31 = 0x143.
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ float dpp_add(float x) {
    int moved = __builtin_amdgcn_update_dpp(0, __float_as_int(x), CTRL,
                                            ROW_MASK, 0xf, true);
    return x + __int_as_float(moved);
}

// Wave64 inclusive add-scan in 6 DPP VALU ops (1-2 cycle dependent
// latency each) instead of 6 dependent ds_bpermute rounds (~50 cycles
// each): the classic GCN row_shr/row_bcast ladder.
__device__ __forceinline__ float wave_inclusive_scan(float v) {
    v = dpp_add<0x111, 0xf>(v);  // row_shr:1
    v = dpp_add<0x112, 0xf>(v);  // row_shr:2
    v = dpp_add<0x114, 0xf>(v);  // row_shr:4
    v = dpp_add<0x118, 0xf>(v);  // row_shr:8  (rows of 16 complete)
    v = dpp_add<0x142, 0xa>(v);  // row_bcast:15 -> rows 1, 3
    v = dpp_add<0x143, 0xc>(v);  // row_bcast:31 -> rows 2, 3
    return v;
}

__device__ __forceinline__ float wave_reduce_sum(float v) {
    return __int_as_float(__builtin_amdgcn_readlane(
        __float_as_int(wave_inclusive_scan(v)), 63));
}
#else
__device__ __forceinline__ float wave_inclusive_scan(float v) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        float n = __shfl_up(v, off, 64);
        if (lane >= off) v += n;
    }
    return v;
}

__device__ __forceinline__ float wave_reduce_sum(float v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}
#endif

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
// Shared per-lane grid state: base-2 logs of this lane's 4 grid points,
// delta-centered (see pass A comment below).
struct LaneGrid {
    double lx0, l1mx0;
    float dlx[PTS_PER_LANE], dl1mx[PTS_PER_LANE];
    float dxf;
    __device__ void init(int lane) {
        const double step = (kGridHi - kGridLo) / (P_POINTS - 1);
        dxf = (float)step;
        double x0 = kGridLo + (double)(lane * PTS_PER_LANE) * step;
        lx0 = log2(x0);
        l1mx0 = log2(1.0 - x0);
#pragma unroll
        for (int j = 0; j < PTS_PER_LANE; ++j) {
            double x = kGridLo + (double)(lane * PTS_PER_LANE + j) * step;
            dlx[j] = (float)(log2(x) - lx0);
            dl1mx[j] = (float)(log2(1.0 - x) - l1mx0);
        }
    }
    // Delta-centered log-pdf: the large, cancellation-prone anchor
    //   K = am1*lx0 + bm1*l1mx0 - log2B
    // is computed in f64 once per (model, lane); per-point remainders are
    // small f32 deltas (~1e-5 absolute accuracy in the base-2 exponent at
    // any Beta count).
    __device__ __forceinline__ void pdf4(float a, float b, double lnB,
                                         float (&pdf)[PTS_PER_LANE]) const {
        const float am1 = a - 1.0f;
        const float bm1 = b - 1.0f;
        const float K = (float)((double)am1 * lx0 + (double)bm1 * l1mx0
                                - lnB);
#pragma unroll
        for (int j = 0; j < PTS_PER_LANE; ++j)
            pdf[j] = exp2f(fmaf(am1, dlx[j], fmaf(bm1, dl1mx[j], K)));
    }
    // pdf4 variant that also returns the base-2 log-pdf values (t2).
    __device__ __forceinline__ void pdf4_log(float a, float b, double lnB,
                                             float (&pdf)[PTS_PER_LANE],
                                             float (&t2)[PTS_PER_LANE]) const {
        const float am1 = a - 1.0f;
        const float bm1 = b - 1.0f;
        const float K = (float)((double)am1 * lx0 + (double)bm1 * l1mx0
                                - lnB);
#pragma unroll
        for (int j = 0; j < PTS_PER_LANE; ++j) {
            t2[j] = fmaf(am1, dlx[j], fmaf(bm1, dl1mx[j], K));
            pdf[j] = exp2f(t2[j]);
        }
    }

    // Trapezoid-cumulative cdf at this lane's 4 points from the wave's pdf.
    __device__ __forceinline__ void cdf4(const float (&pdf)[PTS_PER_LANE],
                                         int lane,
                                         float (&cdf)[PTS_PER_LANE]) const {
        float prev3 = __shfl_up(pdf[PTS_PER_LANE - 1], 1, 64);
        float tr0 = (lane == 0) ? 0.f : 0.5f * (pdf[0] + prev3) * dxf;
        float tr1 = 0.5f * (pdf[1] + pdf[0]) * dxf;
        float tr2 = 0.5f * (pdf[2] + pdf[1]) * dxf;
        float tr3 = 0.5f * (pdf[3] + pdf[2]) * dxf;
        float local = tr0 + tr1 + tr2 + tr3;
        float base = wave_inclusive_scan(local) - local;
        cdf[0] = base + tr0;
        cdf[1] = cdf[0] + tr1;
        cdf[2] = cdf[1] + tr2;
        cdf[3] = cdf[2] + tr3;
    }
};

// Pass A: slog2[j] = log2 PROD_h clamp(cdf_h(p_j), 1e-30), accumulated as
// a (mantissa, exponent) pair - one multiply + native v_frexp per model
// instead of a per-model v_log (base-2 log taken once at the end).
__device__ void pbest_pass_a(const float* s_a, const float* s_b,
                             const double* s_lnB, int H,
                             const LaneGrid& g, int lane,
                             float (&slog2)[PTS_PER_LANE]) {
    float pm[PTS_PER_LANE] = {1.f, 1.f, 1.f, 1.f};
    int pe_[PTS_PER_LANE] = {0, 0, 0, 0};
    CODA_HLOOP
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
    CODA_HLOOP
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

constexpr size_t lds_bytes(int H) {
    // per row: lnB (f64 H) + a, b, pb (f32 H each)
    return (size_t)ROWS_PER_BLOCK * ((size_t)H * 8 + 3 * (size_t)H * 4);
}

// ---------------------------------------------------------------------------
// Kernel 1: generic P(best). alpha/beta: (R, H) -> out: (R, H).
// ---------------------------------------------------------------------------
__global__ void CODA_LB
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
__global__ void CODA_LB
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
__global__ void CODA_LB
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
__global__ void CODA_LB
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

__global__ void CODA_LB
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

__global__ void CODA_LB
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

__global__ void CODA_LB
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

__global__ void CODA_LB
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

__global__ void CODA_LB
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


// ---------------------------------------------------------------------------
// Table-path (v2) fusion kernels. The table-factored EIG (coda_amd/ops/
// table.py) pairs per-step curve tables with per-chunk candidate state;
// these two kernels fuse its elementwise/scatter glue:
//   es_build: ES[c,b,p] = w[p] * 2^( s_base[c,p]
//                + sum_{h: cls(b,h)==c} delta[c,h,p] )
//     - one wave per (b,c) row; the h loop is a wave-uniform compare with
//       a rare (avg H/C) delta-row accumulate; replaces a repeat +
//       scatter-add + exp2 + mul chain over (B,C,P).
//   eig_assemble_k: given M[c,b,2h+v] (the GEMM output), select
//       v = [cls(b,h)==c], normalize over h, and emit the log2-entropy
//       H_after[b,c] of the updated P(best) mixture.
// ---------------------------------------------------------------------------
template <typename TOUT>
__global__ void __launch_bounds__(BLOCK)
es_build_kernel(const float* __restrict__ s_base,   // (C, P)
                const float* __restrict__ delta,    // (C, H, P)
                const float* __restrict__ dall,     // (C, P) sum over h
                const int* __restrict__ hvals,      // (B, H) h sorted by class
                const int* __restrict__ offsets,    // (B, C+1) CSR
                const float* __restrict__ w,        // (P,)
                TOUT* __restrict__ es,              // (C, B, P)
                int B, int C, int H) {
    // 16 lanes per (b, c) row, 16 grid points per lane. A majority
    // class (e.g. ~75% of a 10k-model pool predicting the consensus
    // label) used to serialize one wave on thousands of dependent
    // row loads; rows whose bucket exceeds H/2 now sum the COMPLEMENT
    // positions ([0,k0) u [k1,H) of the same sorted-permutation row)
    // and subtract from the per-class total dall[c], capping the chain
    // at H/2 and halving worst-case traffic.
    const int r = blockIdx.x * 16 + (threadIdx.x >> 4);
    if (r >= B * C) return;
    const int b = r / C, c = r - b * C;
    const int sub = threadIdx.x & 15;
    const int p0 = sub * 16;
    const size_t dbase = (size_t)c * H * P_POINTS + p0;
    const int* hrow = hvals + (size_t)b * H;
    const int k0 = offsets[(size_t)b * (C + 1) + c];
    const int k1 = offsets[(size_t)b * (C + 1) + c + 1];
    const bool comp = (k1 - k0) > H / 2;
    const int len_eff = comp ? (H - (k1 - k0)) : (k1 - k0);
    if (len_eff > ES_LONG_ROW) return;  // block-per-row kernel's rows

    float a0[16] = {}, a1[16] = {};
    auto addrow = [&](int h, float* acc) {
        const float4* d = reinterpret_cast<const float4*>(
            delta + dbase + (size_t)h * P_POINTS);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const float4 v = d[q];
            acc[4 * q] += v.x; acc[4 * q + 1] += v.y;
            acc[4 * q + 2] += v.z; acc[4 * q + 3] += v.w;
        }
    };
    if (!comp) {
        int k = k0;
        for (; k + 1 < k1; k += 2) {          // 2 rows in flight
            addrow(hrow[k], a0);
            addrow(hrow[k + 1], a1);
        }
        if (k < k1) addrow(hrow[k], a0);
    } else {
        int k = 0;
        for (; k + 1 < k0; k += 2) {
            addrow(hrow[k], a0);
            addrow(hrow[k + 1], a1);
        }
        if (k < k0) addrow(hrow[k], a0);
        k = k1;
        for (; k + 1 < H; k += 2) {
            addrow(hrow[k], a0);
            addrow(hrow[k + 1], a1);
        }
        if (k < H) addrow(hrow[k], a0);
    }

    const float4* sb = reinterpret_cast<const float4*>(
        s_base + (size_t)c * P_POINTS + p0);
    const float4* da = comp ? reinterpret_cast<const float4*>(
        dall + (size_t)c * P_POINTS + p0) : nullptr;
    const float4* wv = reinterpret_cast<const float4*>(w + p0);
    float out[16];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const float4 s = sb[q];
        const float4 ww = wv[q];
        float sx[4] = {s.x, s.y, s.z, s.w};
        float wx[4] = {ww.x, ww.y, ww.z, ww.w};
        float dx[4] = {0.f, 0.f, 0.f, 0.f};
        if (comp) {
            const float4 dv = da[q];
            dx[0] = dv.x; dx[1] = dv.y; dx[2] = dv.z; dx[3] = dv.w;
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int i = 4 * q + j;
            const float dsum = comp ? dx[j] - (a0[i] + a1[i])
                                    : a0[i] + a1[i];
            out[i] = exp2f(sx[j] + dsum) * wx[j];
        }
    }
    TOUT* dst = es + ((size_t)c * B + b) * P_POINTS + p0;
#pragma unroll
    for (int i = 0; i < 16; ++i) dst[i] = (TOUT)out[i];
}

// Block-per-row companion for rows whose (possibly complemented)
// bucket is still long (wide pools: a 10k-model consensus class leaves
// ~2500 rows even after complementing - a serial per-wave chain).
// 4 waves split the k-range; lane owns 4 grid points; partials reduce
// through LDS in fixed wave order (deterministic).
template <typename TOUT>
__global__ void __launch_bounds__(BLOCK)
es_build_long_kernel(const float* __restrict__ s_base,
                     const float* __restrict__ delta,
                     const float* __restrict__ dall,
                     const int* __restrict__ hvals,
                     const int* __restrict__ offsets,
                     const float* __restrict__ w,
                     TOUT* __restrict__ es,
                     int B, int C, int H) {
    const int r = blockIdx.x;
    if (r >= B * C) return;
    const int b = r / C, c = r - b * C;
    const int k0 = offsets[(size_t)b * (C + 1) + c];
    const int k1 = offsets[(size_t)b * (C + 1) + c + 1];
    const bool comp = (k1 - k0) > H / 2;
    const int len_eff = comp ? (H - (k1 - k0)) : (k1 - k0);
    if (len_eff <= ES_LONG_ROW) return;  // short kernel's rows

    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int p0 = lane * PTS_PER_LANE;
    const size_t dbase = (size_t)c * H * P_POINTS + p0;
    const int* hrow = hvals + (size_t)b * H;

    float a0[4] = {0.f, 0.f, 0.f, 0.f}, a1[4] = {0.f, 0.f, 0.f, 0.f};
    auto addrow = [&](int h, float* acc) {
        const float4 d = *reinterpret_cast<const float4*>(
            delta + dbase + (size_t)h * P_POINTS);
        acc[0] += d.x; acc[1] += d.y; acc[2] += d.z; acc[3] += d.w;
    };
    // the wave's k-slice: [lo, hi) of the (complement) iteration space
    auto scan = [&](int s0, int s1) {
        const int n = s1 - s0;
        const int per = (n + 3) / 4;
        int lo = s0 + wave * per;
        int hi = min(s1, lo + per);
        int k = lo;
        for (; k + 1 < hi; k += 2) {
            addrow(hrow[k], a0);
            addrow(hrow[k + 1], a1);
        }
        if (k < hi) addrow(hrow[k], a0);
    };
    if (!comp) {
        scan(k0, k1);
    } else {
        // complement = positions outside [k0, k1) of the same row;
        // treat as one logical range of length k0 + (H - k1)
        const int n = k0 + (H - k1);
        const int per = (n + 3) / 4;
        int lo = wave * per;
        int hi = min(n, lo + per);
        for (int s = lo; s < hi; ++s) {
            const int k = (s < k0) ? s : (k1 + (s - k0));
            addrow(hrow[k], a0);
        }
    }

    __shared__ float part[4][P_POINTS];
#pragma unroll
    for (int j = 0; j < 4; ++j)
        part[wave][p0 + j] = a0[j] + a1[j];
    __syncthreads();
    if (wave == 0) {
        const float4 sb = *reinterpret_cast<const float4*>(
            s_base + (size_t)c * P_POINTS + p0);
        const float4 wv = *reinterpret_cast<const float4*>(w + p0);
        float sx[4] = {sb.x, sb.y, sb.z, sb.w};
        float wx[4] = {wv.x, wv.y, wv.z, wv.w};
        float dx[4] = {0.f, 0.f, 0.f, 0.f};
        if (comp) {
            const float4 dv = *reinterpret_cast<const float4*>(
                dall + (size_t)c * P_POINTS + p0);
            dx[0] = dv.x; dx[1] = dv.y; dx[2] = dv.z; dx[3] = dv.w;
        }
        TOUT* dst = es + ((size_t)c * B + b) * P_POINTS + p0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float dsum0 = ((part[0][p0 + j] + part[1][p0 + j])
                               + (part[2][p0 + j] + part[3][p0 + j]));
            const float dsum = comp ? dx[j] - dsum0 : dsum0;
            dst[j] = (TOUT)(exp2f(sx[j] + dsum) * wx[j]);
        }
    }
}

template <typename TM>
__global__ void __launch_bounds__(BLOCK)
eig_assemble_kernel(const TM* __restrict__ m,               // (C, B, 2H)
                    const int* __restrict__ cls,            // (B, H)
                    const float* __restrict__ pi_hat,       // (C,)
                    const float* __restrict__ pbest_before, // (C, H)
                    const float* __restrict__ mixture0,     // (H,)
                    float* __restrict__ h_after,            // (B, C)
                    int B, int C, int H) {
    const int r = blockIdx.x * ROWS_PER_BLOCK + (threadIdx.x >> 6);
    if (r >= B * C) return;
    const int b = r / C, c = r - b * C;
    const int lane = threadIdx.x & 63;
    const TM* row = m + ((size_t)c * B + b) * (2 * H);

    float t0 = 0.f, t1 = 0.f, t2 = 0.f, t3 = 0.f;
    for (int h = lane; h < H; h += 256) {
#define ES_TOT_TERM(acc, hh) \
        if ((hh) < H) { \
            const int v_ = (cls[(size_t)b * H + (hh)] == c) ? 1 : 0; \
            acc += (float)row[2 * (hh) + v_]; \
        }
        ES_TOT_TERM(t0, h)
        ES_TOT_TERM(t1, h + 64)
        ES_TOT_TERM(t2, h + 128)
        ES_TOT_TERM(t3, h + 192)
#undef ES_TOT_TERM
    }
    float total = wave_reduce_sum((t0 + t1) + (t2 + t3));
    const float inv = 1.0f / fmaxf(total, kEps);

    const float pi_c = pi_hat[c];
    float e0 = 0.f, e1 = 0.f;
    for (int h = lane; h < H; h += 128) {
        const int v = (cls[(size_t)b * H + h] == c) ? 1 : 0;
        const float pb = (float)row[2 * h + v] * inv;
        float mm = mixture0[h]
                 + pi_c * (pb - pbest_before[(size_t)c * H + h]);
        e0 += -fmaxf(mm, 1e-12f) * __log2f(fmaxf(mm, 1e-12f));
        const int h2 = h + 64;
        if (h2 < H) {
            const int v2 = (cls[(size_t)b * H + h2] == c) ? 1 : 0;
            const float pb2 = (float)row[2 * h2 + v2] * inv;
            float m2 = mixture0[h2]
                     + pi_c * (pb2 - pbest_before[(size_t)c * H + h2]);
            e1 += -fmaxf(m2, 1e-12f) * __log2f(fmaxf(m2, 1e-12f));
        }
    }
    const float ent = wave_reduce_sum(e0 + e1);
    if (lane == 0) h_after[r] = ent;
}


// Sharded-v2 variants: the cross-rank coupling arrives as the gathered
// selected-delta curves sel_all (B, Hg, P) + gathered classes (B, Hg);
// normalization needs a GLOBAL total, so the assemble step splits into a
// totals kernel (partial sums, all-reduced by the host) and an entropy
// kernel consuming the reduced totals.
template <typename TOUT>
__global__ void __launch_bounds__(BLOCK)
es_build_gathered_kernel(const float* __restrict__ s_base_all,  // (C, P)
                         const float* __restrict__ sel_all,  // (B, Hg, P)
                         const int* __restrict__ hvals,      // (B, Hg) CSR
                         const int* __restrict__ offsets,    // (B, C+1)
                         const float* __restrict__ w,        // (P,)
                         TOUT* __restrict__ es,              // (C, B, P)
                         int B, int C, int Hg) {
    const int r = blockIdx.x * ROWS_PER_BLOCK + (threadIdx.x >> 6);
    if (r >= B * C) return;
    const int b = r / C, c = r - b * C;
    const int lane = threadIdx.x & 63;
    const int p0 = lane * PTS_PER_LANE;

    float acc[PTS_PER_LANE];
    const float4 sb = *reinterpret_cast<const float4*>(
        s_base_all + (size_t)c * P_POINTS + p0);
    acc[0] = sb.x; acc[1] = sb.y; acc[2] = sb.z; acc[3] = sb.w;
    const size_t sbase = (size_t)b * Hg * P_POINTS + p0;
    const int k0 = offsets[(size_t)b * (C + 1) + c];
    const int k1 = offsets[(size_t)b * (C + 1) + c + 1];
    float a1[4] = {0.f, 0.f, 0.f, 0.f}, a2[4] = {0.f, 0.f, 0.f, 0.f},
          a3[4] = {0.f, 0.f, 0.f, 0.f};
    int k = k0;
    for (; k + 3 < k1; k += 4) {
        const int ha = hvals[(size_t)b * Hg + k];
        const int hb = hvals[(size_t)b * Hg + k + 1];
        const int hc2 = hvals[(size_t)b * Hg + k + 2];
        const int hd = hvals[(size_t)b * Hg + k + 3];
        const float4 da = *reinterpret_cast<const float4*>(
            sel_all + sbase + (size_t)ha * P_POINTS);
        const float4 db = *reinterpret_cast<const float4*>(
            sel_all + sbase + (size_t)hb * P_POINTS);
        const float4 dc = *reinterpret_cast<const float4*>(
            sel_all + sbase + (size_t)hc2 * P_POINTS);
        const float4 dd = *reinterpret_cast<const float4*>(
            sel_all + sbase + (size_t)hd * P_POINTS);
        acc[0] += da.x; acc[1] += da.y; acc[2] += da.z; acc[3] += da.w;
        a1[0] += db.x; a1[1] += db.y; a1[2] += db.z; a1[3] += db.w;
        a2[0] += dc.x; a2[1] += dc.y; a2[2] += dc.z; a2[3] += dc.w;
        a3[0] += dd.x; a3[1] += dd.y; a3[2] += dd.z; a3[3] += dd.w;
    }
    for (; k < k1; ++k) {
        const int h = hvals[(size_t)b * Hg + k];
        const float4 d = *reinterpret_cast<const float4*>(
            sel_all + sbase + (size_t)h * P_POINTS);
        acc[0] += d.x; acc[1] += d.y; acc[2] += d.z; acc[3] += d.w;
    }
#pragma unroll
    for (int j = 0; j < PTS_PER_LANE; ++j)
        acc[j] += (a1[j] + a2[j]) + a3[j];
    const float4 wv = *reinterpret_cast<const float4*>(w + p0);
    TOUT* dst = es + ((size_t)c * B + b) * P_POINTS + p0;
    dst[0] = (TOUT)(exp2f(acc[0]) * wv.x);
    dst[1] = (TOUT)(exp2f(acc[1]) * wv.y);
    dst[2] = (TOUT)(exp2f(acc[2]) * wv.z);
    dst[3] = (TOUT)(exp2f(acc[3]) * wv.w);
}

template <typename TM>
__global__ void __launch_bounds__(BLOCK)
eig_totals_kernel(const TM* __restrict__ m,       // (C, B, 2H)
                  const int* __restrict__ cls,    // (B, H) local
                  float* __restrict__ totals,     // (B, C) partial
                  int B, int C, int H) {
    const int r = blockIdx.x * ROWS_PER_BLOCK + (threadIdx.x >> 6);
    if (r >= B * C) return;
    const int b = r / C, c = r - b * C;
    const int lane = threadIdx.x & 63;
    const TM* row = m + ((size_t)c * B + b) * (2 * H);
    float total = 0.f;
    for (int h = lane; h < H; h += 64) {
        const int v = (cls[(size_t)b * H + h] == c) ? 1 : 0;
        total += (float)row[2 * h + v];
    }
    total = wave_reduce_sum(total);
    if (lane == 0) totals[r] = total;
}

template <typename TM>
__global__ void __launch_bounds__(BLOCK)
eig_entropy_kernel(const TM* __restrict__ m,               // (C, B, 2H)
                   const int* __restrict__ cls,            // (B, H) local
                   const float* __restrict__ totals,       // (B, C) GLOBAL
                   const float* __restrict__ pi_hat,       // (C,)
                   const float* __restrict__ pbest_before, // (C, H) local
                   const float* __restrict__ mixture0,     // (H,) local
                   float* __restrict__ h_after,            // (B, C) partial
                   int B, int C, int H) {
    const int r = blockIdx.x * ROWS_PER_BLOCK + (threadIdx.x >> 6);
    if (r >= B * C) return;
    const int b = r / C, c = r - b * C;
    const int lane = threadIdx.x & 63;
    const TM* row = m + ((size_t)c * B + b) * (2 * H);
    const float inv = 1.0f / fmaxf(totals[r], kEps);
    const float pi_c = pi_hat[c];
    float ent = 0.f;
    for (int h = lane; h < H; h += 64) {
        const int v = (cls[(size_t)b * H + h] == c) ? 1 : 0;
        const float pb = (float)row[2 * h + v] * inv;
        float mm = mixture0[h]
                 + pi_c * (pb - pbest_before[(size_t)c * H + h]);
        mm = fmaxf(mm, 1e-12f);
        ent += -mm * __log2f(mm);
    }
    ent = wave_reduce_sum(ent);
    if (lane == 0) h_after[r] = ent;
}


// Per-class table refresh (v2): recompute the H*2 hypothetical Beta
// curves of ONE class row - what changes between steps (add_label moves
// only Dirichlet row true_class). One wave per (model, variant) pair;
// writes EG = 2^(log2 pdf - log2 cdf) and lc = log2 cdf; the tiny
// delta/s_base combines stay on the host.
__global__ void __launch_bounds__(BLOCK)
beta_row_tables_kernel(const float* __restrict__ alpha_col,  // (H,)
                       const float* __restrict__ beta_col,   // (H,)
                       float* __restrict__ eg,                // (H, 2, P)
                       float* __restrict__ lc_out,            // (H, 2, P)
                       float update_weight, int H) {
    const int q = blockIdx.x * ROWS_PER_BLOCK + (threadIdx.x >> 6);
    if (q >= 2 * H) return;
    const int h = q >> 1, v = q & 1;
    const int lane = threadIdx.x & 63;
    const float a = alpha_col[h] + (v ? update_weight : 0.f);
    const float b = beta_col[h] + (v ? 0.f : update_weight);
    const double lnB = (lgamma((double)a) + lgamma((double)b)
                      - lgamma((double)a + (double)b)) * 1.4426950408889634;
    LaneGrid g;
    g.init(lane);
    float pdf[PTS_PER_LANE], t2[PTS_PER_LANE], cdf[PTS_PER_LANE];
    g.pdf4_log(a, b, lnB, pdf, t2);
    g.cdf4(pdf, lane, cdf);
    const size_t base = (size_t)q * P_POINTS + lane * PTS_PER_LANE;
    float4 lcv, egv;
    float lcj[PTS_PER_LANE];
#pragma unroll
    for (int j = 0; j < PTS_PER_LANE; ++j)
        lcj[j] = __log2f(fmaxf(cdf[j], kEps));
    lcv.x = lcj[0]; lcv.y = lcj[1]; lcv.z = lcj[2]; lcv.w = lcj[3];
    egv.x = exp2f(t2[0] - lcj[0]);
    egv.y = exp2f(t2[1] - lcj[1]);
    egv.z = exp2f(t2[2] - lcj[2]);
    egv.w = exp2f(t2[3] - lcj[3]);
    *reinterpret_cast<float4*>(lc_out + base) = lcv;
    *reinterpret_cast<float4*>(eg + base) = egv;
}


// ---------------------------------------------------------------------------
// Per-label table-row commit (v2/v3 tables).  After beta_row_tables
// recomputes class y's eg/lc curves, the torch commit chain was ~14
// small launches (~4.8 us each in-graph: index_copy x5, two 32-thread
// strided reductions at 10-24 us, exp2/mul/convert kernels).  Three
// kernels replace the whole chain:
//   trc_cols   a_col/b_col from the Dirichlet row (the (H, C).sum(1)
//              was a 24 us 32-thread torch reduce)
//   trc_sums   s_base[y], dall[y], esb scratch (fixed-order H sums)
//   trc_rows   EG/eg16/egw/delta/delta16 row writes + conversions
// y is read from the device tensor so the label graph can replay with
// a changed class.
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(BLOCK)
trc_cols_kernel(const float* __restrict__ dir,   // (H, C, C)
                const long long* __restrict__ y, // (1,)
                float* __restrict__ a_col,       // (H,)
                float* __restrict__ b_col,       // (H,)
                int H, int C) {
    const int h = blockIdx.x;
    const long long yy = y[0];
    const float* row = dir + ((size_t)h * C + yy) * C;
    float s = 0.f;
    for (int c = threadIdx.x; c < C; c += BLOCK) s += row[c];
    __shared__ float ss[BLOCK];
    ss[threadIdx.x] = s;
    __syncthreads();
    for (int k = BLOCK / 2; k > 0; k >>= 1) {
        if (threadIdx.x < k) ss[threadIdx.x] += ss[threadIdx.x + k];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const float a = row[yy];
        a_col[h] = a;
        b_col[h] = ss[0] - a;
    }
}

__global__ void __launch_bounds__(P_POINTS)
trc_sums_kernel(const float* __restrict__ lc,    // (H, 2, P)
                const float* __restrict__ w,     // (P,)
                const long long* __restrict__ y,
                float* __restrict__ s_base,      // (C, P)
                float* __restrict__ dall,        // (C, P)
                float* __restrict__ esb,         // (P,) scratch
                int H) {
    const int p = threadIdx.x;
    const long long yy = y[0];
    // 2-row unroll with split accumulators: the serial strided walk
    // over H rows was ~34 us latency-bound on one workgroup
    float s = 0.f, d = 0.f, s2 = 0.f, d2 = 0.f;
    int h = 0;
    for (; h + 1 < H; h += 2) {
        const float l0 = lc[((size_t)h * 2) * P_POINTS + p];
        const float l1 = lc[((size_t)h * 2 + 1) * P_POINTS + p];
        const float m0 = lc[((size_t)(h + 1) * 2) * P_POINTS + p];
        const float m1 = lc[((size_t)(h + 1) * 2 + 1) * P_POINTS + p];
        s += l0;       d += l1 - l0;
        s2 += m0;      d2 += m1 - m0;
    }
    if (h < H) {
        const float l0 = lc[((size_t)h * 2) * P_POINTS + p];
        const float l1 = lc[((size_t)h * 2 + 1) * P_POINTS + p];
        s += l0;
        d += l1 - l0;
    }
    s += s2;
    d += d2;
    s_base[yy * P_POINTS + p] = s;
    dall[yy * P_POINTS + p] = d;
    esb[p] = exp2f(s) * w[p];
}

__global__ void __launch_bounds__(BLOCK)
trc_rows_kernel(const float* __restrict__ eg,    // (H, 2, P)
                const float* __restrict__ lc,    // (H, 2, P)
                const float* __restrict__ esb,   // (P,)
                const long long* __restrict__ y,
                float* __restrict__ EG,          // (C, H, 2, P)
                float* __restrict__ delta,       // (C, H, P)
                hip_bfloat16* __restrict__ eg16, // (C, 2H, P)
                hip_bfloat16* __restrict__ egw,  // (C, 2H, P)
                _Float16* __restrict__ delta16,  // (C, H, P)
                int H) {
    const int i = blockIdx.x * BLOCK + threadIdx.x;  // over (2H, P)
    if (i >= 2 * H * P_POINTS) return;
    const int p = i & (P_POINTS - 1);
    const int q = i >> 8;                            // (h, v)
    const long long yy = y[0];
    const float e = eg[i];
    const size_t rbase = (size_t)yy * 2 * H * P_POINTS;
    EG[rbase + i] = e;
    eg16[rbase + i] = hip_bfloat16(e);
    egw[rbase + i] = hip_bfloat16(e * esb[p]);
    if (q & 1) {   // one visit per (h, p): the v == 1 thread
        const int h = q >> 1;
        const float dv = lc[i] - lc[i - P_POINTS];
        const size_t dbase = ((size_t)yy * H + h) * P_POINTS + p;
        delta[dbase] = dv;
        delta16[dbase] = (_Float16)dv;
    }
}

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
__global__ void CODA_LB
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
__global__ void CODA_LB
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
__global__ void CODA_LB
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

// cls of the v2 assemble kernels: (B, H) int32 next to m (C, B, 2H)
static void check_cls_for_m(const torch::Tensor& m,
                            const torch::Tensor& cls) {
    TORCH_CHECK(m.dim() == 3 && m.size(2) % 2 == 0, "m must be (C, B, 2H)");
    TORCH_CHECK(m.scalar_type() == torch::kFloat32 ||
                m.scalar_type() == torch::kBFloat16,
                "m must be fp32 or bf16");
    TORCH_CHECK(cls.is_cuda() && cls.is_contiguous(),
                "cls must be contiguous on a ROCm device");
    TORCH_CHECK(cls.scalar_type() == torch::kInt32, "cls must be int32");
    TORCH_CHECK(cls.dim() == 2 && cls.size(0) == m.size(1) &&
                cls.size(1) == m.size(2) / 2, "cls must be (B, H)");
}

static void check_f32_cuda(const torch::Tensor& t, const char* name) {
    TORCH_CHECK(t.is_cuda(), name, " must be on a ROCm device");
    TORCH_CHECK(t.scalar_type() == torch::kFloat32, name, " must be fp32");
    TORCH_CHECK(t.is_contiguous(), name, " must be contiguous");
}

// (R, H) Beta rows of the v1 phase kernels
static void check_beta_rows(const torch::Tensor& alpha,
                            const torch::Tensor& beta) {
    check_f32_cuda(alpha, "alpha");
    check_f32_cuda(beta, "beta");
    TORCH_CHECK(alpha.dim() == 2 && alpha.sizes() == beta.sizes(),
                "alpha/beta must be (R, H)");
}

// the H-coupling term a phase-2 kernel reads: one 256-point row per
// P(best) row
static void check_slog2(const torch::Tensor& slog2, int64_t rows) {
    check_f32_cuda(slog2, "slog2");
    TORCH_CHECK(slog2.dim() == 2 && slog2.size(0) == rows &&
                slog2.size(1) == P_POINTS,
                "slog2 must be (R, 256), R = ", rows);
}

// (H, C) diagonal Betas + the (B, H) int32 argmax classes of the v1 EIG
// kernels (stage_hyp indexes cls[b * H + h] and alpha_t[c * H + h])
static void check_hyp_inputs(const torch::Tensor& alpha_cc,
                             const torch::Tensor& beta_cc,
                             const torch::Tensor& cls) {
    TORCH_CHECK(alpha_cc.is_cuda() && beta_cc.is_cuda(),
                "alpha_cc/beta_cc must be on a ROCm device");
    TORCH_CHECK(alpha_cc.scalar_type() == torch::kFloat32 &&
                beta_cc.scalar_type() == torch::kFloat32,
                "alpha_cc/beta_cc must be fp32");
    TORCH_CHECK(alpha_cc.dim() == 2 && alpha_cc.sizes() == beta_cc.sizes(),
                "alpha_cc/beta_cc must be (H, C)");
    TORCH_CHECK(cls.is_cuda() && cls.is_contiguous(),
                "chunk_classes must be contiguous on a ROCm device");
    TORCH_CHECK(cls.scalar_type() == torch::kInt32,
                "chunk_classes must be int32");
    TORCH_CHECK(cls.dim() == 2 && cls.size(1) == alpha_cc.size(0),
                "chunk_classes must be (B, H)");
}

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
    auto stream = c10::hip::getCurrentHIPStream();
    if (R == 1) {
        // one row would give the generic kernel a single wave; the row
        // kernel windows the model axis across the whole workgroup
        const int Hc = (H + ROWS_PER_BLOCK - 1) / ROWS_PER_BLOCK;
        const size_t smem = lds_bytes(Hc)
            + (ROWS_PER_BLOCK * P_POINTS + ROWS_PER_BLOCK) * sizeof(float);
        TORCH_CHECK(smem <= 160 * 1024, "H too large for LDS: ", H);
        hipLaunchKernelGGL(pbest_row_kernel, dim3(1), dim3(BLOCK), smem,
                           stream.stream(), alpha.data_ptr<float>(),
                           beta.data_ptr<float>(), out.data_ptr<float>(),
                           H);
        C10_HIP_CHECK(hipGetLastError());
        return out;
    }
    const size_t smem = lds_bytes(H);
    TORCH_CHECK(smem <= 160 * 1024, "H too large for LDS: ", H);
    const int blocks = (R + ROWS_PER_BLOCK - 1) / ROWS_PER_BLOCK;
    hipLaunchKernelGGL(pbest_kernel, dim3(blocks), dim3(BLOCK), smem,
                       stream.stream(), alpha.data_ptr<float>(),
                       beta.data_ptr<float>(), out.data_ptr<float>(), R, H);
    C10_HIP_CHECK(hipGetLastError());
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
    const size_t smem = lds_bytes(H);
    TORCH_CHECK(smem <= 160 * 1024, "H too large for LDS: ", H);
    const int R = B * C;
    const int blocks = (R + ROWS_PER_BLOCK - 1) / ROWS_PER_BLOCK;
    auto stream = c10::hip::getCurrentHIPStream();
    hipLaunchKernelGGL(eig_hyp_kernel, dim3(blocks), dim3(BLOCK), smem,
                       stream.stream(), alpha_t.data_ptr<float>(),
                       beta_t.data_ptr<float>(),
                       chunk_classes.data_ptr<int>(),
                       pbest_before.data_ptr<float>(),
                       pi_hat.data_ptr<float>(), mixture0.data_ptr<float>(),
                       h_after.data_ptr<float>(), (float)update_weight,
                       B, C, H);
    C10_HIP_CHECK(hipGetLastError());
    // EIG = H_before - sum_c pi_hat_xi[b,c] * H_after[b,c]
    return h_before - (pi_hat_xi * h_after).sum(-1);
}


// ---- Two-phase (sharded) host bindings ----

torch::Tensor pbest_phase1(torch::Tensor alpha, torch::Tensor beta) {
    check_beta_rows(alpha, beta);
    const int R = alpha.size(0), H = alpha.size(1);
    auto slog2 = torch::empty({R, P_POINTS}, alpha.options());
    if (R == 0) return slog2;
    const size_t smem = lds_bytes(H);
    TORCH_CHECK(smem <= 160 * 1024, "H too large for LDS: ", H);
    const int blocks = (R + ROWS_PER_BLOCK - 1) / ROWS_PER_BLOCK;
    auto stream = c10::hip::getCurrentHIPStream();
    hipLaunchKernelGGL(pbest_phase1_kernel, dim3(blocks), dim3(BLOCK), smem,
                       stream.stream(), alpha.data_ptr<float>(),
                       beta.data_ptr<float>(), slog2.data_ptr<float>(),
                       R, H);
    C10_HIP_CHECK(hipGetLastError());
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
    const size_t smem = lds_bytes(H);
    TORCH_CHECK(smem <= 160 * 1024, "H too large for LDS: ", H);
    const int blocks = (R + ROWS_PER_BLOCK - 1) / ROWS_PER_BLOCK;
    auto stream = c10::hip::getCurrentHIPStream();
    hipLaunchKernelGGL(pbest_phase2_kernel, dim3(blocks), dim3(BLOCK), smem,
                       stream.stream(), alpha.data_ptr<float>(),
                       beta.data_ptr<float>(), slog2.data_ptr<float>(),
                       pb.data_ptr<float>(), tot.data_ptr<float>(), R, H);
    C10_HIP_CHECK(hipGetLastError());
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
    const size_t smem = lds_bytes(Hc);
    TORCH_CHECK(smem <= 160 * 1024, "Hc too large for LDS: ", Hc);
    const int bx = (R + ROWS_PER_BLOCK - 1) / ROWS_PER_BLOCK;
    auto stream = c10::hip::getCurrentHIPStream();
    hipLaunchKernelGGL(pbest_phase1_wide_kernel, dim3(bx, KH), dim3(BLOCK),
                       smem, stream.stream(), alpha.data_ptr<float>(),
                       beta.data_ptr<float>(), part.data_ptr<float>(),
                       R, Htot, Hc);
    C10_HIP_CHECK(hipGetLastError());
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
    const size_t smem = lds_bytes(Hc);
    TORCH_CHECK(smem <= 160 * 1024, "Hc too large for LDS: ", Hc);
    const int bx = (R + ROWS_PER_BLOCK - 1) / ROWS_PER_BLOCK;
    auto stream = c10::hip::getCurrentHIPStream();
    hipLaunchKernelGGL(pbest_phase2_wide_kernel, dim3(bx, KH), dim3(BLOCK),
                       smem, stream.stream(), alpha.data_ptr<float>(),
                       beta.data_ptr<float>(), slog2.data_ptr<float>(),
                       pb.data_ptr<float>(), tot_part.data_ptr<float>(),
                       R, Htot, Hc);
    C10_HIP_CHECK(hipGetLastError());
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
    const size_t smem = lds_bytes(H);
    TORCH_CHECK(smem <= 160 * 1024, "H too large for LDS: ", H);
    const int R = B * C;
    const int blocks = (R + ROWS_PER_BLOCK - 1) / ROWS_PER_BLOCK;
    auto stream = c10::hip::getCurrentHIPStream();
    hipLaunchKernelGGL(eig_phase1_kernel, dim3(blocks), dim3(BLOCK), smem,
                       stream.stream(), alpha_t.data_ptr<float>(),
                       beta_t.data_ptr<float>(),
                       chunk_classes.data_ptr<int>(),
                       slog2.data_ptr<float>(), (float)update_weight,
                       B, C, H);
    C10_HIP_CHECK(hipGetLastError());
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
    const size_t smem = lds_bytes(H);
    TORCH_CHECK(smem <= 160 * 1024, "H too large for LDS: ", H);
    const int R = B * C;
    const int blocks = (R + ROWS_PER_BLOCK - 1) / ROWS_PER_BLOCK;
    auto stream = c10::hip::getCurrentHIPStream();
    hipLaunchKernelGGL(eig_phase2_kernel, dim3(blocks), dim3(BLOCK), smem,
                       stream.stream(), alpha_t.data_ptr<float>(),
                       beta_t.data_ptr<float>(),
                       chunk_classes.data_ptr<int>(),
                       slog2.data_ptr<float>(), pb.data_ptr<float>(),
                       tot.data_ptr<float>(), (float)update_weight,
                       B, C, H);
    C10_HIP_CHECK(hipGetLastError());
    return {pb, tot};
}


// ---- Table-path (v2) fusion host bindings ----

torch::Tensor es_build(torch::Tensor s_base, torch::Tensor delta,
                       torch::Tensor dall,
                       torch::Tensor hvals, torch::Tensor offsets,
                       torch::Tensor w, bool bf16_out) {
    check_f32_cuda(s_base, "s_base");
    check_f32_cuda(delta, "delta");
    check_f32_cuda(dall, "dall");
    check_f32_cuda(w, "w");
    TORCH_CHECK(hvals.scalar_type() == torch::kInt32 &&
                offsets.scalar_type() == torch::kInt32,
                "hvals/offsets must be int32");
    TORCH_CHECK(s_base.dim() == 2 && s_base.size(1) == P_POINTS,
                "P must be 256");
    TORCH_CHECK(delta.dim() == 3 && delta.size(2) == P_POINTS,
                "delta must be (C, H, 256)");
    TORCH_CHECK(hvals.is_cuda() && hvals.is_contiguous() &&
                offsets.is_cuda() && offsets.is_contiguous() &&
                hvals.dim() == 2 && offsets.dim() == 2,
                "hvals/offsets must be contiguous 2-d device tensors");
    const int C = s_base.size(0), H = delta.size(1);
    const int B = hvals.size(0);
    TORCH_CHECK(delta.size(0) == C, "delta.size(0) must equal C");
    TORCH_CHECK(dall.dim() == 2 && dall.size(0) == C &&
                dall.size(1) == P_POINTS, "dall must be (C, 256)");
    TORCH_CHECK(hvals.size(1) == H, "hvals must be (B, H)");
    TORCH_CHECK(offsets.size(0) == B && offsets.size(1) == C + 1,
                "offsets must be (B, C+1)");
    TORCH_CHECK(w.numel() == P_POINTS, "w must be (256,)");
    auto es = torch::empty({C, B, P_POINTS},
                           s_base.options().dtype(
                               bf16_out ? torch::kBFloat16
                                        : torch::kFloat32));
    const int R = B * C;
    const int blocks = (R + 15) / 16;  // 16 sublane rows per block
    auto stream = c10::hip::getCurrentHIPStream();
    if (bf16_out) {
        hipLaunchKernelGGL(es_build_kernel<hip_bfloat16>, dim3(blocks),
                           dim3(BLOCK), 0, stream.stream(),
                           s_base.data_ptr<float>(),
                           delta.data_ptr<float>(),
                           dall.data_ptr<float>(),
                           hvals.data_ptr<int>(),
                           offsets.data_ptr<int>(), w.data_ptr<float>(),
                           reinterpret_cast<hip_bfloat16*>(es.data_ptr()),
                           B, C, H);
    } else {
        hipLaunchKernelGGL(es_build_kernel<float>, dim3(blocks),
                           dim3(BLOCK), 0, stream.stream(),
                           s_base.data_ptr<float>(),
                           delta.data_ptr<float>(),
                           dall.data_ptr<float>(),
                           hvals.data_ptr<int>(),
                           offsets.data_ptr<int>(), w.data_ptr<float>(),
                           es.data_ptr<float>(), B, C, H);
    }
    if (H > 2 * ES_LONG_ROW) {  // long rows only exist at wide pools
        if (bf16_out) {
            hipLaunchKernelGGL(es_build_long_kernel<hip_bfloat16>,
                               dim3(R), dim3(BLOCK), 0, stream.stream(),
                               s_base.data_ptr<float>(),
                               delta.data_ptr<float>(),
                               dall.data_ptr<float>(),
                               hvals.data_ptr<int>(),
                               offsets.data_ptr<int>(),
                               w.data_ptr<float>(),
                               reinterpret_cast<hip_bfloat16*>(
                                   es.data_ptr()),
                               B, C, H);
        } else {
            hipLaunchKernelGGL(es_build_long_kernel<float>,
                               dim3(R), dim3(BLOCK), 0, stream.stream(),
                               s_base.data_ptr<float>(),
                               delta.data_ptr<float>(),
                               dall.data_ptr<float>(),
                               hvals.data_ptr<int>(),
                               offsets.data_ptr<int>(),
                               w.data_ptr<float>(),
                               es.data_ptr<float>(), B, C, H);
        }
    }
    C10_HIP_CHECK(hipGetLastError());
    return es;
}

torch::Tensor eig_assemble_k(torch::Tensor m, torch::Tensor cls,
                             torch::Tensor pi_hat,
                             torch::Tensor pbest_before,
                             torch::Tensor mixture0) {
    TORCH_CHECK(m.is_cuda() && m.is_contiguous(), "m");
    check_f32_cuda(pi_hat, "pi_hat");
    check_f32_cuda(pbest_before, "pbest_before");
    check_f32_cuda(mixture0, "mixture0");
    check_cls_for_m(m, cls);
    const int C = m.size(0), B = m.size(1);
    const int H = m.size(2) / 2;
    auto h_after = torch::empty({B, C},
                                m.options().dtype(torch::kFloat32));
    const int R = B * C;
    const int blocks = (R + ROWS_PER_BLOCK - 1) / ROWS_PER_BLOCK;
    auto stream = c10::hip::getCurrentHIPStream();
    if (m.scalar_type() == torch::kBFloat16) {
        hipLaunchKernelGGL(eig_assemble_kernel<hip_bfloat16>, dim3(blocks),
                           dim3(BLOCK), 0, stream.stream(),
                           reinterpret_cast<const hip_bfloat16*>(
                               m.data_ptr()),
                           cls.data_ptr<int>(), pi_hat.data_ptr<float>(),
                           pbest_before.data_ptr<float>(),
                           mixture0.data_ptr<float>(),
                           h_after.data_ptr<float>(), B, C, H);
    } else {
        hipLaunchKernelGGL(eig_assemble_kernel<float>, dim3(blocks),
                           dim3(BLOCK), 0, stream.stream(),
                           m.data_ptr<float>(),
                           cls.data_ptr<int>(), pi_hat.data_ptr<float>(),
                           pbest_before.data_ptr<float>(),
                           mixture0.data_ptr<float>(),
                           h_after.data_ptr<float>(), B, C, H);
    }
    C10_HIP_CHECK(hipGetLastError());
    return h_after;
}


torch::Tensor es_build_gathered(torch::Tensor s_base_all,
                                torch::Tensor sel_all,
                                torch::Tensor hvals, torch::Tensor offsets,
                                torch::Tensor w, bool bf16_out) {
    check_f32_cuda(s_base_all, "s_base_all");
    check_f32_cuda(sel_all, "sel_all");
    check_f32_cuda(w, "w");
    TORCH_CHECK(hvals.scalar_type() == torch::kInt32 &&
                offsets.scalar_type() == torch::kInt32,
                "hvals/offsets must be int32");
    TORCH_CHECK(s_base_all.dim() == 2 && s_base_all.size(1) == P_POINTS,
                "P must be 256");
    TORCH_CHECK(hvals.is_cuda() && hvals.is_contiguous() &&
                offsets.is_cuda() && offsets.is_contiguous() &&
                hvals.dim() == 2 && offsets.dim() == 2,
                "hvals/offsets must be contiguous 2-d device tensors");
    const int C = s_base_all.size(0);
    const int B = hvals.size(0), Hg = hvals.size(1);
    TORCH_CHECK(sel_all.dim() == 3 && sel_all.size(0) == B &&
                sel_all.size(1) == Hg && sel_all.size(2) == P_POINTS,
                "sel_all must be (B, Hg, 256)");
    TORCH_CHECK(offsets.size(0) == B && offsets.size(1) == C + 1,
                "offsets must be (B, C+1)");
    TORCH_CHECK(w.numel() == P_POINTS, "w must be (256,)");
    auto es = torch::empty({C, B, P_POINTS},
                           s_base_all.options().dtype(
                               bf16_out ? torch::kBFloat16
                                        : torch::kFloat32));
    const int R = B * C;
    const int blocks = (R + ROWS_PER_BLOCK - 1) / ROWS_PER_BLOCK;
    auto stream = c10::hip::getCurrentHIPStream();
    if (bf16_out) {
        hipLaunchKernelGGL(es_build_gathered_kernel<hip_bfloat16>,
                           dim3(blocks), dim3(BLOCK), 0, stream.stream(),
                           s_base_all.data_ptr<float>(),
                           sel_all.data_ptr<float>(),
                           hvals.data_ptr<int>(), offsets.data_ptr<int>(),
                           w.data_ptr<float>(),
                           reinterpret_cast<hip_bfloat16*>(es.data_ptr()),
                           B, C, Hg);
    } else {
        hipLaunchKernelGGL(es_build_gathered_kernel<float>, dim3(blocks),
                           dim3(BLOCK), 0, stream.stream(),
                           s_base_all.data_ptr<float>(),
                           sel_all.data_ptr<float>(),
                           hvals.data_ptr<int>(), offsets.data_ptr<int>(),
                           w.data_ptr<float>(), es.data_ptr<float>(),
                           B, C, Hg);
    }
    C10_HIP_CHECK(hipGetLastError());
    return es;
}

torch::Tensor eig_totals(torch::Tensor m, torch::Tensor cls) {
    TORCH_CHECK(m.is_cuda() && m.is_contiguous(), "m");
    check_cls_for_m(m, cls);
    const int C = m.size(0), B = m.size(1), H = m.size(2) / 2;
    auto totals = torch::empty({B, C},
                               m.options().dtype(torch::kFloat32));
    const int R = B * C;
    const int blocks = (R + ROWS_PER_BLOCK - 1) / ROWS_PER_BLOCK;
    auto stream = c10::hip::getCurrentHIPStream();
    if (m.scalar_type() == torch::kBFloat16) {
        hipLaunchKernelGGL(eig_totals_kernel<hip_bfloat16>, dim3(blocks),
                           dim3(BLOCK), 0, stream.stream(),
                           reinterpret_cast<const hip_bfloat16*>(
                               m.data_ptr()),
                           cls.data_ptr<int>(), totals.data_ptr<float>(),
                           B, C, H);
    } else {
        hipLaunchKernelGGL(eig_totals_kernel<float>, dim3(blocks),
                           dim3(BLOCK), 0, stream.stream(),
                           m.data_ptr<float>(), cls.data_ptr<int>(),
                           totals.data_ptr<float>(), B, C, H);
    }
    C10_HIP_CHECK(hipGetLastError());
    return totals;
}

torch::Tensor eig_entropy(torch::Tensor m, torch::Tensor cls,
                          torch::Tensor totals, torch::Tensor pi_hat,
                          torch::Tensor pbest_before,
                          torch::Tensor mixture0) {
    TORCH_CHECK(m.is_cuda() && m.is_contiguous(), "m");
    check_cls_for_m(m, cls);
    check_f32_cuda(totals, "totals");
    check_f32_cuda(pi_hat, "pi_hat");
    check_f32_cuda(pbest_before, "pbest_before");
    check_f32_cuda(mixture0, "mixture0");
    const int C = m.size(0), B = m.size(1), H = m.size(2) / 2;
    TORCH_CHECK(totals.numel() == (int64_t)B * C, "totals must be (B, C)");
    TORCH_CHECK(pi_hat.numel() == C && mixture0.numel() == H &&
                pbest_before.numel() == (int64_t)C * H,
                "pi_hat (C,), pbest_before (C, H), mixture0 (H,)");
    auto h_after = torch::empty({B, C},
                                m.options().dtype(torch::kFloat32));
    const int R = B * C;
    const int blocks = (R + ROWS_PER_BLOCK - 1) / ROWS_PER_BLOCK;
    auto stream = c10::hip::getCurrentHIPStream();
    if (m.scalar_type() == torch::kBFloat16) {
        hipLaunchKernelGGL(eig_entropy_kernel<hip_bfloat16>, dim3(blocks),
                           dim3(BLOCK), 0, stream.stream(),
                           reinterpret_cast<const hip_bfloat16*>(
                               m.data_ptr()),
                           cls.data_ptr<int>(), totals.data_ptr<float>(),
                           pi_hat.data_ptr<float>(),
                           pbest_before.data_ptr<float>(),
                           mixture0.data_ptr<float>(),
                           h_after.data_ptr<float>(), B, C, H);
    } else {
        hipLaunchKernelGGL(eig_entropy_kernel<float>, dim3(blocks),
                           dim3(BLOCK), 0, stream.stream(),
                           m.data_ptr<float>(), cls.data_ptr<int>(),
                           totals.data_ptr<float>(),
                           pi_hat.data_ptr<float>(),
                           pbest_before.data_ptr<float>(),
                           mixture0.data_ptr<float>(),
                           h_after.data_ptr<float>(), B, C, H);
    }
    C10_HIP_CHECK(hipGetLastError());
    return h_after;
}


std::vector<torch::Tensor> beta_row_tables(torch::Tensor alpha_col,
                                           torch::Tensor beta_col,
                                           double update_weight) {
    check_f32_cuda(alpha_col, "alpha_col");
    check_f32_cuda(beta_col, "beta_col");
    const int H = alpha_col.size(0);
    auto eg = torch::empty({H, 2, P_POINTS}, alpha_col.options());
    auto lc = torch::empty({H, 2, P_POINTS}, alpha_col.options());
    const int R = 2 * H;
    const int blocks = (R + ROWS_PER_BLOCK - 1) / ROWS_PER_BLOCK;
    auto stream = c10::hip::getCurrentHIPStream();
    hipLaunchKernelGGL(beta_row_tables_kernel, dim3(blocks), dim3(BLOCK),
                       0, stream.stream(), alpha_col.data_ptr<float>(),
                       beta_col.data_ptr<float>(), eg.data_ptr<float>(),
                       lc.data_ptr<float>(), (float)update_weight, H);
    C10_HIP_CHECK(hipGetLastError());
    return {eg, lc};
}


static void commit_row_launch(torch::Tensor& eg, torch::Tensor& lc,
                              torch::Tensor& y, torch::Tensor& EG,
                              torch::Tensor& delta, torch::Tensor& s_base,
                              torch::Tensor& weights, torch::Tensor& eg16,
                              torch::Tensor& egw, torch::Tensor& delta16,
                              torch::Tensor& dall, int H) {
    auto stream = c10::hip::getCurrentHIPStream();
    auto esb = torch::empty({P_POINTS}, eg.options());
    hipLaunchKernelGGL(trc_sums_kernel, dim3(1), dim3(P_POINTS), 0,
                       stream.stream(), lc.data_ptr<float>(),
                       weights.data_ptr<float>(),
                       reinterpret_cast<const long long*>(
                           y.data_ptr<int64_t>()),
                       s_base.data_ptr<float>(),
                       dall.data_ptr<float>(), esb.data_ptr<float>(), H);
    const int total = 2 * H * P_POINTS;
    hipLaunchKernelGGL(trc_rows_kernel,
                       dim3((total + BLOCK - 1) / BLOCK), dim3(BLOCK), 0,
                       stream.stream(), eg.data_ptr<float>(),
                       lc.data_ptr<float>(), esb.data_ptr<float>(),
                       reinterpret_cast<const long long*>(
                           y.data_ptr<int64_t>()),
                       EG.data_ptr<float>(), delta.data_ptr<float>(),
                       reinterpret_cast<hip_bfloat16*>(eg16.data_ptr()),
                       reinterpret_cast<hip_bfloat16*>(egw.data_ptr()),
                       reinterpret_cast<_Float16*>(delta16.data_ptr()),
                       H);
    C10_HIP_CHECK(hipGetLastError());
}

std::vector<torch::Tensor> table_commit_row(
        torch::Tensor dirichlets, torch::Tensor y, torch::Tensor EG,
        torch::Tensor delta, torch::Tensor s_base, torch::Tensor weights,
        torch::Tensor eg16, torch::Tensor egw, torch::Tensor delta16,
        torch::Tensor dall, double update_weight) {
    check_f32_cuda(dirichlets, "dirichlets");
    TORCH_CHECK(y.scalar_type() == torch::kInt64 && y.numel() == 1);
    TORCH_CHECK(EG.is_contiguous() && delta.is_contiguous()
                && s_base.is_contiguous() && weights.is_contiguous()
                && eg16.is_contiguous() && egw.is_contiguous()
                && delta16.is_contiguous() && dall.is_contiguous(),
                "table tensors must be contiguous");
    const int H = dirichlets.size(0), C = dirichlets.size(1);
    auto a_col = torch::empty({H}, dirichlets.options());
    auto b_col = torch::empty({H}, dirichlets.options());
    auto stream = c10::hip::getCurrentHIPStream();
    hipLaunchKernelGGL(trc_cols_kernel, dim3(H), dim3(BLOCK), 0,
                       stream.stream(), dirichlets.data_ptr<float>(),
                       reinterpret_cast<const long long*>(y.data_ptr<int64_t>()), a_col.data_ptr<float>(),
                       b_col.data_ptr<float>(), H, C);
    auto eglc = beta_row_tables(a_col, b_col, update_weight);
    commit_row_launch(eglc[0], eglc[1], y, EG, delta, s_base, weights,
                      eg16, egw, delta16, dall, H);
    return {a_col, b_col};
}

// eager-path variant: caller already has the class column (the
// distributed ranks' table refresh); y is a host int.
void table_commit_cols(torch::Tensor a_col, torch::Tensor b_col,
                       int64_t y, torch::Tensor EG, torch::Tensor delta,
                       torch::Tensor s_base, torch::Tensor weights,
                       torch::Tensor eg16, torch::Tensor egw,
                       torch::Tensor delta16, torch::Tensor dall,
                       double update_weight) {
    check_f32_cuda(a_col, "a_col");
    check_f32_cuda(b_col, "b_col");
    const int H = a_col.size(0);
    auto y_t = torch::full({1}, y,
                           a_col.options().dtype(torch::kInt64));
    auto eglc = beta_row_tables(a_col, b_col, update_weight);
    commit_row_launch(eglc[0], eglc[1], y_t, EG, delta, s_base, weights,
                      eg16, egw, delta16, dall, H);
}

torch::Tensor pi_hat_delta(torch::Tensor preds, torch::Tensor cls) {
    TORCH_CHECK(preds.is_cuda() && preds.is_contiguous(),
                "preds must be contiguous on a ROCm device");
    TORCH_CHECK(cls.scalar_type() == torch::kInt32, "cls must be int32");
    const int H = preds.size(0), C = preds.size(2);
    const long long N = preds.size(1);
    auto out = torch::empty({N}, preds.options().dtype(torch::kFloat32));
    const int blocks = (int)((N + BLOCK - 1) / BLOCK);
    auto stream = c10::hip::getCurrentHIPStream();
    if (preds.scalar_type() == torch::kFloat32) {
        hipLaunchKernelGGL(pi_hat_delta_kernel<float>, dim3(blocks),
                           dim3(BLOCK), 0, stream.stream(),
                           preds.data_ptr<float>(), cls.data_ptr<int>(),
                           out.data_ptr<float>(), H, N, C);
    } else if (preds.scalar_type() == torch::kBFloat16) {
        hipLaunchKernelGGL(pi_hat_delta_kernel<hip_bfloat16>, dim3(blocks),
                           dim3(BLOCK), 0, stream.stream(),
                           reinterpret_cast<const hip_bfloat16*>(
                               preds.data_ptr()),
                           cls.data_ptr<int>(), out.data_ptr<float>(),
                           H, N, C);
    } else if (preds.scalar_type() == torch::kFloat16) {
        hipLaunchKernelGGL(pi_hat_delta_kernel<_Float16>, dim3(blocks),
                           dim3(BLOCK), 0, stream.stream(),
                           reinterpret_cast<const _Float16*>(
                               preds.data_ptr()),
                           cls.data_ptr<int>(), out.data_ptr<float>(),
                           H, N, C);
    } else if (preds.scalar_type() == torch::kFloat8_e4m3fn) {
        hipLaunchKernelGGL(pi_hat_delta_kernel<__hip_fp8_e4m3>,
                           dim3(blocks), dim3(BLOCK), 0, stream.stream(),
                           reinterpret_cast<const __hip_fp8_e4m3*>(
                               preds.data_ptr()),
                           cls.data_ptr<int>(), out.data_ptr<float>(),
                           H, N, C);
    } else {
        TORCH_CHECK(false,
                    "pi_hat_delta kernel supports fp32/fp16/bf16/fp8");
    }
    C10_HIP_CHECK(hipGetLastError());
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
    auto stream = c10::hip::getCurrentHIPStream();
    if (preds.scalar_type() == torch::kFloat32) {
        hipLaunchKernelGGL(pi_hat_delta_part_kernel<float>, dim3(bx, KH),
                           dim3(BLOCK), 0, stream.stream(),
                           preds.data_ptr<float>(), cls.data_ptr<int>(),
                           partial.data_ptr<float>(), H, N, C, Hc);
    } else if (preds.scalar_type() == torch::kBFloat16) {
        hipLaunchKernelGGL(pi_hat_delta_part_kernel<hip_bfloat16>,
                           dim3(bx, KH), dim3(BLOCK), 0, stream.stream(),
                           reinterpret_cast<const hip_bfloat16*>(
                               preds.data_ptr()),
                           cls.data_ptr<int>(), partial.data_ptr<float>(),
                           H, N, C, Hc);
    } else if (preds.scalar_type() == torch::kFloat16) {
        hipLaunchKernelGGL(pi_hat_delta_part_kernel<_Float16>,
                           dim3(bx, KH), dim3(BLOCK), 0, stream.stream(),
                           reinterpret_cast<const _Float16*>(
                               preds.data_ptr()),
                           cls.data_ptr<int>(), partial.data_ptr<float>(),
                           H, N, C, Hc);
    } else if (preds.scalar_type() == torch::kFloat8_e4m3fn) {
        hipLaunchKernelGGL(pi_hat_delta_part_kernel<__hip_fp8_e4m3>,
                           dim3(bx, KH), dim3(BLOCK), 0, stream.stream(),
                           reinterpret_cast<const __hip_fp8_e4m3*>(
                               preds.data_ptr()),
                           cls.data_ptr<int>(), partial.data_ptr<float>(),
                           H, N, C, Hc);
    } else {
        TORCH_CHECK(false,
                    "pi_hat_delta kernel supports fp32/fp16/bf16/fp8");
    }
    C10_HIP_CHECK(hipGetLastError());
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
    auto stream = c10::hip::getCurrentHIPStream();
    if (preds_t.scalar_type() == torch::kFloat32) {
        hipLaunchKernelGGL(pi_hat_delta_t_part_kernel<float>,
                           dim3(bx, KH), dim3(BLOCK), 0, stream.stream(),
                           preds_t.data_ptr<float>(), cls.data_ptr<int>(),
                           partial.data_ptr<float>(), H, N, C, Hc);
    } else if (preds_t.scalar_type() == torch::kBFloat16) {
        hipLaunchKernelGGL(pi_hat_delta_t_part_kernel<hip_bfloat16>,
                           dim3(bx, KH), dim3(BLOCK), 0, stream.stream(),
                           reinterpret_cast<const hip_bfloat16*>(
                               preds_t.data_ptr()),
                           cls.data_ptr<int>(), partial.data_ptr<float>(),
                           H, N, C, Hc);
    } else if (preds_t.scalar_type() == torch::kFloat16) {
        hipLaunchKernelGGL(pi_hat_delta_t_part_kernel<_Float16>,
                           dim3(bx, KH), dim3(BLOCK), 0, stream.stream(),
                           reinterpret_cast<const _Float16*>(
                               preds_t.data_ptr()),
                           cls.data_ptr<int>(), partial.data_ptr<float>(),
                           H, N, C, Hc);
    } else if (preds_t.scalar_type() == torch::kFloat8_e4m3fn) {
        hipLaunchKernelGGL(pi_hat_delta_t_part_kernel<__hip_fp8_e4m3>,
                           dim3(bx, KH), dim3(BLOCK), 0, stream.stream(),
                           reinterpret_cast<const __hip_fp8_e4m3*>(
                               preds_t.data_ptr()),
                           cls.data_ptr<int>(), partial.data_ptr<float>(),
                           H, N, C, Hc);
    } else {
        TORCH_CHECK(false,
                    "pi_hat_delta kernel supports fp32/fp16/bf16/fp8");
    }
    C10_HIP_CHECK(hipGetLastError());
    return partial;
}


void dirichlet_add(torch::Tensor dir, torch::Tensor y, torch::Tensor cls,
                   double lr) {
    check_f32_cuda(dir, "dirichlets");
    TORCH_CHECK(y.scalar_type() == torch::kInt64 && y.numel() == 1, "y");
    TORCH_CHECK(cls.scalar_type() == torch::kInt64, "cls");
    const int H = dir.size(0), C = dir.size(1);
    const int blocks = (H + BLOCK - 1) / BLOCK;
    auto stream = c10::hip::getCurrentHIPStream();
    hipLaunchKernelGGL(dirichlet_add_kernel, dim3(blocks), dim3(BLOCK), 0,
                       stream.stream(), dir.data_ptr<float>(),
                       y.data_ptr<long>(), cls.data_ptr<long>(),
                       (float)lr, H, C);
    C10_HIP_CHECK(hipGetLastError());
}

void col_add(torch::Tensor adjusted, torch::Tensor row_sums,
             torch::Tensor y, torch::Tensor delta) {
    check_f32_cuda(adjusted, "adjusted");
    check_f32_cuda(row_sums, "row_sums");
    check_f32_cuda(delta, "delta");
    TORCH_CHECK(y.scalar_type() == torch::kInt64 && y.numel() == 1, "y");
    const long long N = adjusted.size(0);
    const int C = adjusted.size(1);
    const int blocks = (int)((N + BLOCK - 1) / BLOCK);
    auto stream = c10::hip::getCurrentHIPStream();
    hipLaunchKernelGGL(col_add_kernel, dim3(blocks), dim3(BLOCK), 0,
                       stream.stream(), adjusted.data_ptr<float>(),
                       row_sums.data_ptr<float>(), y.data_ptr<long>(),
                       delta.data_ptr<float>(), N, C);
    C10_HIP_CHECK(hipGetLastError());
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
    auto stream = c10::hip::getCurrentHIPStream();
    hipLaunchKernelGGL(mix_part_kernel, dim3(G), dim3(BLOCK), 0,
                       stream.stream(), rows.data_ptr<float>(),
                       pi.data_ptr<float>(), partial.data_ptr<float>(),
                       C, H);
    hipLaunchKernelGGL(mix_combine_kernel, dim3(1), dim3(BLOCK), 0,
                       stream.stream(), partial.data_ptr<float>(),
                       mixture0.data_ptr<float>(), h0.data_ptr<float>(),
                       G, H);
    C10_HIP_CHECK(hipGetLastError());
    return {mixture0, h0};
}

torch::Tensor pi_marginal(torch::Tensor adjusted, torch::Tensor row_sums) {
    check_f32_cuda(adjusted, "adjusted");
    check_f32_cuda(row_sums, "row_sums");
    const long long N = adjusted.size(0);
    const int C = adjusted.size(1);
    TORCH_CHECK(C <= 8 * BLOCK, "C too large for pi_marginal kernel");
    auto stream = c10::hip::getCurrentHIPStream();
    if ((C & 3) == 0 && C <= 4 * BLOCK) {
        // deterministic two-stage-reduce path (probe: 36 us vs 165 us
        // for the atomic single-kernel at N=50k, C=1000).  G sized so
        // the partial stage keeps ~1024 ACTIVE waves streaming: a block
        // covers ceil(C/4) lanes = awpb active waves.
        const int awpb = (C / 4 + 63) / 64;
        const int G = std::min(1024, std::max(256, 1024 / awpb));
        constexpr int S = 16;  // G-reduce split
        auto out = torch::empty({C}, adjusted.options());
        auto work = torch::empty({G + S, C}, adjusted.options());
        float* partial = work.data_ptr<float>();
        float* part2 = partial + (long long)G * C;
        const int cblocks = (C + 4 * BLOCK - 1) / (4 * BLOCK);
        hipLaunchKernelGGL(pi_marginal_part_kernel, dim3(G), dim3(BLOCK),
                           0, stream.stream(), adjusted.data_ptr<float>(),
                           row_sums.data_ptr<float>(), partial, N, C, C);
        hipLaunchKernelGGL(pi_marginal_reduce_kernel, dim3(cblocks, S),
                           dim3(BLOCK), 0, stream.stream(), partial,
                           part2, G, C, C, C);
        hipLaunchKernelGGL(pi_marginal_reduce_kernel, dim3(cblocks, 1),
                           dim3(BLOCK), 0, stream.stream(), part2,
                           out.data_ptr<float>(), S, C, C, C);
        C10_HIP_CHECK(hipGetLastError());
        return out;
    }
    // every other C: scalar slab partials + the same fixed-order reduce,
    // on columns padded to a multiple of 4
    const int Cpad = (C + 3) & ~3;
    const int G = 1536;  // 6 blocks/CU: enough row-slabs in flight
                         // to cover HBM latency (512 ran at 1 TB/s)
    constexpr int S = 16;
    auto out = torch::empty({Cpad}, adjusted.options());
    auto work = torch::empty({G + S, Cpad}, adjusted.options());
    float* partial = work.data_ptr<float>();
    float* part2 = partial + (long long)G * Cpad;
    const int cblocks = (Cpad + 4 * BLOCK - 1) / (4 * BLOCK);
    hipLaunchKernelGGL(pi_marginal_kernel, dim3(G), dim3(BLOCK), 0,
                       stream.stream(), adjusted.data_ptr<float>(),
                       row_sums.data_ptr<float>(), partial, N, C, Cpad);
    hipLaunchKernelGGL(pi_marginal_reduce_kernel, dim3(cblocks, S),
                       dim3(BLOCK), 0, stream.stream(), partial, part2,
                       G, Cpad, Cpad, Cpad);
    hipLaunchKernelGGL(pi_marginal_reduce_kernel, dim3(cblocks, 1),
                       dim3(BLOCK), 0, stream.stream(), part2,
                       out.data_ptr<float>(), S, Cpad, Cpad, Cpad);
    C10_HIP_CHECK(hipGetLastError());
    return out.narrow(0, 0, C);
}

void register_pair_ops(pybind11::module_& m);  // pair.hip (v3 engine)
void register_ingest_ops(pybind11::module_& m);  // ingest.hip (pool ingest)
void register_ingest_logits_ops(pybind11::module_& m);  // ingest_logits.hip
void register_modelpicker_ops(pybind11::module_& m);  // modelpicker.hip

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
    m.doc() = "coda_amd fused gfx950 kernels";
    register_pair_ops(m);
    register_ingest_ops(m);
    register_ingest_logits_ops(m);
    register_modelpicker_ops(m);
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
    m.def("pi_hat_delta_t_part", &pi_hat_delta_t_part,
          "class-major (H, C, N) rank-1 pi_hat gather partials");
    m.def("pi_hat_delta_part", &pi_hat_delta_part,
          "H-chunked rank-1 pi_hat increment partials (KH, N)");
    m.def("col_add", &col_add,
          "fused adjusted[:, y] += delta; row_sums += delta");
    m.def("dirichlet_add", &dirichlet_add,
          "dir[h, y, cls_h] += lr scatter (the posterior label update)");
    m.def("eig_phase1", &eig_phase1,
          "Sharded hypothetical pass A: slog2 partials (B*C, P)");
    m.def("eig_phase2", &eig_phase2,
          "Sharded hypothetical pass B: unnorm masses + totals");
    m.def("es_build", &es_build,
          "v2: fused slog scatter + exp2 + trapz weights -> ES (C,B,P)");
    m.def("eig_assemble_k", &eig_assemble_k,
          "v2: v-select + normalize + log2-entropy -> H_after (B,C)");
    m.def("es_build_gathered", &es_build_gathered,
          "sharded v2: ES from gathered selected-delta curves");
    m.def("eig_totals", &eig_totals,
          "sharded v2: local normalizer partials (B,C)");
    m.def("eig_entropy", &eig_entropy,
          "sharded v2: entropy partials from globally-reduced totals");
    m.def("beta_row_tables", &beta_row_tables,
          "v2: one class row's H*2 hypothetical curves (EG, log2 cdf)");
    m.def("pi_hat_delta", &pi_hat_delta,
          "rank-1 pi_hat increment: sum_h preds[h, :, cls_h]");
    m.def("mixture_entropy", &mixture_entropy,
          "mixture0 (H,) = sum_c pi[c]*rows[c,h] + fused log2 entropy");
    m.def("table_commit_cols", &table_commit_cols,
          "per-class table refresh from Beta columns (eager path)");
    m.def("table_commit_row", &table_commit_row,
          "per-label class-row table refresh (cols + curves + commits)");
    m.def("pi_marginal", &pi_marginal,
          "pi[c] = sum_n adjusted[n,c]/clamp(rowsum[n]) in one pass");
}
