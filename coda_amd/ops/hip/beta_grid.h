// The Beta-grid geometry that the v1 P(best)/EIG kernels (pbest.hip) and
// the v2 table refresh (table.hip, beta_row_tables_kernel) share: the
// P = 256 point grid, the wave-per-row block shape, the reference's clamp
// ladder, and the per-lane grid state. label.hip takes the block shape
// only.
#pragma once

#include <hip/hip_runtime.h>
#include "wave.h"

#define P_POINTS 256
#define BLOCK 256          // workgroup = 4 waves
#define ROWS_PER_BLOCK 4   // one wave per row
#define PTS_PER_LANE 4     // P = 64 lanes x 4 points

// The tuned kernels carry __launch_bounds__(BLOCK, 4): 4 waves/SIMD. It
// forces the register allocator toward higher occupancy; the wave-per-row
// kernels are latency-bound and intentionally spill ~50 VGPRs for it.
// Measured on MI355X with the DPP wave scan: 1.86x the untuned kernel
// (82.9 -> 44.6 ns/row on the fused EIG kernel at H=128, C=1000;
// profiles/README.md has the sweep).

constexpr double kGridLo = 1e-6;
constexpr double kGridHi = 1.0 - 1e-6;
constexpr float kEps = 1e-30f;                    // cdf / normalizer clamp
constexpr float kLog2Clamp = 115.41560327111707f; // the reference's +-80
                                                  // natural-log clamp, base 2

// Per-lane grid state: base-2 logs of this lane's 4 grid points,
// delta-centered.
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
