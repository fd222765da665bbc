// gfx950 kernels of the v2 table engine (coda_amd/ops/table.py) and the
// per-label table-row commit that the v2 and v3 tables share.
//
// Kernel inventory (host bindings at the bottom):
//   es_build[_long]        CSR-bucketed log-cdf scatter + exp2 + trapz
//                          weights -> the GEMM B operand (bf16/f32); the
//                          block-per-row companion takes buckets longer
//                          than ES_LONG_ROW
//   es_build_gathered      the same from gathered selected-delta curves
//                          (sharded v2)
//   eig_assemble_kernel    variant select + normalize + log2 entropy
//   eig_totals/entropy     sharded split around the normalizer all-reduce
//   beta_row_tables_kernel per-class incremental table refresh (shares
//                          LaneGrid, beta_grid.h, with the v1 kernels)
//   trc_cols/sums/rows     per-label class-row commit into the tables

#include "host_util.h"
#include <algorithm>
#include <vector>

#define ES_LONG_ROW 512

namespace {

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

}  // namespace

// ---------------------------------------------------------------------------
// Host bindings
// ---------------------------------------------------------------------------

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
    dispatch_bf16_f32(es, [&](auto* out) {
        const auto run = [&](auto kern, int blocks) {
            launch(kern, dim3(blocks), 0, s_base.data_ptr<float>(),
                   delta.data_ptr<float>(), dall.data_ptr<float>(),
                   hvals.data_ptr<int>(), offsets.data_ptr<int>(),
                   w.data_ptr<float>(), out, B, C, H);
        };
        // 16 sublane rows per block
        run(es_build_kernel<elem_t<decltype(out)>>, (R + 15) / 16);
        if (H > 2 * ES_LONG_ROW)  // long rows only exist at wide pools
            run(es_build_long_kernel<elem_t<decltype(out)>>, R);
    });
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
    dispatch_bf16_f32(m, [&](auto* mp) {
        launch(eig_assemble_kernel<elem_t<decltype(mp)>>,
               dim3(row_blocks(B * C)), 0, mp, cls.data_ptr<int>(),
               pi_hat.data_ptr<float>(), pbest_before.data_ptr<float>(),
               mixture0.data_ptr<float>(), h_after.data_ptr<float>(),
               B, C, H);
    });
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
    dispatch_bf16_f32(es, [&](auto* out) {
        launch(es_build_gathered_kernel<elem_t<decltype(out)>>,
               dim3(row_blocks(B * C)), 0, s_base_all.data_ptr<float>(),
               sel_all.data_ptr<float>(), hvals.data_ptr<int>(),
               offsets.data_ptr<int>(), w.data_ptr<float>(), out,
               B, C, Hg);
    });
    return es;
}

torch::Tensor eig_totals(torch::Tensor m, torch::Tensor cls) {
    TORCH_CHECK(m.is_cuda() && m.is_contiguous(), "m");
    check_cls_for_m(m, cls);
    const int C = m.size(0), B = m.size(1), H = m.size(2) / 2;
    auto totals = torch::empty({B, C},
                               m.options().dtype(torch::kFloat32));
    dispatch_bf16_f32(m, [&](auto* mp) {
        launch(eig_totals_kernel<elem_t<decltype(mp)>>,
               dim3(row_blocks(B * C)), 0, mp, cls.data_ptr<int>(),
               totals.data_ptr<float>(), B, C, H);
    });
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
    dispatch_bf16_f32(m, [&](auto* mp) {
        launch(eig_entropy_kernel<elem_t<decltype(mp)>>,
               dim3(row_blocks(B * C)), 0, mp, cls.data_ptr<int>(),
               totals.data_ptr<float>(), pi_hat.data_ptr<float>(),
               pbest_before.data_ptr<float>(), mixture0.data_ptr<float>(),
               h_after.data_ptr<float>(), B, C, H);
    });
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
    launch(beta_row_tables_kernel, dim3(row_blocks(2 * H)), 0,
           alpha_col.data_ptr<float>(), beta_col.data_ptr<float>(),
           eg.data_ptr<float>(), lc.data_ptr<float>(),
           (float)update_weight, H);
    return {eg, lc};
}


static const long long* y_ptr(const torch::Tensor& y) {
    return reinterpret_cast<const long long*>(y.data_ptr<int64_t>());
}

static void commit_row_launch(torch::Tensor& eg, torch::Tensor& lc,
                              torch::Tensor& y, torch::Tensor& EG,
                              torch::Tensor& delta, torch::Tensor& s_base,
                              torch::Tensor& weights, torch::Tensor& eg16,
                              torch::Tensor& egw, torch::Tensor& delta16,
                              torch::Tensor& dall, int H) {
    auto esb = torch::empty({P_POINTS}, eg.options());
    launch(trc_sums_kernel, dim3(1), 0,  // BLOCK == P_POINTS threads
           lc.data_ptr<float>(), weights.data_ptr<float>(), y_ptr(y),
           s_base.data_ptr<float>(), dall.data_ptr<float>(),
           esb.data_ptr<float>(), H);
    const int total = 2 * H * P_POINTS;
    launch(trc_rows_kernel, dim3((total + BLOCK - 1) / BLOCK), 0,
           eg.data_ptr<float>(), lc.data_ptr<float>(),
           esb.data_ptr<float>(), y_ptr(y), EG.data_ptr<float>(),
           delta.data_ptr<float>(),
           reinterpret_cast<hip_bfloat16*>(eg16.data_ptr()),
           reinterpret_cast<hip_bfloat16*>(egw.data_ptr()),
           reinterpret_cast<_Float16*>(delta16.data_ptr()), H);
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
    launch(trc_cols_kernel, dim3(H), 0, dirichlets.data_ptr<float>(),
           y_ptr(y), a_col.data_ptr<float>(), b_col.data_ptr<float>(),
           H, C);
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

void register_table_ops(pybind11::module_& m) {
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
    m.def("table_commit_cols", &table_commit_cols,
          "per-class table refresh from Beta columns (eager path)");
    m.def("table_commit_row", &table_commit_row,
          "per-label class-row table refresh (cols + curves + commits)");
}
