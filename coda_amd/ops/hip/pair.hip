// v3 pair-factored EIG kernels for gfx950 (see coda_amd/ops/pair.py for
// the math and the sparsity argument; reference semantics:
// coda/coda.py:150-168 + :235-281 restricted to hit cells).
//
// Three kernels per acquisition step, covering the WHOLE candidate pool:
//
//   pair_dsum_es_kernel    one wave per (candidate, class) hit pair:
//                          sums the pair's selected log2-cdf delta
//                          curves (fp16 table - traffic-bound) and
//                          exponentiates -> the bf16 MFMA A operand
//                          (K, P). The baseline curve exp2(s_base)*w is
//                          folded into the B operand (egw).
//
//   pair_gemm_entropy{16,128}_kernel
//                          one workgroup per class-uniform pair tile
//                          (or group of same-class tiles): bf16 MFMA
//                          (tile x 2H x P) pairing GEMM with the
//                          variant-select + normalize + log2 entropy
//                          epilogue fused (the (K, 2H) M tensor never
//                          reaches global memory). The 128-pair
//                          variant (2H <= 272, i.e. H <= 136) keeps the
//                          class's whole B operand resident in LDS,
//                          dividing the dominant B traffic by 8 vs the
//                          16-pair tile; the 16-pair variant covers H
//                          up to 1024. 128-pair tiles with 2H > 272
//                          take the split wide pipeline below (M
//                          written to global as bf16, H <= 2048).
//
//   pair_eig_finalize_kernel
//                          one wave per candidate: EIG[b] = H_before -
//                          (pi_xi row) . h_base - sum over the
//                          candidate's hit pairs of pi_xi*(h_after -
//                          h_base), in a fixed lane-strided order
//                          (deterministic - no atomics).
//
// Pair cache (fused 128-pair route with a static structure): a label
// rewrites ONE class's table rows, and everything up to a pair's
// selected pairing masses and their normalizer depends only on its own
// class's rows. pair_gemm_pbn128_kernel keeps those in a persistent
// (K, H) fp32 cache; per step pair_dsum_es_cls_kernel +
// pair_gemm_pbn128_kernel refresh the labelled class's run of pairs and
// pair_entropy_cached_kernel streams the cache into h_after, replacing
// the full dsum + GEMM over all K pairs with bit-identical results.
//
// MFMA: v_mfma_f32_16x16x32_bf16. Lane mapping (cdna_hip_programming.md
// section 3): A[i][k] i=lane&15, k=(lane>>4)*8+e; B[k][j] j=lane&15,
// same k; C/D col=lane&15, row=(lane>>4)*4+reg. The B operand is stored
// row-major (j, p) = egw (C, 2H, P) so both fragments load 16
// contiguous bytes per lane. Layout verified by the mfma_probe test
// (tests/test_gpu.py).

#include <algorithm>
#include <climits>
#include <initializer_list>
#include <torch/extension.h>
#include <hip/hip_runtime.h>
#include <c10/hip/HIPStream.h>
#include <hip/hip_bfloat16.h>
#include "wave.h"  // wave_reduce_sum, row16_reduce

#define P_POINTS 256
#define BLOCK 256

namespace pairops {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef _Float16 half4v __attribute__((ext_vector_type(4)));

// ---------------------------------------------------------------------
// A-operand build: a16[k, p] = 2^(sum_{h in seg(k)} delta16[c_k, h, p])
// ---------------------------------------------------------------------
// One pair's row, by the 16 lanes that own it: pair k of the structure,
// written to a16 row `arow` (k itself for the full operand, k minus the
// class's run start for the one-class scratch operand).
__device__ __forceinline__ void
dsum_es_row(const _Float16* __restrict__ delta16,  // (C, H, P)
            const float* __restrict__ dall,        // (C, P)
            const int* __restrict__ pair_c,        // (K,)
            const int* __restrict__ pair_neg,      // (K,)
            const int* __restrict__ seg_off,       // (K+1,)
            const int* __restrict__ seg_h,         // (S,)
            hip_bfloat16* __restrict__ a16,
            int k, int arow, int H) {
    // 16 lanes per pair (the hit distribution is singleton-heavy:
    // avg segment ~2 models - a wave per pair would mostly idle on one
    // 512-B load). Each lane owns 16 grid points as 4x half4v loads.
    const int sublane = threadIdx.x & 15;
    const int p0 = sublane * 16;
    const int c = pair_c[k];
    const int s0 = seg_off[k], s1 = seg_off[k + 1];
    const size_t dbase = (size_t)c * H * P_POINTS + p0;

    float acc[16] = {};
    float acc2[16] = {};
    int s = s0;
    // 2-row software pipeline: the single-row loop is a dependent
    // seg_h -> 4-load -> FMA chain (the table lives in the LLC, so
    // this kernel is latency-bound, not HBM-bound); two rows with
    // split accumulators keep 8 loads in flight per lane (a 4-row
    // variant measured the same)
    for (; s + 1 < s1; s += 2) {
        const _Float16* ra = delta16 + dbase
            + (size_t)seg_h[s] * P_POINTS;
        const _Float16* rb = delta16 + dbase
            + (size_t)seg_h[s + 1] * P_POINTS;
        const half4v a0 = *reinterpret_cast<const half4v*>(ra);
        const half4v a1 = *reinterpret_cast<const half4v*>(ra + 4);
        const half4v a2 = *reinterpret_cast<const half4v*>(ra + 8);
        const half4v a3 = *reinterpret_cast<const half4v*>(ra + 12);
        const half4v b0 = *reinterpret_cast<const half4v*>(rb);
        const half4v b1 = *reinterpret_cast<const half4v*>(rb + 4);
        const half4v b2 = *reinterpret_cast<const half4v*>(rb + 8);
        const half4v b3 = *reinterpret_cast<const half4v*>(rb + 12);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            acc[j] += (float)a0[j];      acc2[j] += (float)b0[j];
            acc[4 + j] += (float)a1[j];  acc2[4 + j] += (float)b1[j];
            acc[8 + j] += (float)a2[j];  acc2[8 + j] += (float)b2[j];
            acc[12 + j] += (float)a3[j]; acc2[12 + j] += (float)b3[j];
        }
    }
    if (s < s1) {
        const _Float16* row = delta16 + dbase + (size_t)seg_h[s] * P_POINTS;
        const half4v d0 = *reinterpret_cast<const half4v*>(row);
        const half4v d1 = *reinterpret_cast<const half4v*>(row + 4);
        const half4v d2 = *reinterpret_cast<const half4v*>(row + 8);
        const half4v d3 = *reinterpret_cast<const half4v*>(row + 12);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            acc[j] += (float)d0[j];
            acc[4 + j] += (float)d1[j];
            acc[8 + j] += (float)d2[j];
            acc[12 + j] += (float)d3[j];
        }
    }
#pragma unroll
    for (int j = 0; j < 16; ++j) acc[j] += acc2[j];
    if (pair_neg[k]) {
        // complement segment: dsum = (sum over ALL models) - partial
        const float4* da = reinterpret_cast<const float4*>(
            dall + (size_t)c * P_POINTS + p0);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const float4 d = da[q];
            acc[4 * q] = d.x - acc[4 * q];
            acc[4 * q + 1] = d.y - acc[4 * q + 1];
            acc[4 * q + 2] = d.z - acc[4 * q + 2];
            acc[4 * q + 3] = d.w - acc[4 * q + 3];
        }
    }
    ushort4 out[4];
    unsigned short* o = reinterpret_cast<unsigned short*>(out);
#pragma unroll
    for (int j = 0; j < 16; ++j)
        o[j] = hip_bfloat16(exp2f(acc[j])).data;
    ushort4* dst = reinterpret_cast<ushort4*>(
        a16 + (size_t)arow * P_POINTS + p0);
    dst[0] = out[0]; dst[1] = out[1]; dst[2] = out[2]; dst[3] = out[3];
}

__global__ void __launch_bounds__(BLOCK)
pair_dsum_es_kernel(const _Float16* __restrict__ delta16,  // (C, H, P)
                    const float* __restrict__ dall,        // (C, P)
                    const int* __restrict__ pair_c,        // (K,)
                    const int* __restrict__ pair_neg,      // (K,)
                    const int* __restrict__ seg_off,       // (K+1,)
                    const int* __restrict__ seg_h,         // (S,)
                    hip_bfloat16* __restrict__ a16,        // (K, P)
                    int K, int H) {
    const int k = blockIdx.x * 16 + (threadIdx.x >> 4);
    if (k >= K) return;
    dsum_es_row(delta16, dall, pair_c, pair_neg, seg_off, seg_h, a16,
                k, k, H);
}

// One class's run of pairs [run_off[y], run_off[y+1]) with the class id
// read on the device (the label graph's y_t), into the (max_run, P)
// scratch operand indexed from the run start. The grid covers the
// longest run of any class; the rest return.
__global__ void __launch_bounds__(BLOCK)
pair_dsum_es_cls_kernel(const _Float16* __restrict__ delta16,
                        const float* __restrict__ dall,
                        const int* __restrict__ pair_c,
                        const int* __restrict__ pair_neg,
                        const int* __restrict__ seg_off,
                        const int* __restrict__ seg_h,
                        const int* __restrict__ run_off,    // (C+1,)
                        const long long* __restrict__ y_t,  // (1,)
                        hip_bfloat16* __restrict__ a_run,   // (max_run, P)
                        int max_run, int C, int H) {
    const long long y = y_t[0];
    if (y < 0 || y >= C) return;
    const int rel = blockIdx.x * 16 + (threadIdx.x >> 4);
    const int k = run_off[y] + rel;
    if (rel >= max_run || k >= run_off[y + 1]) return;
    dsum_es_row(delta16, dall, pair_c, pair_neg, seg_off, seg_h, a_run,
                k, rel, H);
}

// ---------------------------------------------------------------------
// 16-pair tile GEMM+entropy (any H <= 1024): B streamed from L2.
// ---------------------------------------------------------------------
__global__ void __launch_bounds__(BLOCK)
pair_gemm_entropy16_kernel(const hip_bfloat16* __restrict__ a16,
                           const hip_bfloat16* __restrict__ egw,
                           const unsigned* __restrict__ vmask,
                           const int* __restrict__ pair_c,
                           int W,
                           const float* __restrict__ pi_hat,
                           const float* __restrict__ pbest_before,
                           const float* __restrict__ mixture0,
                           float* __restrict__ h_after,
                           int H, int mstride) {
    extern __shared__ char smem[];
    hip_bfloat16* a_lds = reinterpret_cast<hip_bfloat16*>(smem);
    float* m_tile = reinterpret_cast<float*>(
        smem + 16 * P_POINTS * sizeof(hip_bfloat16));

    const int k0 = blockIdx.x * 16;
    const int c = pair_c[k0];
    const int tid = threadIdx.x;
    const int wave = tid >> 6, lane = tid & 63;
    const int row16 = lane & 15;
    const int kgrp = lane >> 4;

    {   // stage A tile: 16 rows x 256 bf16 = 8 KB
        const uint4* g = reinterpret_cast<const uint4*>(
            a16 + (size_t)k0 * P_POINTS);
        uint4* d = reinterpret_cast<uint4*>(a_lds);
        d[tid] = g[tid];
        d[tid + BLOCK] = g[tid + BLOCK];
    }
    __syncthreads();

    const int twoH = 2 * H;
    const int JT = (twoH + 15) / 16;
    for (int jt = wave; jt < JT; jt += 4) {
        const int j = jt * 16 + row16;
        const bool jvalid = j < twoH;
        const hip_bfloat16* brow =
            egw + ((size_t)c * twoH + (jvalid ? j : 0)) * P_POINTS;
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int kk = 0; kk < P_POINTS; kk += 32) {
            const bf16x8 afrag = *reinterpret_cast<const bf16x8*>(
                a_lds + row16 * P_POINTS + kk + kgrp * 8);
            bf16x8 bfrag = {};
            if (jvalid)
                bfrag = *reinterpret_cast<const bf16x8*>(
                    brow + kk + kgrp * 8);
            acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                afrag, bfrag, acc, 0, 0, 0);
        }
        if (jvalid) {
#pragma unroll
            for (int r = 0; r < 4; ++r)
                m_tile[(kgrp * 4 + r) * mstride + j] = acc[r];
        }
    }
    __syncthreads();

    for (int pi = wave; pi < 16; pi += 4) {
        const int k = k0 + pi;
        const unsigned* vm = vmask + (size_t)k * W;
        const float* mrow = m_tile + (size_t)pi * mstride;
        float tot = 0.f;
        for (int h = lane; h < H; h += 64) {
            const int v = (vm[h >> 5] >> (h & 31)) & 1;
            tot += mrow[2 * h + v];
        }
        tot = wave_reduce_sum(tot);
        const float inv = 1.0f / fmaxf(tot, 1e-30f);
        const float pic = pi_hat[c];
        float ent = 0.f;
        for (int h = lane; h < H; h += 64) {
            const int v = (vm[h >> 5] >> (h & 31)) & 1;
            const float pb = mrow[2 * h + v] * inv;
            const float mm = fmaxf(
                mixture0[h] + pic * (pb - pbest_before[(size_t)c * H + h]),
                1e-12f);
            ent += -mm * __log2f(mm);
        }
        ent = wave_reduce_sum(ent);
        if (lane == 0) h_after[k] = ent;
    }
}

// ---------------------------------------------------------------------
// 128-pair B-resident tile GEMM+entropy (2H <= 272): the tile's whole
// egw[c] table (2H x P bf16) is staged into LDS ONCE with a coalesced
// row-major copy (stride 264 elems - a 16-B-aligned row start is
// required for the b128 fragment loads; an odd-word "bank-ideal"
// stride measurably loses more to misalignment than it wins back in
// conflicts), then 8 waves run the whole K loop against it
// barrier-free with the A operand streamed from L2. The epilogue is REGISTER-RESIDENT: each lane holds
// pairs kgrp*4+r at columns jt*16+row16, the static vmask selects the
// v variant per (pair, h) (the mask word index (8*jt)>>5 is
// compile-time), and 16-lane DPP row reductions produce tot/entropy -
// the (128, 2H) M tile never exists in LDS or HBM.
// ---------------------------------------------------------------------
#define BSTRIDE 272  // B row stride in halfs: 136 words, 8-word aligned (132
                     // put odd-row b128 reads at =4 mod 8 words: +60
                     // stall cycles each on CDNA4)
#define BLOCK2 512

// One selected column's entropy term, added to the lane's running sum:
// pb = m * inv (the pair's normalized P(best) for model h), mm =
// max(mix + pic * (pb - pbb), 1e-12), ent - mm * log2(mm). The fused
// epilogue and the cached pass below both inline THIS function, so the
// compiler contracts it the same way in both (as it always has in the
// fused kernel: fma(m, inv, -pbb), fma(pic, ., mix), fma(-mm, log2 mm,
// ent) - pb is never rounded on its own, which is why the cache keeps m
// and inv apart). tests/test_pair_cache_gpu.py holds the two kernels to
// bit equality.
__device__ __forceinline__ void pair_ent_acc(float& ent, float mix,
                                             float pic, float m,
                                             float inv, float pbb) {
    const float pb = m * inv;
    const float mm = fmaxf(mix + pic * (pb - pbb), 1e-12f);
    ent += -mm * __log2f(mm);
}

template <int JT>
__global__ void __launch_bounds__(BLOCK2)
pair_gemm_entropy128_kernel(const hip_bfloat16* __restrict__ a16,
                            const hip_bfloat16* __restrict__ egw,
                            const unsigned* __restrict__ vmask,
                            const int* __restrict__ pair_c,
                            int W,
                            const float* __restrict__ pi_hat,
                            const float* __restrict__ pbest_before,
                            const float* __restrict__ mixture0,
                            float* __restrict__ h_after,
                            const int* __restrict__ grp_off,
                            int H, int mstride) {
    extern __shared__ char smem[];
    const int twoH = 2 * H;
    hip_bfloat16* b_lds = reinterpret_cast<hip_bfloat16*>(smem);

    // block owns tiles [t0, t1) - all the same class, so the 131 KB
    // B stage amortizes over up to GRP_MAX tiles (classes average
    // ~2.4 tiles at the headline hit distribution; B staging was
    // ~60% of this kernel's global traffic)
    const int t0 = grp_off[blockIdx.x], t1 = grp_off[blockIdx.x + 1];
    const int c = pair_c[t0 * 128];
    const int tid = threadIdx.x;
    const int wave = tid >> 6, lane = tid & 63;
    const int row16 = lane & 15;
    const int kgrp = lane >> 4;
    const hip_bfloat16* egw_c = egw + (size_t)c * twoH * P_POINTS;

    // stage the whole B table: row j (512 B) split in 2 halves; thread
    // t copies half (t&1) of row (t>>1) - fully coalesced 16-B loads
    for (int t = tid; t < 2 * twoH; t += BLOCK2) {
        const int j = t >> 1, half = t & 1;
        const uint4* g = reinterpret_cast<const uint4*>(
            egw_c + (size_t)j * P_POINTS + half * 128);
        uint4* d = reinterpret_cast<uint4*>(
            reinterpret_cast<char*>(b_lds)
            + (size_t)j * BSTRIDE * 2 + half * 256);
#pragma unroll
        for (int i = 0; i < 16; ++i) d[i] = g[i];
    }
    __syncthreads();

    for (int tile = t0; tile < t1; ++tile) {
    const int k0 = tile * 128;
    f32x4 acc[JT];
#pragma unroll
    for (int jt = 0; jt < JT; ++jt) acc[jt] = {0.f, 0.f, 0.f, 0.f};

    const hip_bfloat16* arow =
        a16 + (size_t)(k0 + wave * 16 + row16) * P_POINTS;
#pragma unroll
    for (int kk = 0; kk < P_POINTS; kk += 32) {
        const bf16x8 afrag = *reinterpret_cast<const bf16x8*>(
            arow + kk + kgrp * 8);
#pragma unroll
        for (int jt = 0; jt < JT; ++jt) {
            const int j = jt * 16 + row16;
            bf16x8 bfrag = {};
            if (j < twoH)
                bfrag = *reinterpret_cast<const bf16x8*>(
                    b_lds + (size_t)j * BSTRIDE + kk + kgrp * 8);
            acc[jt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                afrag, bfrag, acc[jt], 0, 0, 0);
        }
    }

    // register-resident epilogue: lane owns pairs kbase..kbase+3 (the
    // accumulator rows) at columns jt*16+row16. For column j: h = j>>1
    // and it contributes to pair r iff vmask bit h == (j&1).
    const int kbase = k0 + wave * 16 + kgrp * 4;
    unsigned vmw[4][(JT + 3) / 4];
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int w = 0; w < (JT + 3) / 4; ++w)
            vmw[r][w] = (w < W)
                ? vmask[(size_t)(kbase + r) * W + w] : 0u;

    float tot[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int jt = 0; jt < JT; ++jt) {
        const int j = jt * 16 + row16;
        if (j >= twoH) continue;
        const int h = j >> 1, v = j & 1;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int bit = (vmw[r][jt >> 2] >> (h & 31)) & 1;
            if (bit == v) tot[r] += acc[jt][r];
        }
    }
    float inv[4];
#pragma unroll
    for (int r = 0; r < 4; ++r)
        inv[r] = 1.0f / fmaxf(row16_reduce(tot[r]), 1e-30f);

    const float pic = pi_hat[c];
    float ent[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int jt = 0; jt < JT; ++jt) {
        const int j = jt * 16 + row16;
        if (j >= twoH) continue;
        const int h = j >> 1, v = j & 1;
        const float mix = mixture0[h];
        const float pbb = pbest_before[(size_t)c * H + h];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int bit = (vmw[r][jt >> 2] >> (h & 31)) & 1;
            if (bit == v)
                pair_ent_acc(ent[r], mix, pic, acc[jt][r], inv[r], pbb);
        }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const float e = row16_reduce(ent[r]);
        if (row16 == 0) h_after[kbase + r] = e;
    }
    }  // tile loop
    (void)mstride;
}


// Pair-cache build/refresh: pair_gemm_entropy128_kernel's B stage, MFMA
// loop, vmask select and tot reduction, with the entropy epilogue
// replaced by a store of what depends only on the class's own table
// rows - the selected accumulators pm[k, h] and the pair's inv[k] - to
// the persistent cache; pair_entropy_cached_kernel finishes from them.
// (A sibling, not a shared inlined body: wrapping the fused kernel's
// body in a device function changed its code generation - 24 more
// VGPRs and a spill at JT = 17.)
// y_t == nullptr: block b takes group b (the one-off full build over
// the full (K, P) operand). Otherwise the class id is read on the
// device and block b takes ONE tile: tile b % 4 of group
// cls_grp_off[y] + b / 4 (a group holds at most 4 tiles; a tile's
// results do not depend on the grouping, and a refresh has one class's
// few tiles to spread over the chip, where a block per group ran them
// back to back behind one B stage), reading the one-class scratch
// operand, whose row 0 is structure row run_off[y]; the grid is 4x the
// largest group count of any class, and a block past the class's groups
// or past its group's tiles returns - the whole block takes that
// branch, before the first __syncthreads(). Class y's groups cover rows
// [run_off[y], run_off[y+1]) exactly, so a refresh writes those cache
// rows and no others.
#define PBN_GRP_TILES 4   // most tiles of a group: coda_amd/ops/pair.py
                          // GRP_MAX (tests/test_pair_stream.py ties them)

template <int JT>
__global__ void __launch_bounds__(BLOCK2)
pair_gemm_pbn128_kernel(const hip_bfloat16* __restrict__ a16,
                        const hip_bfloat16* __restrict__ egw,
                        const unsigned* __restrict__ vmask,
                        const int* __restrict__ pair_c,
                        int W,
                        const int* __restrict__ grp_off,      // (G+1,)
                        const int* __restrict__ cls_grp_off,  // (C+1,)
                        const int* __restrict__ run_off,      // (C+1,)
                        const long long* __restrict__ y_t,    // (1,)
                        float* __restrict__ pm,               // (K, H)
                        float* __restrict__ pinv,             // (K,)
                        int C, int H) {
    int g = blockIdx.x, a_row0 = 0, tsel = -1;
    if (y_t != nullptr) {
        const long long y = y_t[0];
        if (y < 0 || y >= C) return;
        g = cls_grp_off[y] + (int)(blockIdx.x / PBN_GRP_TILES);
        if (g >= cls_grp_off[y + 1]) return;
        tsel = (int)(blockIdx.x % PBN_GRP_TILES);
        a_row0 = run_off[y];
    }
    extern __shared__ char smem[];
    const int twoH = 2 * H;
    hip_bfloat16* b_lds = reinterpret_cast<hip_bfloat16*>(smem);

    int t0 = grp_off[g];
    const int t1 = grp_off[g + 1];
    int tstep = 1;
    if (tsel >= 0) {
        // one-class refresh: this block's tile of the group (and every
        // PBN_GRP_TILES-th after it, should a group ever hold more)
        t0 += tsel;
        if (t0 >= t1) return;
        tstep = PBN_GRP_TILES;
    }
    const int c = pair_c[t0 * 128];
    const int tid = threadIdx.x;
    const int wave = tid >> 6, lane = tid & 63;
    const int row16 = lane & 15;
    const int kgrp = lane >> 4;
    const hip_bfloat16* egw_c = egw + (size_t)c * twoH * P_POINTS;

    // stage the whole B table: row j (512 B) split in 2 halves; thread
    // t copies half (t&1) of row (t>>1) - fully coalesced 16-B loads
    for (int t = tid; t < 2 * twoH; t += BLOCK2) {
        const int j = t >> 1, half = t & 1;
        const uint4* g = reinterpret_cast<const uint4*>(
            egw_c + (size_t)j * P_POINTS + half * 128);
        uint4* d = reinterpret_cast<uint4*>(
            reinterpret_cast<char*>(b_lds)
            + (size_t)j * BSTRIDE * 2 + half * 256);
#pragma unroll
        for (int i = 0; i < 16; ++i) d[i] = g[i];
    }
    __syncthreads();

    for (int tile = t0; tile < t1; tile += tstep) {
    const int k0 = tile * 128;
    f32x4 acc[JT];
#pragma unroll
    for (int jt = 0; jt < JT; ++jt) acc[jt] = {0.f, 0.f, 0.f, 0.f};

    const hip_bfloat16* arow =
        a16 + (size_t)(k0 - a_row0 + wave * 16 + row16) * P_POINTS;
#pragma unroll
    for (int kk = 0; kk < P_POINTS; kk += 32) {
        const bf16x8 afrag = *reinterpret_cast<const bf16x8*>(
            arow + kk + kgrp * 8);
#pragma unroll
        for (int jt = 0; jt < JT; ++jt) {
            const int j = jt * 16 + row16;
            bf16x8 bfrag = {};
            if (j < twoH)
                bfrag = *reinterpret_cast<const bf16x8*>(
                    b_lds + (size_t)j * BSTRIDE + kk + kgrp * 8);
            acc[jt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                afrag, bfrag, acc[jt], 0, 0, 0);
        }
    }

    // register-resident epilogue: lane owns pairs kbase..kbase+3 (the
    // accumulator rows) at columns jt*16+row16. For column j: h = j>>1
    // and it contributes to pair r iff vmask bit h == (j&1).
    const int kbase = k0 + wave * 16 + kgrp * 4;
    unsigned vmw[4][(JT + 3) / 4];
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int w = 0; w < (JT + 3) / 4; ++w)
            vmw[r][w] = (w < W)
                ? vmask[(size_t)(kbase + r) * W + w] : 0u;

    float tot[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int jt = 0; jt < JT; ++jt) {
        const int j = jt * 16 + row16;
        if (j >= twoH) continue;
        const int h = j >> 1, v = j & 1;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int bit = (vmw[r][jt >> 2] >> (h & 31)) & 1;
            if (bit == v) tot[r] += acc[jt][r];
        }
    }
    float inv[4];
#pragma unroll
    for (int r = 0; r < 4; ++r)
        inv[r] = 1.0f / fmaxf(row16_reduce(tot[r]), 1e-30f);

    // lanes 2m and 2m+1 hold the two variants of model h = j >> 1; the
    // vmask bit picks the one that writes pm[k, h]
#pragma unroll
    for (int jt = 0; jt < JT; ++jt) {
        const int j = jt * 16 + row16;
        if (j >= twoH) continue;
        const int h = j >> 1, v = j & 1;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int bit = (vmw[r][jt >> 2] >> (h & 31)) & 1;
            if (bit == v) pm[(size_t)(kbase + r) * H + h] = acc[jt][r];
        }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r)
        if (row16 == 0) pinv[kbase + r] = inv[r];
    }  // tile loop
}


// ---------------------------------------------------------------------
// Per-step pass over the pair cache: h_after[k] from pm[k, :], inv[k]
// and the quantities that move every step (pi_hat, mixture0, one row of
// pbest_before), bit-identical to pair_gemm_entropy128_kernel.
//
// The fused kernel gives a pair 16 lanes: lane l walks jt ascending with
// column j = jt*16 + l (h = j >> 1, v = j & 1) and adds the term iff
// vmask bit h == v, so lanes 2m and 2m+1 evaluate the SAME term (it
// depends on h alone) and one of them keeps it. Here a pair has EIGHT
// lanes: lane m takes h = 8*jt + m, evaluates the term once, and keeps
// the fused kernel's two running sums - `even` (its lane 2m) and `odd`
// (lane 2m+1); the vmask bit selects which of them takes the fma, the
// other keeps its value. odd + even is then row16_reduce's first step,
// and row8_reduce_last the rest of its tree. Half the transcendental
// issue, twice the pairs per wave.
//
// A block owns one 128-pair tile (one class: runs are 128-padded) as
// four 32-pair chunks; chunk i+1's rows are in flight in registers while
// chunk i is evaluated from LDS. A chunk is one contiguous 32*H-float
// span, loaded as float4 and laid out in LDS with a row stride = 8 mod
// 64 words, so the 8 pairs of a wave read 64 different banks.
//
// Pad rows (run_off / run_live given): a class's run is its base pair,
// its unique pairs, then padding; a pad row holds the base row's pm and
// inv bit for bit under an all-zero vmask, so its h_after is the base
// row's. A chunk with no live row is not read: the block evaluates the
// class's base row once, through the same code, and stores that value
// into the chunk's rows. Without the two arguments every chunk is read.
// ---------------------------------------------------------------------
#define ECH 4        // 32-pair chunks per block: one 128-pair tile
#define ENQ 5        // float4 per thread per chunk: 8*H/256, H <= 136
#define EWMAX 5      // vmask words: ceil(136 / 32)

__host__ __device__ __forceinline__ int pair_ent_stride(int H) {
    return ((H + 55) / 64) * 64 + 8;     // >= H, = 8 mod 64, 16-B rows
}

// One pair's entropy by the 8 lanes that own it (m = lane & 7), valid in
// lane m == 7. row: the pair's H selected masses.
__device__ __forceinline__ float
pair_ent_row8(const float* row, const float* mix_s, const float* pbb_s,
              const unsigned (&vw)[EWMAX], float inv, float pic, int m,
              int H) {
    float even = 0.f, odd = 0.f;
#pragma unroll
    for (int w = 0; w < EWMAX; ++w) {
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int h = (4 * w + t) * 8 + m;     // h >> 5 == w
            if (h < H) {
                const bool bit = (vw[w] >> (h & 31)) & 1;
                float sel = bit ? odd : even;
                pair_ent_acc(sel, mix_s[h], pic, row[h], inv, pbb_s[h]);
                even = bit ? even : sel;
                odd = bit ? sel : odd;
            }
        }
    }
    return row8_reduce_last(odd + even);
}

__global__ void __launch_bounds__(BLOCK)
pair_entropy_cached_kernel(const float* __restrict__ pm,      // (K, H)
                           const float* __restrict__ pinv,    // (K,)
                           const unsigned* __restrict__ vmask,
                           const int* __restrict__ pair_c,
                           int W,
                           const float* __restrict__ pi_hat,
                           const float* __restrict__ pbest_before,
                           const float* __restrict__ mixture0,
                           const int* __restrict__ run_off,   // (C+1,) / null
                           const int* __restrict__ run_live,  // (C,) / null
                           float* __restrict__ h_after,       // (K,)
                           int H) {
    extern __shared__ char smem[];
    const int stride = pair_ent_stride(H);
    float* rows = reinterpret_cast<float*>(smem);   // [32 * stride]
    float* mix_s = rows + 32 * stride;              // [H]
    float* pbb_s = mix_s + H;                       // [H]
    float* brow = pbb_s + H;                        // [H] the base row
    float* bval = brow + H;                         // [1] its entropy

    const int kb = blockIdx.x * (32 * ECH);
    const int c = pair_c[kb];
    const int tid = threadIdx.x;
    const int pi = tid >> 3, m = tid & 7;
    // chunks of this tile that hold a live row (block-uniform)
    int nlive = ECH, kbase = 0;
    if (run_live != nullptr) {
        kbase = run_off[c];
        const int rem = kbase + run_live[c] - kb;   // live rows from kb on
        nlive = rem <= 0 ? 0 : (rem >= 32 * ECH ? ECH : (rem + 31) >> 5);
    }

    const int nv4 = 8 * H;      // float4 per chunk: 32*H floats, <= 1088
    // chunk start kb + 32*ch: (kb + 32*ch)*H*4 bytes, 128-B aligned
    const f32x4* g = reinterpret_cast<const f32x4*>(pm + (size_t)kb * H);
    // (native vectors: an array of HIP's float4 struct stays in scratch)
    const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
    f32x4 nxt[ENQ];
    if (nlive > 0) {
#pragma unroll
        for (int q = 0; q < ENQ; ++q)
            nxt[q] = tid + q * BLOCK < nv4 ? g[tid + q * BLOCK] : zero4;
    }
    for (int h = tid; h < H; h += BLOCK) {
        mix_s[h] = mixture0[h];
        pbb_s[h] = pbest_before[(size_t)c * H + h];
        if (nlive < ECH) brow[h] = pm[(size_t)kbase * H + h];
    }
    const float pic = pi_hat[c];
    // where this thread's float4s land: element 4*(tid + q*BLOCK) of the
    // chunk is (row, col) = divmod(., H); the same for every chunk
    int drow[ENQ], dcol[ENQ];
#pragma unroll
    for (int q = 0; q < ENQ; ++q) {
        const int e = 4 * (tid + q * BLOCK);
        drow[q] = e / H;
        dcol[q] = e - drow[q] * H;
    }

    if (nlive < ECH) {
        // the tile ends in all-pad chunks: the base row's value, once
        __syncthreads();
        if (pi == 0) {
            unsigned vw[EWMAX];
#pragma unroll
            for (int w = 0; w < EWMAX; ++w)
                vw[w] = w < W ? vmask[(size_t)kbase * W + w] : 0u;
            const float e = pair_ent_row8(brow, mix_s, pbb_s, vw,
                                          pinv[kbase], pic, m, H);
            if (m == 7) bval[0] = e;
        }
        __syncthreads();
        const float e = bval[0];
        for (int r = nlive * 32 + tid; r < 32 * ECH; r += BLOCK)
            h_after[kb + r] = e;
        if (nlive == 0) return;
    }

#pragma unroll 1
    for (int ch = 0; ch < nlive; ++ch) {
        const int k = kb + ch * 32 + pi;
        unsigned vw[EWMAX];
#pragma unroll
        for (int w = 0; w < EWMAX; ++w)
            vw[w] = w < W ? vmask[(size_t)k * W + w] : 0u;
        const float inv = pinv[k];
        if ((H & 3) == 0) {
#pragma unroll
            for (int q = 0; q < ENQ; ++q)
                if (tid + q * BLOCK < nv4)
                    *reinterpret_cast<f32x4*>(
                        rows + drow[q] * stride + dcol[q]) = nxt[q];
        } else {
            // a float4 may straddle rows
#pragma unroll
            for (int q = 0; q < ENQ; ++q)
                if (tid + q * BLOCK < nv4) {
                    int r = drow[q], cc = dcol[q];
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        while (cc >= H) { cc -= H; ++r; }
                        rows[r * stride + cc] = nxt[q][i];
                        ++cc;
                    }
                }
        }
        __syncthreads();
        if (ch + 1 < nlive) {
            const f32x4* gn = g + (size_t)(ch + 1) * nv4;
#pragma unroll
            for (int q = 0; q < ENQ; ++q)
                nxt[q] = tid + q * BLOCK < nv4 ? gn[tid + q * BLOCK]
                                               : zero4;
        }
        const float e = pair_ent_row8(rows + pi * stride, mix_s, pbb_s, vw,
                                      inv, pic, m, H);
        if (m == 7) h_after[k] = e;
        __syncthreads();     // rows are overwritten by the next chunk
    }
}

// ---------------------------------------------------------------------
// Wide-H pipeline (272 < 2H <= 4096, i.e. the multi-GPU H=256..1024
// pools): the fused B-resident tile cannot hold egw[c] or the M tile in
// LDS, so the pairing GEMM writes M (K, 2H) bf16 to global with a
// standard 128x128 double-buffered MFMA tile (B traffic divided by 128
// vs the 16-pair fused tile), and a wave-per-pair entropy kernel
// consumes it with the same vmask epilogue.
// ---------------------------------------------------------------------
#define WSTRIDE 40   // 32 k-elems + 8 pad (16-B-aligned rows)

__global__ void __launch_bounds__(BLOCK)
pair_gemm_wide_kernel(const hip_bfloat16* __restrict__ a16,  // (K, P)
                      const hip_bfloat16* __restrict__ egw,  // (C, 2H, P)
                      const int* __restrict__ pair_c,        // (K,)
                      hip_bfloat16* __restrict__ mout,       // (K, 2H)
                      int twoH) {
    extern __shared__ char smem[];
    // [2 buffers][128 rows][WSTRIDE] for A and B chunks
    hip_bfloat16* a_lds = reinterpret_cast<hip_bfloat16*>(smem);
    hip_bfloat16* b_lds = a_lds + 2 * 128 * WSTRIDE;

    const int k0 = blockIdx.x * 128;
    const int j0 = blockIdx.y * 128;
    const int c = pair_c[k0];
    const int tid = threadIdx.x;
    const int wave = tid >> 6, lane = tid & 63;
    const int row16 = lane & 15, kgrp = lane >> 4;
    const hip_bfloat16* egw_c = egw + (size_t)c * twoH * P_POINTS;

    // stage one 128x32 chunk of A or B: thread t loads 16 B (8 elems)
    auto stage = [&](hip_bfloat16* dst, const hip_bfloat16* src,
                     int kk, bool valid_rows) {
        const int row = tid >> 1, half = tid & 1;
        const uint4* g = reinterpret_cast<const uint4*>(
            src + (size_t)row * P_POINTS + kk + half * 16);
        uint4* d = reinterpret_cast<uint4*>(
            reinterpret_cast<char*>(dst)
            + (size_t)row * WSTRIDE * 2 + half * 32);
        if (valid_rows) { d[0] = g[0]; d[1] = g[1]; }
    };

    stage(a_lds, a16 + (size_t)k0 * P_POINTS, 0, true);
    stage(b_lds, egw_c + (size_t)j0 * P_POINTS, 0,
          j0 + (tid >> 1) < twoH);
    __syncthreads();

    f32x4 acc[2][8];
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
        for (int jt = 0; jt < 8; ++jt) acc[r][jt] = {0.f, 0.f, 0.f, 0.f};

    for (int kk = 0; kk < P_POINTS; kk += 32) {
        const int cur = (kk >> 5) & 1;
        if (kk + 32 < P_POINTS) {
            stage(a_lds + (cur ^ 1) * 128 * WSTRIDE,
                  a16 + (size_t)k0 * P_POINTS, kk + 32, true);
            stage(b_lds + (cur ^ 1) * 128 * WSTRIDE,
                  egw_c + (size_t)j0 * P_POINTS, kk + 32,
                  j0 + (threadIdx.x >> 1) < twoH);
        }
        const hip_bfloat16* ab = a_lds + cur * 128 * WSTRIDE;
        const hip_bfloat16* bb = b_lds + cur * 128 * WSTRIDE;
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            // wave w owns pair rows [wave*32 + r*16 + row16]
            const bf16x8 afrag = *reinterpret_cast<const bf16x8*>(
                ab + (size_t)(wave * 32 + r * 16 + row16) * WSTRIDE
                + kgrp * 8);
#pragma unroll
            for (int jt = 0; jt < 8; ++jt) {
                const bf16x8 bfrag = *reinterpret_cast<const bf16x8*>(
                    bb + (size_t)(jt * 16 + row16) * WSTRIDE + kgrp * 8);
                acc[r][jt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                    afrag, bfrag, acc[r][jt], 0, 0, 0);
            }
        }
        __syncthreads();
    }

    // write M tile: D col = row16 (the B row j), D rows = kgrp*4+e
#pragma unroll
    for (int r = 0; r < 2; ++r) {
#pragma unroll
        for (int jt = 0; jt < 8; ++jt) {
            const int j = j0 + jt * 16 + row16;
            if (j >= twoH) continue;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int k = k0 + wave * 32 + r * 16 + kgrp * 4 + e;
                mout[(size_t)k * twoH + j] =
                    hip_bfloat16(acc[r][jt][e]);
            }
        }
    }
}

__global__ void __launch_bounds__(BLOCK)
pair_entropy_wide_kernel(const hip_bfloat16* __restrict__ m,  // (K, 2H)
                         const unsigned* __restrict__ vmask,  // (K, W)
                         const int* __restrict__ pair_c,      // (K,)
                         int W,
                         const float* __restrict__ pi_hat,
                         const float* __restrict__ pbest_before,
                         const float* __restrict__ mixture0,
                         float* __restrict__ h_after,         // (K,)
                         int K, int H) {
    const int k = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (k >= K) return;
    const int lane = threadIdx.x & 63;
    const int c = pair_c[k];
    const unsigned* vm = vmask + (size_t)k * W;
    const hip_bfloat16* mrow = m + (size_t)k * 2 * H;

    float val[32];   // H <= 2048 -> <= 32 h per lane
    float tot = 0.f;
    int i = 0;
    for (int h = lane; h < H; h += 64, ++i) {
        const int v = (vm[h >> 5] >> (h & 31)) & 1;
        val[i] = (float)mrow[2 * h + v];
        tot += val[i];
    }
    tot = wave_reduce_sum(tot);
    const float inv = 1.0f / fmaxf(tot, 1e-30f);
    const float pic = pi_hat[c];
    float ent = 0.f;
    i = 0;
    for (int h = lane; h < H; h += 64, ++i) {
        const float pb = val[i] * inv;
        const float mm = fmaxf(
            mixture0[h] + pic * (pb - pbest_before[(size_t)c * H + h]),
            1e-12f);
        ent += -mm * __log2f(mm);
    }
    ent = wave_reduce_sum(ent);
    if (lane == 0) h_after[k] = ent;
}

// ---------------------------------------------------------------------
// Finalize: q[b] = H_before - (1/rowsum) * (arow . h_base
//                 + sum_{pairs of b} arow[c]*(h_after - h_base[c]))
// One wave per candidate at a time; fixed reduction order
// (deterministic): lane l owns classes 4l + 256i, i ascending, then the
// scalar tail; hits s = off + l + 64i, ascending; wave_reduce_sum.
//
// The pass is a stream over the (N, C) `adjusted` rows carrying a
// gather per hit, so what matters is how many loads a wave has in
// flight and how few dependent latencies it pays per 4 KB row:
//   - a strided grid (at most FIN_MAX_BLOCKS blocks) whose waves walk
//     candidates b, b + stride, ...; h_base (4 KB at C = 1000) is staged
//     in LDS once per block and serves the row dot and the hit gathers;
//   - the wave index is made uniform, so cand_ids / cand_off are scalar
//     loads, and the NEXT candidate's are fetched while this one's row
//     is in flight;
//   - per candidate the packed-hit load is issued first, then the row's
//     float4 chunks four at a time (C = 1000 is one batch), then the
//     first hit's gathers - all before the first product is formed, and
//     straight-line, so the compiler's load counters stay exact.
// Which candidate a wave takes changes nothing in a candidate's sums.
// ---------------------------------------------------------------------
#define FIN_MAX_BLOCKS 2048   // 256 CUs x 8 blocks of 4 waves
#define FIN_LDS_MAX_C 8192    // h_base beyond 32 KB is read from L2

// VEC: C >= 4, the float4 part exists (C < 4 is the scalar tail alone).
template <bool HB_LDS, bool VEC>
__global__ void __launch_bounds__(BLOCK)
pair_eig_finalize_kernel(const float* __restrict__ h_after,   // (K,)
                         const float* __restrict__ h_base,    // (C,)
                         const int* __restrict__ cand_off,    // (B+1,)
                         const long long* __restrict__ cand_ck,  // (hits,)
                         const long* __restrict__ cand_ids,   // (B,)
                         const float* __restrict__ adjusted,  // (N, C)
                         const float* __restrict__ row_sums,  // (N,)
                         float H_before,
                         float* __restrict__ q,               // (B,)
                         int B, int C, int nhits) {
    extern __shared__ char smem[];
    float* hb_s = reinterpret_cast<float*>(smem);              // [C]
    if constexpr (HB_LDS) {
        for (int i = threadIdx.x; i < C; i += BLOCK) hb_s[i] = h_base[i];
        __syncthreads();       // the only barrier: waves part ways below
    }
    auto hb1 = [&](int i) -> float {
        if constexpr (HB_LDS) return hb_s[i]; else return h_base[i];
    };
    auto hb4 = [&](int i) -> f32x4 {
        if constexpr (HB_LDS)
            return *reinterpret_cast<const f32x4*>(hb_s + i);
        else
            return *reinterpret_cast<const f32x4*>(h_base + i);
    };

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int stride = gridDim.x * 4;
    int b = blockIdx.x * 4 + wave;
    if (b >= B) return;
    // float4 chunks this lane owns (4*lane + 256*i + 3 < C), and lane
    // 0's count, the most of any lane
    const int n4 = C - 3 > 4 * lane ? (C - 3 - 4 * lane + 255) / 256 : 0;
    const int n4w = C > 3 ? (C - 3 + 255) / 256 : 0;
    // Every load up to the first product is UNCONDITIONAL, on an address
    // clamped into bounds: a load under a lane mask costs the compiler
    // its count of the loads in flight, and it then waits for all of
    // them at the next use. A clamped load's value is never used.
    // (global float4 row loads are only 4-B aligned whenever C % 4 != 0,
    // here as in every row of such a pool: the hardware takes them)
    const int cvec = C - 4;                    // last in-row float4 start
    const int cvec_hb = cvec & ~3;             // the same, 16-B aligned (LDS)
    const int nh1 = nhits - 1;                 // nhits >= 1 (host)

    long id = cand_ids[b];
    int s0 = cand_off[b], s1 = cand_off[b + 1];
    for (;;) {
        const int s = s0 + lane;
        const bool hit = s < s1;
        // a lane without a hit gathers entry (pair 0, class 0) - K >= 1
        // and C >= 1 (host) - whatever the clamped slot holds
        const long long pk0 = cand_ck[min(hit ? s : s0, nh1)];
        long long pk = hit ? pk0 : 0;
        const float rs = row_sums[id];
        const float* arow = adjusted + (size_t)id * C;
        // the next candidate's scalars, behind this one's loads
        const int bn = b + stride;
        const int bnc = min(bn, B - 1);
        const long idn = cand_ids[bnc];
        const int s0n = cand_off[bnc], s1n = cand_off[bnc + 1];

        float base = 0.f;
        // (native vectors: an array of HIP's float4 stays in scratch)
        f32x4 a[4], hb[4];
        if constexpr (VEC) {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                a[j] = *reinterpret_cast<const f32x4*>(
                    arow + min(lane * 4 + j * 256, cvec));
        }
        // first hit's gathers
        const int c2 = (int)(pk & 0xffffffff);
        const float ga = arow[c2];
        const float gh = h_after[(int)(pk >> 32)];
        const float ghb = hb1(c2);
        if constexpr (VEC) {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                hb[j] = hb4(min(lane * 4 + j * 256, cvec_hb));
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                // a select, not a branch: the load must not sink into it
                const float nb = base
                    + (a[j][0] * hb[j][0] + a[j][1] * hb[j][1]
                       + a[j][2] * hb[j][2] + a[j][3] * hb[j][3]);
                base = j < n4 ? nb : base;
            }
            for (int i0 = 4; i0 < n4w; i0 += 4) {      // C > 1024
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    a[j] = *reinterpret_cast<const f32x4*>(
                        arow + min(lane * 4 + (i0 + j) * 256, cvec));
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    hb[j] = hb4(min(lane * 4 + (i0 + j) * 256, cvec_hb));
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float nb = base
                        + (a[j][0] * hb[j][0] + a[j][1] * hb[j][1]
                           + a[j][2] * hb[j][2] + a[j][3] * hb[j][3]);
                    base = i0 + j < n4 ? nb : base;
                }
            }
        }
        for (int cc = lane * 4 + n4 * 256; cc < C; ++cc)
            base += arow[cc] * hb1(cc);

        // (pair, class) packed per hit: one load decodes both, so the
        // chase is packed -> {h_after, arow} (2 dependent levels)
        const float c0 = 0.f + ga * (gh - ghb);
        float corr = hit ? c0 : 0.f;
        for (int s2 = s + 64; s2 < s1; s2 += 64) {
            pk = cand_ck[s2];
            const int k = (int)(pk >> 32);
            const int cx = (int)(pk & 0xffffffff);
            corr += arow[cx] * (h_after[k] - hb1(cx));
        }
        const float inv = 1.0f / fmaxf(rs, 1e-12f);
        const float tot = wave_reduce_sum(base + corr);
        if (lane == 0) q[b] = H_before - tot * inv;
        if (bn >= B) break;
        b = bn; id = idn; s0 = s0n; s1 = s1n;
    }
}

// cls-based wide entropy (H beyond the vmask regime, e.g. 10k-model
// pools): v-select reads the candidate's argmax classes directly (the
// B x H cls block is small for prefiltered candidate sets and
// L2-resident); no per-lane value cache (H unbounded), so M is read
// twice.
__global__ void __launch_bounds__(BLOCK)
pair_entropy_wide_cls_kernel(const hip_bfloat16* __restrict__ m,  // (K, 2H)
                             const int* __restrict__ cls,         // (B, H)
                             const int* __restrict__ pair_b,      // (K,)
                             const int* __restrict__ pair_c,      // (K,)
                             const float* __restrict__ pi_hat,
                             const float* __restrict__ pbest_before,
                             const float* __restrict__ mixture0,
                             float* __restrict__ h_after,         // (K,)
                             int K, int H) {
    const int k = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (k >= K) return;
    const int lane = threadIdx.x & 63;
    const int c = pair_c[k];
    const int b = pair_b[k];
    const hip_bfloat16* mrow = m + (size_t)k * 2 * H;

    float tot = 0.f;
    for (int h = lane; h < H; h += 64) {
        const int v = (b >= 0 && cls[(size_t)b * H + h] == c) ? 1 : 0;
        tot += (float)mrow[2 * h + v];
    }
    tot = wave_reduce_sum(tot);
    const float inv = 1.0f / fmaxf(tot, 1e-30f);
    const float pic = pi_hat[c];
    float ent = 0.f;
    for (int h = lane; h < H; h += 64) {
        const int v = (b >= 0 && cls[(size_t)b * H + h] == c) ? 1 : 0;
        const float pb = (float)mrow[2 * h + v] * inv;
        const float mm = fmaxf(
            mixture0[h] + pic * (pb - pbest_before[(size_t)c * H + h]),
            1e-12f);
        ent += -mm * __log2f(mm);
    }
    ent = wave_reduce_sum(ent);
    if (lane == 0) h_after[k] = ent;
}

// ---------------------------------------------------------------------
// Fused acquisition epilogue.  After pair_eig_finalize the graphed
// get_next tail was ~10 small torch launches (add + where(-inf) + max
// + isclose chain + sum + qbuf copy + stack/copy, ~120 us/step at
// B=50k): three kernels replace it.
//   K1: qbuf = active ? h0 + q0 : -inf, per-block (max, first-idx)
//   K2: one block combines the partials -> out[0..1]
//   K3: tie count q == best, or |q - best| finite and <= atol +
//       rtol*|best|, over active candidates (torch.isclose on finite
//       and infinite values), f64 atomic into out[2] (integer-valued
//       doubles: exact, order-independent)
// The contract, as plain numpy, is tests/acq_ref.py.
// ---------------------------------------------------------------------
#define ACQ_GRID 256

__global__ void __launch_bounds__(BLOCK)
acq_select_part_kernel(const float* __restrict__ q0,
                       const float* __restrict__ h0,     // scalar (1,)
                       const bool* __restrict__ active,
                       float* __restrict__ qbuf,
                       float* __restrict__ pmax, int* __restrict__ pidx,
                       int B) {
    const int per = (B + gridDim.x - 1) / gridDim.x;
    const int b0 = blockIdx.x * per;
    const int b1 = min(b0 + per, B);
    const float h = h0[0];
    float best = -INFINITY;
    int bidx = -1;
    for (int i = b0 + threadIdx.x; i < b1; i += BLOCK) {
        const bool a = active[i];
        const float q = a ? h + q0[i] : -INFINITY;
        qbuf[i] = q;
        // strict: first index wins.  The first active candidate seeds
        // (best, bidx) even at -inf, so an all -inf active set yields its
        // first index, not -1.  NaN compares false both ways and is
        // skipped, unlike the eager chain, whose max propagates it.
        if (a && (q > best || (bidx < 0 && q == best))) {
            best = q;
            bidx = i;
        }
    }
    __shared__ float sv[BLOCK];
    __shared__ int si[BLOCK];
    sv[threadIdx.x] = best;
    si[threadIdx.x] = bidx;
    __syncthreads();
    for (int s = BLOCK / 2; s > 0; s >>= 1) {
        if (threadIdx.x < s) {
            const float ov = sv[threadIdx.x + s];
            const int oi = si[threadIdx.x + s];
            if (ov > sv[threadIdx.x]
                || (ov == sv[threadIdx.x] && oi != -1
                    && (si[threadIdx.x] == -1 || oi < si[threadIdx.x]))) {
                sv[threadIdx.x] = ov;
                si[threadIdx.x] = oi;
            }
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        pmax[blockIdx.x] = sv[0];
        pidx[blockIdx.x] = si[0];
    }
}

__global__ void __launch_bounds__(ACQ_GRID)
acq_select_combine_kernel(const float* __restrict__ pmax,
                          const int* __restrict__ pidx,
                          double* __restrict__ out,     // (3,) f64
                          long long* __restrict__ tbuf) {
    __shared__ float sv[ACQ_GRID];
    __shared__ int si[ACQ_GRID];
    sv[threadIdx.x] = pmax[threadIdx.x];
    si[threadIdx.x] = pidx[threadIdx.x];
    __syncthreads();
    for (int s = ACQ_GRID / 2; s > 0; s >>= 1) {
        if (threadIdx.x < s) {
            const float ov = sv[threadIdx.x + s];
            const int oi = si[threadIdx.x + s];
            if (ov > sv[threadIdx.x]
                || (ov == sv[threadIdx.x] && oi != -1
                    && (si[threadIdx.x] == -1 || oi < si[threadIdx.x]))) {
                sv[threadIdx.x] = ov;
                si[threadIdx.x] = oi;
            }
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        out[0] = (double)sv[0];
        out[1] = (double)si[0];
        out[2] = 0.0;
        tbuf[0] = 0;                       // reset the tie-slot counter
    }
}

__global__ void __launch_bounds__(BLOCK)
acq_select_ties_kernel(const float* __restrict__ qbuf,
                       const bool* __restrict__ active,
                       double* __restrict__ out,
                       long long* __restrict__ tbuf,  // [0]=n, [1..cap]
                       int cap, int B) {
    const float best = (float)out[0];
    const float thr = 1e-8f + 1e-8f * fabsf(best);
    const int per = (B + gridDim.x - 1) / gridDim.x;
    const int b0 = blockIdx.x * per;
    const int b1 = min(b0 + per, B);
    int cnt = 0;
    for (int i = b0 + threadIdx.x; i < b1; i += BLOCK) {
        if (!active[i]) continue;
        // isclose as ATen defines it: equal (which is what makes equal
        // infinities tie), or a FINITE difference within the threshold
        // (thr is +inf at an infinite best, where |q - best| is too)
        const float q = qbuf[i];
        const float d = fabsf(q - best);
        if (q == best || (d <= thr && d < INFINITY)) {
            ++cnt;
            // unordered slots, each packing (position, q value) so the
            // host tie-break needs NO second device fetch; the host
            // sorts the <= cap entries back to ascending position
            const int slot = (int)atomicAdd(
                reinterpret_cast<unsigned long long*>(tbuf), 1ull);
            if (slot < cap)
                tbuf[1 + slot] = ((long long)i << 32)
                    | (unsigned int)__float_as_int(q);
        }
    }
    __shared__ int sc[BLOCK];
    sc[threadIdx.x] = cnt;
    __syncthreads();
    for (int s = BLOCK / 2; s > 0; s >>= 1) {
        if (threadIdx.x < s) sc[threadIdx.x] += sc[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0 && sc[0] > 0)
        atomicAdd(out + 2, (double)sc[0]);
}

// ---------------------------------------------------------------------
// Batch acquisition: the K best DISTINCT candidates of the qbuf the
// epilogue above left, in rank order (q descending, position ascending,
// -0 as +0), optionally one per group. The contract, as plain numpy, is
// tests/acq_topk_ref.py.
//
// Every active candidate maps to one u64 key, high word the monotone
// unsigned image of its q, low word 0xFFFFFFFF - position; 0 is "empty".
// The order is then "larger key first" and keys are unique, so every
// reduction is an integer max or an integer count: order-independent,
// bit-reproducible through atomics.
//   prep     zero the digit histograms, the slot counter and (groups)
//            the best-per-group keys
//   group    (groups only) u64 atomicMax of each candidate's key into
//            its group's word: the survivors are the group winners
//   hist x6  radix select of the K-th largest key, most significant
//            digit first (11 bits a pass, 9 in the last). Each block
//            derives the prefix found so far from the previous pass's
//            histogram, counts its slice's matching keys per digit in
//            LDS and adds the counts to the pass's global histogram
//   gather   keys >= the K-th largest go to unordered slots
//   sort     one block: bitonic sort of the <= 1024 slots, decoded to
//            (position << 32) | q bits, padded with -1
// A kernel boundary is the only ordering between blocks.
// ---------------------------------------------------------------------
#define TOPK_MAX 1024
#define TOPK_BINS 2048
#define TOPK_PASSES 6
// int32 workspace: [0, PASSES*BINS) histograms, then the slot counter,
// then (prefix lo, prefix hi, still wanted, take-all) per pass
#define TOPK_WS_CNT (TOPK_PASSES * TOPK_BINS)
#define TOPK_WS_STATE (TOPK_WS_CNT + 4)
#define TOPK_WS_INTS (TOPK_WS_STATE + 4 * TOPK_PASSES)

__device__ __forceinline__ int topk_shift(int p) {
    return p == TOPK_PASSES - 1 ? 0 : 64 - 11 * (p + 1);
}

__device__ __forceinline__ int topk_mask(int p) {
    return p == TOPK_PASSES - 1 ? 511 : TOPK_BINS - 1;
}

__device__ __forceinline__ unsigned long long
topk_key_of(float q, int i) {
    if (q == 0.0f) q = 0.0f;                    // -0 orders as +0
    const unsigned int u = (unsigned int)__float_as_int(q);
    const unsigned int m = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
    return ((unsigned long long)m << 32) | (0xFFFFFFFFu - (unsigned int)i);
}

// survivor i's key: the group winners when keys is given, else built
// from the masked q
__device__ __forceinline__ unsigned long long
topk_load(const unsigned long long* __restrict__ keys,
          const float* __restrict__ qbuf, const bool* __restrict__ active,
          int i) {
    if (keys != nullptr) return keys[i];
    return active[i] ? topk_key_of(qbuf[i], i) : 0ull;
}

struct TopkState {
    unsigned long long prefix;  // digits found so far, in place
    int want;                   // ranks still to find under the prefix
    int all;                    // fewer survivors than K: take them all
};

// State entering pass p, by every thread of a BLOCK-thread block: the
// state entering pass p-1 (written by that pass's block 0) advanced by
// that pass's finished histogram. Pass 0 starts from (0, K).
__device__ TopkState topk_state(const int* __restrict__ ws, int p, int K) {
    __shared__ int ssum[BLOCK];
    __shared__ int sres[2];     // digit, ranks wanted inside it
    TopkState s;
    if (p == 0) {
        s.prefix = 0ull; s.want = K; s.all = 0;
        return s;
    }
    if (p == 1) {
        s.prefix = 0ull; s.want = K; s.all = 0;
    } else {
        const int* st = ws + TOPK_WS_STATE + 4 * (p - 1);
        s.prefix = ((unsigned long long)(unsigned int)st[1] << 32)
            | (unsigned int)st[0];
        s.want = st[2];
        s.all = st[3];
    }
    if (s.all) return s;        // uniform: read from global
    const int* h = ws + (p - 1) * TOPK_BINS + threadIdx.x * 8;
    int hv[8];
    int tot = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) { hv[j] = h[j]; tot += hv[j]; }
    ssum[threadIdx.x] = tot;
    if (threadIdx.x == 0) sres[0] = -1;
    __syncthreads();
    // inclusive suffix sums over the threads' totals
    for (int d = 1; d < BLOCK; d <<= 1) {
        const int add = threadIdx.x + d < BLOCK
            ? ssum[threadIdx.x + d] : 0;
        __syncthreads();
        ssum[threadIdx.x] += add;
        __syncthreads();
    }
    int above = ssum[threadIdx.x] - tot;   // counts in higher digits
    if (above < s.want && s.want <= above + tot) {
#pragma unroll
        for (int j = 7; j >= 0; --j) {
            if (above < s.want && s.want <= above + hv[j]) {
                sres[0] = threadIdx.x * 8 + j;
                sres[1] = s.want - above;
            }
            above += hv[j];
        }
    }
    __syncthreads();
    const int digit = sres[0];
    const int want = sres[1];
    __syncthreads();            // sres is reused by the caller's next call
    if (digit < 0) {
        s.all = 1;
    } else {
        s.prefix |= (unsigned long long)digit << topk_shift(p - 1);
        s.want = want;
    }
    return s;
}

__global__ void __launch_bounds__(BLOCK)
topk_prep_kernel(int* __restrict__ ws,
                 unsigned long long* __restrict__ gbest, int G) {
    const int t = blockIdx.x * BLOCK + threadIdx.x;
    const int n = gridDim.x * BLOCK;
    for (int i = t; i <= TOPK_WS_CNT; i += n) ws[i] = 0;
    for (int i = t; i < G; i += n) gbest[i] = 0ull;
}

__global__ void __launch_bounds__(BLOCK)
topk_group_kernel(const float* __restrict__ qbuf,
                  const bool* __restrict__ active,
                  const int* __restrict__ group_of,
                  unsigned long long* __restrict__ gbest, int G, int B) {
    const int per = (B + gridDim.x - 1) / gridDim.x;
    const int b0 = blockIdx.x * per;
    const int b1 = min(b0 + per, B);
    for (int i = b0 + threadIdx.x; i < b1; i += BLOCK) {
        if (!active[i]) continue;
        const int g = group_of[i];
        if ((unsigned int)g < (unsigned int)G)
            atomicMax(gbest + g, topk_key_of(qbuf[i], i));
    }
}

__global__ void __launch_bounds__(BLOCK)
topk_hist_kernel(const unsigned long long* __restrict__ keys,
                 const float* __restrict__ qbuf,
                 const bool* __restrict__ active,
                 int* __restrict__ ws, int p, int K, int n) {
    __shared__ int hist[TOPK_BINS];
    for (int j = threadIdx.x; j < TOPK_BINS; j += BLOCK) hist[j] = 0;
    const TopkState s = topk_state(ws, p, K);   // syncs (p > 0)
    if (p > 0 && blockIdx.x == 0 && threadIdx.x == 0) {
        int* st = ws + TOPK_WS_STATE + 4 * p;
        st[0] = (int)(unsigned int)s.prefix;
        st[1] = (int)(unsigned int)(s.prefix >> 32);
        st[2] = s.want;
        st[3] = s.all;
    }
    if (s.all) return;
    __syncthreads();
    const int shift = topk_shift(p);
    const int above = p == 0 ? 64 : topk_shift(p - 1);
    const int per = (n + gridDim.x - 1) / gridDim.x;
    const int b0 = blockIdx.x * per;
    const int b1 = min(b0 + per, n);
    for (int i = b0 + threadIdx.x; i < b1; i += BLOCK) {
        const unsigned long long k = topk_load(keys, qbuf, active, i);
        if (k == 0ull) continue;
        if (above < 64 && (k >> above) != (s.prefix >> above)) continue;
        atomicAdd(&hist[(int)(k >> shift) & topk_mask(p)], 1);
    }
    __syncthreads();
    int* gh = ws + p * TOPK_BINS;
    for (int j = threadIdx.x; j < TOPK_BINS; j += BLOCK)
        if (hist[j] != 0) atomicAdd(gh + j, hist[j]);
}

__global__ void __launch_bounds__(BLOCK)
topk_gather_kernel(const unsigned long long* __restrict__ keys,
                   const float* __restrict__ qbuf,
                   const bool* __restrict__ active,
                   int* __restrict__ ws,
                   unsigned long long* __restrict__ sel, int K, int n) {
    const TopkState s = topk_state(ws, TOPK_PASSES, K);
    const unsigned long long thr = s.all ? 1ull : s.prefix;
    const int per = (n + gridDim.x - 1) / gridDim.x;
    const int b0 = blockIdx.x * per;
    const int b1 = min(b0 + per, n);
    for (int i = b0 + threadIdx.x; i < b1; i += BLOCK) {
        const unsigned long long k = topk_load(keys, qbuf, active, i);
        if (k == 0ull || k < thr) continue;
        const int slot = atomicAdd(ws + TOPK_WS_CNT, 1);
        if (slot < TOPK_MAX) sel[slot] = k;
    }
}

__global__ void __launch_bounds__(TOPK_MAX)
topk_sort_kernel(const unsigned long long* __restrict__ sel,
                 const int* __restrict__ ws,
                 const float* __restrict__ qbuf,
                 long long* __restrict__ topk, int K) {
    __shared__ unsigned long long sk[TOPK_MAX];
    const int t = threadIdx.x;
    const int cnt = min(ws[TOPK_WS_CNT], TOPK_MAX);
    sk[t] = t < cnt ? sel[t] : 0ull;
    __syncthreads();
    for (int k = 2; k <= TOPK_MAX; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            const int o = t ^ j;
            if (o > t) {
                const unsigned long long a = sk[t], b = sk[o];
                // descending overall
                if (((t & k) == 0) ? (a < b) : (a > b)) {
                    sk[t] = b;
                    sk[o] = a;
                }
            }
            __syncthreads();
        }
    }
    if (t < K) {
        const unsigned long long k = sk[t];
        long long w = -1;
        if (k != 0ull && t < cnt) {
            const unsigned int pos = 0xFFFFFFFFu - (unsigned int)k;
            // the entry's own bits (a -0 stays -0), as the tie words
            w = ((long long)pos << 32)
                | (unsigned int)__float_as_int(qbuf[pos]);
        }
        topk[t] = w;
    }
}

// MFMA layout probe (correctness insurance, not a production op):
// C (16,16) = A (16,32) x B stored row-major as BT (16 cols x 32 k).
__global__ void mfma_probe_kernel(const float* __restrict__ a,   // (16,32)
                                  const float* __restrict__ bt,  // (16,32)
                                  float* __restrict__ out) {     // (16,16)
    if (threadIdx.x >= 64) return;
    const int lane = threadIdx.x;
    const int row16 = lane & 15, kgrp = lane >> 4;
    bf16x8 afrag, bfrag;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        afrag[e] = (__bf16)a[row16 * 32 + kgrp * 8 + e];
        bfrag[e] = (__bf16)bt[row16 * 32 + kgrp * 8 + e];
    }
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(afrag, bfrag, acc,
                                                  0, 0, 0);
#pragma unroll
    for (int r = 0; r < 4; ++r)
        out[(kgrp * 4 + r) * 16 + row16] = acc[r];
}

}  // namespace pairops

// ---------------------------------------------------------------------
// Host bindings
// ---------------------------------------------------------------------

torch::Tensor pair_dsum_es(torch::Tensor delta16, torch::Tensor dall,
                           torch::Tensor pair_c, torch::Tensor pair_neg,
                           torch::Tensor seg_off, torch::Tensor seg_h) {
    TORCH_CHECK(delta16.is_cuda() && delta16.dtype() == torch::kFloat16);
    TORCH_CHECK(delta16.size(-1) == P_POINTS);
    TORCH_CHECK(dall.dtype() == torch::kFloat32);
    const int H = delta16.size(1);
    const int K = pair_c.size(0);
    auto a16 = torch::empty({K, P_POINTS},
                            delta16.options().dtype(torch::kBFloat16));
    auto stream = c10::hip::getCurrentHIPStream();
    dim3 grid((K + 15) / 16);
    hipLaunchKernelGGL(pairops::pair_dsum_es_kernel, grid, dim3(BLOCK), 0,
                       stream.stream(),
                       reinterpret_cast<const _Float16*>(
                           delta16.data_ptr()),
                       dall.data_ptr<float>(),
                       pair_c.data_ptr<int>(), pair_neg.data_ptr<int>(),
                       seg_off.data_ptr<int>(), seg_h.data_ptr<int>(),
                       reinterpret_cast<hip_bfloat16*>(a16.data_ptr()),
                       K, H);
    return a16;
}

torch::Tensor pair_gemm_entropy(torch::Tensor a16, torch::Tensor egw,
                                torch::Tensor vmask, torch::Tensor pair_c,
                                torch::Tensor pi_hat,
                                torch::Tensor pbest_before,
                                torch::Tensor mixture0, int64_t tile,
                                int64_t ablate, torch::Tensor grp) {
    TORCH_CHECK(a16.is_cuda() && a16.dtype() == torch::kBFloat16);
    TORCH_CHECK(egw.dtype() == torch::kBFloat16);
    const int K = a16.size(0);
    const int H = mixture0.size(0);
    TORCH_CHECK(K % tile == 0, "pair count must be tile-padded");
    TORCH_CHECK(egw.size(1) == 2 * H);
    const int mstride = 2 * H + 4;  // LDS row pad against bank conflicts
    auto h_after = torch::empty({K}, pi_hat.options());
    auto stream = c10::hip::getCurrentHIPStream();
    const auto ab16 = reinterpret_cast<const hip_bfloat16*>(
        a16.data_ptr());
    const auto eb16 = reinterpret_cast<const hip_bfloat16*>(
        egw.data_ptr());
    if (tile == 128 && 2 * H > 272) {
        // wide-H split pipeline: M to global, entropy second pass
        TORCH_CHECK(2 * H <= 4096, "pair engine caps at H = 2048");
        const int twoH = 2 * H;
        auto mout = torch::empty({(long)K, (long)twoH},
                                 a16.options());
        const size_t shmem = 4 * 128 * WSTRIDE * sizeof(hip_bfloat16);
        dim3 grid(K / 128, (twoH + 127) / 128);
        hipLaunchKernelGGL(pairops::pair_gemm_wide_kernel, grid,
                           dim3(BLOCK), shmem, stream.stream(), ab16,
                           eb16, pair_c.data_ptr<int>(),
                           reinterpret_cast<hip_bfloat16*>(
                               mout.data_ptr()),
                           twoH);
        hipLaunchKernelGGL(pairops::pair_entropy_wide_kernel,
                           dim3((K + 3) / 4), dim3(BLOCK), 0,
                           stream.stream(),
                           reinterpret_cast<const hip_bfloat16*>(
                               mout.data_ptr()),
                           reinterpret_cast<const unsigned*>(
                               vmask.data_ptr<int>()),
                           pair_c.data_ptr<int>(), (int)vmask.size(1),
                           pi_hat.data_ptr<float>(),
                           pbest_before.data_ptr<float>(),
                           mixture0.data_ptr<float>(),
                           h_after.data_ptr<float>(), K, H);
    } else if (tile == 128) {
        TORCH_CHECK(2 * H <= 272, "128-pair tile needs 2H <= 272");
        const size_t shmem = (size_t)2 * H * BSTRIDE
                           * sizeof(hip_bfloat16);
        const int JT = (2 * H + 15) / 16;
        // tile groups (same-class runs, capped): default 1 tile/block
        torch::Tensor grp_t = grp;
        if (grp_t.numel() == 0)
            grp_t = torch::arange(K / 128 + 1,
                                  pair_c.options().dtype(torch::kInt32));
        TORCH_CHECK(grp_t.scalar_type() == torch::kInt32
                    && grp_t.is_contiguous());
        const int ngrp = grp_t.numel() - 1;
        auto launch = [&](auto kern) {
            hipLaunchKernelGGL(kern, dim3(ngrp), dim3(BLOCK2), shmem,
                               stream.stream(), ab16, eb16,
                               reinterpret_cast<const unsigned*>(
                                   vmask.data_ptr<int>()),
                               pair_c.data_ptr<int>(),
                               (int)vmask.size(1),
                               pi_hat.data_ptr<float>(),
                               pbest_before.data_ptr<float>(),
                               mixture0.data_ptr<float>(),
                               h_after.data_ptr<float>(),
                               grp_t.data_ptr<int>(), H, mstride);
        };
        (void)ablate;  // phase-ablation diagnostics retired
        if (JT <= 4) launch(pairops::pair_gemm_entropy128_kernel<4>);
        else if (JT <= 8)
            launch(pairops::pair_gemm_entropy128_kernel<8>);
        else if (JT <= 16)
            launch(pairops::pair_gemm_entropy128_kernel<16>);
        else launch(pairops::pair_gemm_entropy128_kernel<17>);
    } else {
        TORCH_CHECK(tile == 16, "tile must be 16 or 128");
        const size_t shmem = 16 * P_POINTS * sizeof(hip_bfloat16)
                           + (size_t)16 * mstride * sizeof(float);
        TORCH_CHECK(shmem <= 160 * 1024, "H too large for the fused "
                    "pair kernel (use the table engine beyond H=1024)");
        hipLaunchKernelGGL(pairops::pair_gemm_entropy16_kernel,
                           dim3(K / 16), dim3(BLOCK), shmem,
                           stream.stream(), ab16, eb16,
                           reinterpret_cast<const unsigned*>(
                               vmask.data_ptr<int>()),
                           pair_c.data_ptr<int>(),
                           (int)vmask.size(1),
                           pi_hat.data_ptr<float>(),
                           pbest_before.data_ptr<float>(),
                           mixture0.data_ptr<float>(),
                           h_after.data_ptr<float>(), H, mstride);
    }
    return h_after;
}

// -- pair cache (fused B-resident route only: tile 128, 2H <= 272) -----

void pair_dsum_es_cls(torch::Tensor delta16, torch::Tensor dall,
                      torch::Tensor pair_c, torch::Tensor pair_neg,
                      torch::Tensor seg_off, torch::Tensor seg_h,
                      torch::Tensor run_off, torch::Tensor y_t,
                      torch::Tensor a_run) {
    TORCH_CHECK(delta16.is_cuda() && delta16.dtype() == torch::kFloat16);
    TORCH_CHECK(delta16.size(-1) == P_POINTS);
    TORCH_CHECK(dall.dtype() == torch::kFloat32);
    TORCH_CHECK(a_run.dtype() == torch::kBFloat16 && a_run.is_contiguous()
                && a_run.dim() == 2 && a_run.size(1) == P_POINTS,
                "a_run must be a contiguous (max_run, P) bf16 scratch");
    TORCH_CHECK(y_t.is_cuda() && y_t.scalar_type() == torch::kInt64
                && y_t.numel() == 1, "y_t must be a (1,) int64 tensor");
    const int C = delta16.size(0);
    const int H = delta16.size(1);
    TORCH_CHECK(run_off.scalar_type() == torch::kInt32
                && run_off.is_contiguous() && run_off.numel() == C + 1,
                "run_off must be (C+1,) int32");
    const int max_run = a_run.size(0);
    if (max_run == 0) return;
    auto stream = c10::hip::getCurrentHIPStream();
    hipLaunchKernelGGL(pairops::pair_dsum_es_cls_kernel,
                       dim3((max_run + 15) / 16), dim3(BLOCK), 0,
                       stream.stream(),
                       reinterpret_cast<const _Float16*>(
                           delta16.data_ptr()),
                       dall.data_ptr<float>(),
                       pair_c.data_ptr<int>(), pair_neg.data_ptr<int>(),
                       seg_off.data_ptr<int>(), seg_h.data_ptr<int>(),
                       run_off.data_ptr<int>(),
                       reinterpret_cast<const long long*>(
                           y_t.data_ptr<int64_t>()),
                       reinterpret_cast<hip_bfloat16*>(a_run.data_ptr()),
                       max_run, C, H);
}

// y_t absent: all groups from the full (K, P) operand a16.
// Otherwise class y_t[0]'s groups from the one-class scratch operand
// (a16 = a_run), on a grid of 4 * max_grp blocks, one per tile.
void pair_gemm_pbn(torch::Tensor a16, torch::Tensor egw,
                   torch::Tensor vmask, torch::Tensor pair_c,
                   torch::Tensor grp, torch::Tensor pm,
                   torch::Tensor pinv,
                   c10::optional<torch::Tensor> cls_grp_off_o,
                   c10::optional<torch::Tensor> run_off_o,
                   c10::optional<torch::Tensor> y_t_o,
                   int64_t max_grp) {
    TORCH_CHECK(a16.is_cuda() && a16.dtype() == torch::kBFloat16
                && a16.is_contiguous() && a16.size(1) == P_POINTS);
    TORCH_CHECK(egw.dtype() == torch::kBFloat16 && egw.is_contiguous());
    TORCH_CHECK(pm.dtype() == torch::kFloat32 && pm.is_contiguous()
                && pm.dim() == 2, "pm must be contiguous (K, H) fp32");
    const int K = pm.size(0);
    const int H = pm.size(1);
    const int C = egw.size(0);
    TORCH_CHECK(pinv.dtype() == torch::kFloat32 && pinv.is_contiguous()
                && pinv.numel() == K, "pinv must be (K,) fp32");
    TORCH_CHECK(K % 128 == 0 && pair_c.numel() == K
                && vmask.size(0) == K, "pair cache needs 128-pair tiles");
    TORCH_CHECK(egw.size(1) == 2 * H && 2 * H <= 272,
                "pair cache covers the fused route only (2H <= 272)");
    TORCH_CHECK(grp.scalar_type() == torch::kInt32 && grp.is_contiguous()
                && grp.numel() >= 2, "grp must be the (G+1,) tile groups");
    const bool one_class = y_t_o.has_value();
    int nblk = grp.numel() - 1;
    const int* cgo = nullptr;
    const int* roff = nullptr;
    const long long* yp = nullptr;
    if (one_class) {
        TORCH_CHECK(cls_grp_off_o.has_value() && run_off_o.has_value(),
                    "one-class mode needs cls_grp_off and run_off");
        const torch::Tensor& y_t = *y_t_o;
        const torch::Tensor& cls_grp_off = *cls_grp_off_o;
        const torch::Tensor& run_off = *run_off_o;
        TORCH_CHECK(y_t.is_cuda() && y_t.scalar_type() == torch::kInt64
                    && y_t.numel() == 1, "y_t must be a (1,) int64 tensor");
        TORCH_CHECK(cls_grp_off.scalar_type() == torch::kInt32
                    && cls_grp_off.is_contiguous()
                    && cls_grp_off.numel() == C + 1
                    && run_off.scalar_type() == torch::kInt32
                    && run_off.is_contiguous()
                    && run_off.numel() == C + 1,
                    "cls_grp_off / run_off must be (C+1,) int32");
        TORCH_CHECK(max_grp >= 1 && max_grp <= nblk);
        nblk = (int)max_grp * PBN_GRP_TILES;   // one block per tile
        cgo = cls_grp_off.data_ptr<int>();
        roff = run_off.data_ptr<int>();
        yp = reinterpret_cast<const long long*>(y_t.data_ptr<int64_t>());
    } else {
        TORCH_CHECK(a16.size(0) == K, "full build needs the (K, P) operand");
    }
    const size_t shmem = (size_t)2 * H * BSTRIDE * sizeof(hip_bfloat16);
    const int JT = (2 * H + 15) / 16;
    auto stream = c10::hip::getCurrentHIPStream();
    auto launch = [&](auto kern) {
        hipLaunchKernelGGL(kern, dim3(nblk), dim3(BLOCK2), shmem,
                           stream.stream(),
                           reinterpret_cast<const hip_bfloat16*>(
                               a16.data_ptr()),
                           reinterpret_cast<const hip_bfloat16*>(
                               egw.data_ptr()),
                           reinterpret_cast<const unsigned*>(
                               vmask.data_ptr<int>()),
                           pair_c.data_ptr<int>(), (int)vmask.size(1),
                           grp.data_ptr<int>(), cgo, roff, yp,
                           pm.data_ptr<float>(), pinv.data_ptr<float>(),
                           C, H);
    };
    if (JT <= 4) launch(pairops::pair_gemm_pbn128_kernel<4>);
    else if (JT <= 8) launch(pairops::pair_gemm_pbn128_kernel<8>);
    else if (JT <= 16) launch(pairops::pair_gemm_pbn128_kernel<16>);
    else launch(pairops::pair_gemm_pbn128_kernel<17>);
}

// run_off (C+1,) + run_live (C,) int32, both or neither: class c's rows
// from run_off[c] + run_live[c] to the end of its run are padding (the
// base row's pm / inv under an all-zero vmask); tiles' all-pad chunks
// are then filled from the base row instead of being read.
torch::Tensor pair_entropy_cached(torch::Tensor pm, torch::Tensor pinv,
                                  torch::Tensor vmask,
                                  torch::Tensor pair_c,
                                  torch::Tensor pi_hat,
                                  torch::Tensor pbest_before,
                                  torch::Tensor mixture0,
                                  c10::optional<torch::Tensor> run_off_o,
                                  c10::optional<torch::Tensor> run_live_o) {
    TORCH_CHECK(pm.is_cuda() && pm.dtype() == torch::kFloat32
                && pm.is_contiguous() && pm.dim() == 2);
    const int K = pm.size(0);
    const int H = pm.size(1);
    TORCH_CHECK(K % 128 == 0 && 2 * H <= 272,
                "pair cache covers the fused route only");
    TORCH_CHECK(pinv.is_contiguous() && pinv.numel() == K
                && pair_c.numel() == K && vmask.size(0) == K);
    TORCH_CHECK(vmask.is_contiguous() && vmask.size(1) <= EWMAX);
    TORCH_CHECK(mixture0.numel() == H && mixture0.is_contiguous()
                && pbest_before.is_contiguous()
                && pbest_before.size(1) == H
                && pi_hat.is_contiguous());
    TORCH_CHECK(run_off_o.has_value() == run_live_o.has_value(),
                "run_off and run_live go together");
    const int* roff = nullptr;
    const int* rlive = nullptr;
    if (run_off_o.has_value()) {
        const torch::Tensor& run_off = *run_off_o;
        const torch::Tensor& run_live = *run_live_o;
        const int64_t C = pbest_before.size(0);
        TORCH_CHECK(run_off.is_cuda() && run_live.is_cuda()
                    && run_off.scalar_type() == torch::kInt32
                    && run_live.scalar_type() == torch::kInt32
                    && run_off.is_contiguous() && run_live.is_contiguous()
                    && run_off.numel() == C + 1 && run_live.numel() == C,
                    "run_off (C+1,) / run_live (C,) must be int32");
        roff = run_off.data_ptr<int>();
        rlive = run_live.data_ptr<int>();
    }
    auto h_after = torch::empty({K}, pi_hat.options());
    if (K == 0) return h_after;
    const size_t shmem = ((size_t)32 * pairops::pair_ent_stride(H)
                          + 3 * H + 1) * sizeof(float);
    auto stream = c10::hip::getCurrentHIPStream();
    hipLaunchKernelGGL(pairops::pair_entropy_cached_kernel,
                       dim3(K / (32 * ECH)), dim3(BLOCK), shmem,
                       stream.stream(),
                       pm.data_ptr<float>(), pinv.data_ptr<float>(),
                       reinterpret_cast<const unsigned*>(
                           vmask.data_ptr<int>()),
                       pair_c.data_ptr<int>(), (int)vmask.size(1),
                       pi_hat.data_ptr<float>(),
                       pbest_before.data_ptr<float>(),
                       mixture0.data_ptr<float>(), roff, rlive,
                       h_after.data_ptr<float>(), H);
    return h_after;
}

torch::Tensor pair_eig_finalize(torch::Tensor h_after,
                                torch::Tensor h_base,
                                torch::Tensor pair_c,
                                torch::Tensor cand_off,
                                torch::Tensor cand_ck,
                                torch::Tensor cand_ids,
                                torch::Tensor adjusted,
                                torch::Tensor row_sums,
                                double H_before) {
    const int B = cand_ids.size(0);
    const int C = adjusted.size(1);
    TORCH_CHECK(h_base.is_contiguous() && h_base.size(0) == C);
    TORCH_CHECK(cand_ck.scalar_type() == torch::kInt64,
                "cand_ck must be the packed int64 hit table");
    TORCH_CHECK(cand_ids.is_contiguous() && cand_off.is_contiguous()
                && cand_ck.is_contiguous(),
                "finalize inputs must be contiguous");
    auto q = torch::empty({B}, adjusted.options());
    if (B == 0) return q;
    (void)pair_c;   // the packed hit table carries each pair's class
    TORCH_CHECK(cand_off.numel() == B + 1 && cand_ck.numel() < INT_MAX);
    // The kernel's first hit load is unconditional, on an index clamped
    // into the table, and a lane without a hit gathers h_after[0] and
    // column 0 of its row (values it never uses): both must exist. With
    // no hit at all the load reads cand_ids' first entry instead (B >= 1
    // int64, discarded likewise) - nothing is allocated here, so the
    // call captures.
    TORCH_CHECK(h_after.numel() >= 1 && C >= 1,
                "finalize needs at least one pair and one class");
    const int nhits = cand_ck.numel() ? (int)cand_ck.numel() : 1;
    const long long* ckp = cand_ck.numel()
        ? reinterpret_cast<const long long*>(cand_ck.data_ptr<int64_t>())
        : reinterpret_cast<const long long*>(cand_ids.data_ptr<int64_t>());
    auto stream = c10::hip::getCurrentHIPStream();
    const int nblk = std::min((B + 3) / 4, FIN_MAX_BLOCKS);
    auto launch = [&](auto kern, size_t shmem) {
        hipLaunchKernelGGL(kern, dim3(nblk), dim3(BLOCK), shmem,
                           stream.stream(),
                           h_after.data_ptr<float>(),
                           h_base.data_ptr<float>(),
                           cand_off.data_ptr<int>(),
                           ckp, cand_ids.data_ptr<long>(),
                           adjusted.data_ptr<float>(),
                           row_sums.data_ptr<float>(),
                           (float)H_before, q.data_ptr<float>(), B, C,
                           nhits);
    };
    if (C < 4)
        launch(pairops::pair_eig_finalize_kernel<true, false>,
               (size_t)C * sizeof(float));
    else if (C <= FIN_LDS_MAX_C)
        launch(pairops::pair_eig_finalize_kernel<true, true>,
               (size_t)C * sizeof(float));
    else
        launch(pairops::pair_eig_finalize_kernel<false, true>, 0);
    return q;
}

void acq_select(torch::Tensor q0, torch::Tensor h0, torch::Tensor active,
                torch::Tensor qbuf, torch::Tensor out,
                torch::Tensor ties,
                c10::optional<torch::Tensor> topk_o,
                c10::optional<torch::Tensor> group_of_o,
                int64_t n_groups) {
    TORCH_CHECK(q0.is_cuda() && q0.dtype() == torch::kFloat32
                && q0.is_contiguous(), "q0 must be contiguous fp32");
    TORCH_CHECK(h0.dtype() == torch::kFloat32 && h0.numel() == 1);
    TORCH_CHECK(active.dtype() == torch::kBool && active.is_contiguous()
                && active.numel() == q0.numel());
    TORCH_CHECK(qbuf.dtype() == torch::kFloat32 && qbuf.is_contiguous()
                && qbuf.numel() == q0.numel());
    TORCH_CHECK(out.dtype() == torch::kFloat64 && out.is_contiguous()
                && out.numel() == 3);
    TORCH_CHECK(ties.dtype() == torch::kInt64 && ties.is_contiguous()
                && ties.numel() >= 2, "ties buffer too small");
    const int cap = ties.numel() - 1;
    const int B = q0.numel();
    // batch outputs: everything is checked before the first launch
    const bool want_topk = topk_o.has_value() && topk_o->defined();
    const bool grouped = group_of_o.has_value() && group_of_o->defined();
    TORCH_CHECK(want_topk || !grouped, "group_of needs a topk buffer");
    int K = 0, G = 0;
    if (want_topk) {
        const auto& topk = *topk_o;
        TORCH_CHECK(B >= 1, "topk needs at least one candidate");
        TORCH_CHECK(topk.dtype() == torch::kInt64 && topk.is_contiguous()
                    && topk.dim() == 1, "topk must be contiguous int64");
        TORCH_CHECK(topk.numel() >= 1 && topk.numel() <= TOPK_MAX,
                    "topk holds 1 to ", TOPK_MAX, " slots");
        K = topk.numel();
        for (const torch::Tensor* t : std::initializer_list<
                 const torch::Tensor*>{&h0, &active, &qbuf, &out, &ties,
                                       &topk})
            TORCH_CHECK(t->device() == q0.device(),
                        "every acq_select tensor lives on q0's device");
        if (grouped) {
            const auto& gof = *group_of_o;
            TORCH_CHECK(gof.dtype() == torch::kInt32 && gof.is_contiguous()
                        && gof.numel() == B,
                        "group_of must be contiguous int32 (B,)");
            TORCH_CHECK(gof.device() == q0.device(),
                        "every acq_select tensor lives on q0's device");
            TORCH_CHECK(n_groups >= 1 && n_groups <= INT_MAX,
                        "n_groups must be at least 1 with group_of");
            G = (int)n_groups;
        }
    }
    auto pmax = torch::empty({ACQ_GRID}, q0.options());
    auto pidx = torch::empty({ACQ_GRID},
                             q0.options().dtype(torch::kInt32));
    auto stream = c10::hip::getCurrentHIPStream();
    hipLaunchKernelGGL(pairops::acq_select_part_kernel, dim3(ACQ_GRID),
                       dim3(BLOCK), 0, stream.stream(),
                       q0.data_ptr<float>(), h0.data_ptr<float>(),
                       active.data_ptr<bool>(), qbuf.data_ptr<float>(),
                       pmax.data_ptr<float>(), pidx.data_ptr<int>(), B);
    hipLaunchKernelGGL(pairops::acq_select_combine_kernel, dim3(1),
                       dim3(ACQ_GRID), 0, stream.stream(),
                       pmax.data_ptr<float>(), pidx.data_ptr<int>(),
                       out.data_ptr<double>(),
                       reinterpret_cast<long long*>(
                           ties.data_ptr<int64_t>()));
    hipLaunchKernelGGL(pairops::acq_select_ties_kernel, dim3(ACQ_GRID),
                       dim3(BLOCK), 0, stream.stream(),
                       qbuf.data_ptr<float>(), active.data_ptr<bool>(),
                       out.data_ptr<double>(),
                       reinterpret_cast<long long*>(
                           ties.data_ptr<int64_t>()),
                       cap, B);
    C10_HIP_CHECK(hipGetLastError());
    if (!want_topk) return;

    auto iopt = q0.options().dtype(torch::kInt32);
    auto lopt = q0.options().dtype(torch::kInt64);
    auto ws = torch::empty({TOPK_WS_INTS}, iopt);
    auto sel = torch::empty({TOPK_MAX}, lopt);
    auto gbest = torch::empty({grouped ? G : 1}, lopt);
    int* wsp = ws.data_ptr<int>();
    auto* selp = reinterpret_cast<unsigned long long*>(
        sel.data_ptr<int64_t>());
    auto* gbp = reinterpret_cast<unsigned long long*>(
        gbest.data_ptr<int64_t>());
    const float* qp = qbuf.data_ptr<float>();
    const bool* ap = active.data_ptr<bool>();
    // survivors: the group winners, or every candidate
    const unsigned long long* keys = grouped ? gbp : nullptr;
    const int n = grouped ? G : B;
    hipLaunchKernelGGL(pairops::topk_prep_kernel, dim3(ACQ_GRID),
                       dim3(BLOCK), 0, stream.stream(), wsp, gbp,
                       grouped ? G : 0);
    if (grouped)
        hipLaunchKernelGGL(pairops::topk_group_kernel, dim3(ACQ_GRID),
                           dim3(BLOCK), 0, stream.stream(), qp, ap,
                           group_of_o->data_ptr<int>(), gbp, G, B);
    for (int p = 0; p < TOPK_PASSES; ++p)
        hipLaunchKernelGGL(pairops::topk_hist_kernel, dim3(ACQ_GRID),
                           dim3(BLOCK), 0, stream.stream(), keys, qp, ap,
                           wsp, p, K, n);
    hipLaunchKernelGGL(pairops::topk_gather_kernel, dim3(ACQ_GRID),
                       dim3(BLOCK), 0, stream.stream(), keys, qp, ap, wsp,
                       selp, K, n);
    hipLaunchKernelGGL(pairops::topk_sort_kernel, dim3(1), dim3(TOPK_MAX),
                       0, stream.stream(), selp, wsp, qp,
                       reinterpret_cast<long long*>(
                           topk_o->data_ptr<int64_t>()), K);
    C10_HIP_CHECK(hipGetLastError());
}

torch::Tensor pair_gemm_entropy_cls(torch::Tensor a16, torch::Tensor egw,
                                    torch::Tensor pair_b,
                                    torch::Tensor pair_c,
                                    torch::Tensor cls,
                                    torch::Tensor pi_hat,
                                    torch::Tensor pbest_before,
                                    torch::Tensor mixture0) {
    // wide-H pools (no v-select bitmask): 128x128 M-writing GEMM + the
    // cls-based entropy pass; any 2H (memory-bound by the (K, 2H) M
    // workspace)
    TORCH_CHECK(a16.is_cuda() && a16.dtype() == torch::kBFloat16);
    const int K = a16.size(0);
    const int H = mixture0.size(0);
    TORCH_CHECK(K % 128 == 0, "cls route needs 128-pair tiles");
    const int twoH = 2 * H;
    auto mout = torch::empty({(long)K, (long)twoH}, a16.options());
    auto h_after = torch::empty({K}, pi_hat.options());
    auto stream = c10::hip::getCurrentHIPStream();
    const size_t shmem = 4 * 128 * WSTRIDE * sizeof(hip_bfloat16);
    dim3 grid(K / 128, (twoH + 127) / 128);
    hipLaunchKernelGGL(pairops::pair_gemm_wide_kernel, grid, dim3(BLOCK),
                       shmem, stream.stream(),
                       reinterpret_cast<const hip_bfloat16*>(
                           a16.data_ptr()),
                       reinterpret_cast<const hip_bfloat16*>(
                           egw.data_ptr()),
                       pair_c.data_ptr<int>(),
                       reinterpret_cast<hip_bfloat16*>(mout.data_ptr()),
                       twoH);
    hipLaunchKernelGGL(pairops::pair_entropy_wide_cls_kernel,
                       dim3((K + 3) / 4), dim3(BLOCK), 0, stream.stream(),
                       reinterpret_cast<const hip_bfloat16*>(
                           mout.data_ptr()),
                       cls.data_ptr<int>(), pair_b.data_ptr<int>(),
                       pair_c.data_ptr<int>(), pi_hat.data_ptr<float>(),
                       pbest_before.data_ptr<float>(),
                       mixture0.data_ptr<float>(),
                       h_after.data_ptr<float>(), K, H);
    return h_after;
}

torch::Tensor mfma_probe(torch::Tensor a, torch::Tensor bt) {
    TORCH_CHECK(a.sizes() == torch::IntArrayRef({16, 32}));
    TORCH_CHECK(bt.sizes() == torch::IntArrayRef({16, 32}));
    auto out = torch::zeros({16, 16}, a.options());
    auto stream = c10::hip::getCurrentHIPStream();
    hipLaunchKernelGGL(pairops::mfma_probe_kernel, dim3(1), dim3(64), 0,
                       stream.stream(), a.data_ptr<float>(),
                       bt.data_ptr<float>(), out.data_ptr<float>());
    return out;
}

void register_pair_ops(pybind11::module_& m) {
    m.def("pair_dsum_es", &pair_dsum_es,
          "v3 pair A-operand: 2^(summed delta curves) -> (K, P) bf16");
    m.def("pair_gemm_entropy", &pair_gemm_entropy,
          "v3 fused pairing MFMA GEMM + entropy epilogue -> (K,)",
          pybind11::arg("a16"), pybind11::arg("egw"),
          pybind11::arg("vmask"), pybind11::arg("pair_c"),
          pybind11::arg("pi_hat"),
          pybind11::arg("pbest_before"), pybind11::arg("mixture0"),
          pybind11::arg("tile"), pybind11::arg("ablate") = 0,
          pybind11::arg("grp") = torch::Tensor());
    m.def("pair_gemm_entropy_cls", &pair_gemm_entropy_cls,
          "v3 wide-H pairing GEMM + cls-based entropy -> (K,)");
    m.def("pair_dsum_es_cls", &pair_dsum_es_cls,
          "pair A-operand of ONE class (id read on device) into the "
          "(max_run, P) scratch operand");
    m.def("pair_gemm_pbn", &pair_gemm_pbn,
          "pair-cache build (all groups) / one-class refresh: selected "
          "pairing masses pm (K, H) and inv (K,)",
          pybind11::arg("a16"), pybind11::arg("egw"),
          pybind11::arg("vmask"), pybind11::arg("pair_c"),
          pybind11::arg("grp"), pybind11::arg("pm"),
          pybind11::arg("pinv"),
          pybind11::arg("cls_grp_off") = pybind11::none(),
          pybind11::arg("run_off") = pybind11::none(),
          pybind11::arg("y_t") = pybind11::none(),
          pybind11::arg("max_grp") = 0);
    m.def("pair_entropy_cached", &pair_entropy_cached,
          "per-step entropy pass over the pair cache -> (K,), bit-equal "
          "to the fused 128-pair kernel; run_off + run_live skip the "
          "all-pad chunks",
          pybind11::arg("pm"), pybind11::arg("pinv"),
          pybind11::arg("vmask"), pybind11::arg("pair_c"),
          pybind11::arg("pi_hat"), pybind11::arg("pbest_before"),
          pybind11::arg("mixture0"),
          pybind11::arg("run_off") = pybind11::none(),
          pybind11::arg("run_live") = pybind11::none());
    m.def("pair_eig_finalize", &pair_eig_finalize,
          "v3 per-candidate EIG assembly (deterministic) -> (B,)");
    m.def("acq_select", &acq_select,
          "fused acquisition epilogue: qbuf = active ? h0+q0 : -inf; "
          "out(f64[3]) = [masked max, first argmax, isclose tie count]; "
          "topk (K,) int64, when given, = the K best in rank order, one "
          "per group with group_of, -1 padded",
          pybind11::arg("q0"), pybind11::arg("h0"),
          pybind11::arg("active"), pybind11::arg("qbuf"),
          pybind11::arg("out"), pybind11::arg("ties"),
          pybind11::arg("topk") = pybind11::none(),
          pybind11::arg("group_of") = pybind11::none(),
          pybind11::arg("n_groups") = 0);
    m.def("mfma_probe", &mfma_probe,
          "16x16x32 bf16 MFMA fragment-layout probe");
}
