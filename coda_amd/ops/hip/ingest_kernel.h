// Shared template of the fused prediction-pool ingest kernel (gfx950):
// dtype codecs, the kernel and its launch helpers. The design notes are in
// ingest.hip, which holds the fp32 / bf16 / fp8 storage instantiations and
// the host entry point; ingest_f16.hip holds the fp16 storage ones. The
// split keeps each translation unit's instantiation count (and compile
// time) bounded.
#pragma once

#include <torch/extension.h>
#include <hip/hip_runtime.h>
#include <c10/hip/HIPException.h>
#include <cstdint>
#include <climits>
#include <type_traits>

namespace coda_ingest {

constexpr int kIngestThreads = 512;
constexpr int kIngestMaxTN = 64;
// two blocks per CU out of the 160 KB LDS
constexpr int kIngestLdsBudget = 80 * 1024;

struct F32 {
    using T = float;
    static __device__ __forceinline__ float dec(T x) { return x; }
    static __device__ __forceinline__ T enc(float x) { return x; }
};

struct F16 {  // IEEE binary16 (bias 15)
    using T = uint16_t;
    static __device__ __forceinline__ float dec(T x) {
        return (float)__builtin_bit_cast(_Float16, x);
    }
    // integer round-to-nearest-even, independent of the wave's rounding
    // and denormal modes
    static __device__ __forceinline__ T enc(float x) {
        uint32_t u = __float_as_uint(x);
        const uint32_t sign = u & 0x80000000u;
        u ^= sign;
        uint32_t r;
        if (u > 0x7f800000u) {             // NaN
            r = 0x7e00u;
        } else if (u >= (143u << 23)) {    // >= 65536 (and inf)
            r = 0x7c00u;
        } else if (u < (113u << 23)) {     // below 2^-14: fp16 subnormal
            // adding 0.5 leaves the 10 subnormal mantissa bits (units of
            // 2^-24) in the low bits of the fp32 sum, rounded to nearest
            // even by the add; a round-up to 2^-14 carries into the
            // exponent field, which is the right encoding
            const uint32_t magic = 126u << 23;
            const float f = __uint_as_float(u) + __uint_as_float(magic);
            r = __float_as_uint(f) - magic;
        } else {
            // a mantissa carry moves up the exponent; [65520, 65536)
            // lands on 0x7c00 = inf
            const uint32_t odd = (u >> 13) & 1u;
            u += ((uint32_t)(15 - 127) << 23) + 0xfffu;
            u += odd;
            r = u >> 13;
        }
        return (T)(r | (sign >> 16));
    }
};

struct BF16 {
    using T = uint16_t;
    static __device__ __forceinline__ float dec(T x) {
        return __uint_as_float((uint32_t)x << 16);
    }
    // round-to-nearest-even on the dropped 16 bits (finite inputs)
    static __device__ __forceinline__ T enc(float x) {
        uint32_t u = __float_as_uint(x);
        if ((u & 0x7fffffffu) > 0x7f800000u) return 0x7fc0;
        u += ((u >> 16) & 1u) + 0x7fffu;
        return (T)(u >> 16);
    }
};

struct FP8 {  // OCP e4m3fn (bias 7, no infinities)
    using T = uint8_t;
    static __device__ __forceinline__ float dec(T x) {
        const uint32_t sign = ((uint32_t)x & 0x80u) << 24;
        const uint32_t em = x & 0x7fu;
        float mag;
        if (em >= 8u) {
            mag = __uint_as_float((em << 20) + (120u << 23));
        } else {
            // subnormal m * 2^-9 as 2^-6 * (1 + m/8) - 2^-6: exact, and no
            // multiply that could contract into the consensus add
            mag = __uint_as_float((em << 20) + (121u << 23)) - 0.015625f;
        }
        return __uint_as_float(__float_as_uint(mag) | sign);
    }
    static __device__ __forceinline__ T enc(float x) {
        uint32_t u = __float_as_uint(x);
        const uint32_t sign = u & 0x80000000u;
        u ^= sign;
        uint32_t r;
        if (u >= (1087u << 20)) {          // >= 480: past the last finite
            r = 0x7fu;
        } else if (u < (121u << 23)) {     // below 2^-6: fp8 subnormal
            // adding 2^14 leaves the 3 subnormal mantissa bits in the low
            // bits of the fp32 sum, rounded to nearest even by the add
            const uint32_t magic = 141u << 23;
            const float f = __uint_as_float(u) + __uint_as_float(magic);
            r = __float_as_uint(f) - magic;
        } else {
            const uint32_t odd = (u >> 20) & 1u;
            u += ((uint32_t)(7 - 127) << 23) + 0x7ffffu;
            u += odd;
            r = u >> 20;
        }
        return (T)(r | (sign >> 24));
    }
};

template <typename T, int V>
struct alignas(sizeof(T) * V) Vec {
    T v[V];
};

__host__ __device__ inline int round_up16(int x) { return (x + 15) & ~15; }

// Row pitch of the LDS tile in bytes: an odd multiple of 16.
inline int tile_row_bytes(int C, int elem) {
    int rb = round_up16(C * elem);
    if (((rb / 16) & 1) == 0) rb += 16;
    return rb;
}

template <typename W, typename S, int V>
__global__ __launch_bounds__(kIngestThreads) void ingest_kernel(
    const typename W::T* __restrict__ wire,
    typename S::T* __restrict__ preds,
    typename S::T* __restrict__ preds_t,   // may be null
    long long* __restrict__ classes,
    float* __restrict__ ens,
    int hc, int nc, int C, long long N, int h0, long long n0,
    int TN, int logTN, int RS) {
    using WT = typename W::T;
    using ST = typename S::T;
    extern __shared__ __align__(16) unsigned char ingest_smem[];
    float* ens_s = reinterpret_cast<float*>(ingest_smem);
    ST* tile_s = reinterpret_cast<ST*>(ingest_smem + round_up16(TN * C * 4));

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int nwaves = blockDim.x >> 6;
    const int pn = blockIdx.x * TN;        // first point of the tile (chunk-local)
    const int tn = min(TN, nc - pn);
    if (tn <= 0) return;
    const int ne = tn * C;                 // multiple of V (V=4 needs C % 4 == 0)
    const int step = blockDim.x * V;

    float* ens_g = ens + (n0 + pn) * (long long)C;
    for (int e = tid * V; e < ne; e += step) {
        *reinterpret_cast<Vec<float, V>*>(ens_s + e) =
            *reinterpret_cast<const Vec<float, V>*>(ens_g + e);
    }
    // thread t touches the same ens_s elements in every loop below:
    // no barrier is needed for the accumulator

    const int dq = step / C, dr = step % C;
    const int p_first = (tid * V) / C, c_first = (tid * V) % C;

    for (int h = 0; h < hc; ++h) {
        const WT* wbase = wire + ((long long)h * nc + pn) * C;
        ST* obase = preds + (((long long)(h0 + h)) * N + n0 + pn) * C;
        int p = p_first, c = c_first;
        for (int e = tid * V; e < ne; e += step) {
            const Vec<WT, V> w = *reinterpret_cast<const Vec<WT, V>*>(wbase + e);
            Vec<float, V> acc = *reinterpret_cast<Vec<float, V>*>(ens_s + e);
            Vec<ST, V> s;
#pragma unroll
            for (int j = 0; j < V; ++j) {
                if constexpr (std::is_same<W, S>::value) {
                    s.v[j] = w.v[j];   // finite values round-trip exactly
                } else {
                    s.v[j] = S::enc(W::dec(w.v[j]));
                }
                acc.v[j] = acc.v[j] + S::dec(s.v[j]);
            }
            *reinterpret_cast<Vec<float, V>*>(ens_s + e) = acc;
            *reinterpret_cast<Vec<ST, V>*>(obase + e) = s;
            *reinterpret_cast<Vec<ST, V>*>(tile_s + p * RS + c) = s;
            c += dr;
            p += dq;
            if (c >= C) { c -= C; ++p; }
        }
        __syncthreads();

        // argmax on the storage-rounded values, lowest index on ties
        for (int q = wave; q < tn; q += nwaves) {
            const ST* row = tile_s + q * RS;
            float bv = -INFINITY;
            int bi = INT_MAX;
            for (int cc = lane; cc < C; cc += 64) {
                const float v = S::dec(row[cc]);
                if (v > bv) { bv = v; bi = cc; }   // ascending cc: first max stays
            }
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) {
                const float ov = __shfl_xor(bv, off, 64);
                const int oi = __shfl_xor(bi, off, 64);
                if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
            }
            if (lane == 0)
                classes[(long long)(h0 + h) * N + n0 + pn + q] = bi;
        }

        if (preds_t != nullptr) {
            ST* tbase = preds_t + (long long)(h0 + h) * C * N + n0 + pn;
            const int total = C << logTN;
            for (int i = tid; i < total; i += blockDim.x) {
                const int q = i & (TN - 1);
                const int cc = i >> logTN;
                if (q < tn) tbase[(long long)cc * N + q] = tile_s[q * RS + cc];
            }
        }
        __syncthreads();   // tile is rewritten by the next model
    }

    for (int e = tid * V; e < ne; e += step) {
        *reinterpret_cast<Vec<float, V>*>(ens_g + e) =
            *reinterpret_cast<const Vec<float, V>*>(ens_s + e);
    }
}

struct IngestArgs {
    const void* wire;
    void* preds;
    void* preds_t;
    long long* classes;
    float* ens;
    int hc, nc, C;
    long long N;
    int h0;
    long long n0;
    int TN, logTN, RS, blocks, lds;
    bool vec;
    hipStream_t stream;
};

template <typename W, typename S, int V>
void launch_one(const IngestArgs& a) {
    auto kern = ingest_kernel<W, S, V>;
    if (a.lds > 64 * 1024) {
        C10_HIP_CHECK(hipFuncSetAttribute(
            reinterpret_cast<const void*>(kern),
            hipFuncAttributeMaxDynamicSharedMemorySize, a.lds));
    }
    hipLaunchKernelGGL(kern, dim3(a.blocks), dim3(kIngestThreads), a.lds,
                       a.stream,
                       reinterpret_cast<const typename W::T*>(a.wire),
                       reinterpret_cast<typename S::T*>(a.preds),
                       reinterpret_cast<typename S::T*>(a.preds_t),
                       a.classes, a.ens, a.hc, a.nc, a.C, a.N, a.h0, a.n0,
                       a.TN, a.logTN, a.RS);
}

template <typename W, typename S>
void launch_vec(const IngestArgs& a) {
    if (a.vec) launch_one<W, S, 4>(a);
    else launch_one<W, S, 1>(a);
}

// wire dtype dispatch for one storage codec S; the caller has checked wt
template <typename S>
void launch_wire(const IngestArgs& a, torch::ScalarType wt) {
    if (wt == torch::kFloat32) launch_vec<F32, S>(a);
    else if (wt == torch::kFloat16) launch_vec<F16, S>(a);
    else if (wt == torch::kBFloat16) launch_vec<BF16, S>(a);
    else launch_vec<FP8, S>(a);
}

// fp16 storage instantiations (ingest_f16.hip)
void launch_f16_storage(const IngestArgs& a, torch::ScalarType wt);

}  // namespace coda_ingest
