// CDNA4 (gfx950) HIP kernel: fused prediction-pool ingest.
//
// One pass over a host-wire chunk (hc, nc, C) in the file's own dtype
// (fp32 / fp16 / bf16 / fp8-e4m3fn) produces everything the selector
// needs from the pool before its first step:
//   preds_out[h0+h, n0+n, c]   storage-rounded value s (fp32 / bf16 / fp8)
//   preds_t_out[h0+h, c, n0+n] optional class-major mirror of s
//   classes_out[h0+h, n0+n]    lowest index of max_c float(s)
//   ens_out[n0+n, c]          += float(s) over h ascending (adds only)
// replacing the three generic torch passes (.to(storage), the chunked
// init_model_stats up-cast, permute().contiguous()) and their fp32
// transients.
//
// Decomposition: a block owns a tile of TN consecutive points. For a fixed
// model h the tile's TN*C elements are ONE contiguous run in the wire
// chunk, in preds_out and in ens_out, so phase 1 is a flat coalesced
// stream whatever C is (C=3 streams as well as C=1000); thread t always
// owns the same flat elements, so the fp32 consensus accumulator sits in
// LDS with fixed ownership - no atomics, no cross-thread traffic, and
// the h-ascending add chain of the contract is kept literally. Phase 1
// also drops the storage-rounded tile into a padded LDS tile; phase 2
// reads it back twice: a wave per point for the argmax (xor ladder with
// the lowest-index tie rule), and point-fastest for the mirror so that
// preds_t gets TN-element contiguous runs along n.
//
// The tile row pitch is an odd multiple of 16 B: the point-fastest
// mirror read then walks 16 distinct banks for 16 points instead of
// hitting one.
//
// Two instantiations per dtype pair: V=4 (C % 4 == 0 and 16-B aligned
// bases: every tile run starts on a 4-element boundary, so 4-element
// vector loads/stores never straddle a row) and V=1 (any C, any
// alignment - odd C with 1- and 2-byte elements lands here).
//
// The fp8 / bf16 encoders are the integer round-to-nearest-even
// sequences torch's CPU conversion uses, so stored bytes match the
// legacy loader's bit for bit, fp8 subnormals (below 2^-6 - most of a
// softmax row at C >= 64) included.

#include <torch/extension.h>
#include <hip/hip_runtime.h>
#include <c10/hip/HIPStream.h>
#include <c10/util/Optional.h>
#include <cstdint>
#include <climits>
#include <type_traits>

namespace {

constexpr int kIngestThreads = 512;
constexpr int kIngestMaxTN = 64;
// two blocks per CU out of the 160 KB LDS
constexpr int kIngestLdsBudget = 80 * 1024;

struct F32 {
    using T = float;
    static __device__ __forceinline__ float dec(T x) { return x; }
    static __device__ __forceinline__ T enc(float x) { return x; }
};

struct F16 {  // wire only
    using T = uint16_t;
    static __device__ __forceinline__ float dec(T x) {
        return (float)__builtin_bit_cast(_Float16, x);
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

template <typename W>
void launch_storage(const IngestArgs& a, torch::ScalarType st) {
    if (st == torch::kFloat32) launch_vec<W, F32>(a);
    else if (st == torch::kBFloat16) launch_vec<W, BF16>(a);
    else launch_vec<W, FP8>(a);
}

bool aligned16(const void* p) {
    return (reinterpret_cast<uintptr_t>(p) & 15u) == 0;
}

}  // namespace

void ingest_chunk(torch::Tensor wire, int64_t h0, int64_t n0,
                  torch::Tensor preds_out, torch::Tensor classes_out,
                  torch::Tensor ens_out,
                  c10::optional<torch::Tensor> preds_t_out) {
    TORCH_CHECK(wire.is_cuda() && wire.is_contiguous() && wire.dim() == 3,
                "wire must be a contiguous (hc, nc, C) tensor on a ROCm device");
    TORCH_CHECK(preds_out.is_cuda() && preds_out.is_contiguous()
                && preds_out.dim() == 3,
                "preds_out must be a contiguous (Hl, N, C) device tensor");
    const auto wt = wire.scalar_type();
    const auto st = preds_out.scalar_type();
    TORCH_CHECK(wt == torch::kFloat32 || wt == torch::kFloat16
                || wt == torch::kBFloat16 || wt == torch::kFloat8_e4m3fn,
                "wire dtype must be fp32/fp16/bf16/fp8-e4m3fn");
    TORCH_CHECK(st == torch::kFloat32 || st == torch::kBFloat16
                || st == torch::kFloat8_e4m3fn,
                "storage dtype must be fp32/bf16/fp8-e4m3fn");
    const int64_t hc = wire.size(0), nc = wire.size(1), C = wire.size(2);
    const int64_t Hl = preds_out.size(0), N = preds_out.size(1);
    TORCH_CHECK(preds_out.size(2) == C, "class count mismatch");
    TORCH_CHECK(h0 >= 0 && n0 >= 0 && h0 + hc <= Hl && n0 + nc <= N,
                "chunk [", h0, ":", h0 + hc, ") x [", n0, ":", n0 + nc,
                ") outside the (", Hl, ", ", N, ") pool");
    TORCH_CHECK(classes_out.is_cuda() && classes_out.is_contiguous()
                && classes_out.scalar_type() == torch::kInt64
                && classes_out.dim() == 2 && classes_out.size(0) == Hl
                && classes_out.size(1) == N,
                "classes_out must be a contiguous (Hl, N) int64 device tensor");
    TORCH_CHECK(ens_out.is_cuda() && ens_out.is_contiguous()
                && ens_out.scalar_type() == torch::kFloat32
                && ens_out.dim() == 2 && ens_out.size(0) == N
                && ens_out.size(1) == C,
                "ens_out must be a contiguous (N, C) fp32 device tensor");
    void* pt = nullptr;
    if (preds_t_out.has_value()) {
        const auto& t = *preds_t_out;
        TORCH_CHECK(t.is_cuda() && t.is_contiguous() && t.scalar_type() == st
                    && t.dim() == 3 && t.size(0) == Hl && t.size(1) == C
                    && t.size(2) == N,
                    "preds_t_out must be a contiguous (Hl, C, N) device "
                    "tensor in the storage dtype");
        pt = t.data_ptr();
    }
    if (hc == 0 || nc == 0 || C == 0) return;
    TORCH_CHECK(hc < INT_MAX && nc < INT_MAX && Hl < INT_MAX,
                "chunk dimensions exceed int range");

    TORCH_CHECK(C <= kIngestLdsBudget / 4,
                "ingest_chunk: C=", C, " does not fit one point in LDS");

    const int elem = (int)preds_out.element_size();
    const int row_bytes = tile_row_bytes((int)C, elem);
    auto lds_for = [&](int tn) {
        return round_up16(tn * (int)C * 4) + tn * row_bytes;
    };
    // largest power-of-two tile (<= the chunk) whose accumulator + padded
    // tile fit the budget
    int TN = kIngestMaxTN, logTN = 6;
    while (TN > 1 && ((TN >> 1) >= nc || lds_for(TN) > kIngestLdsBudget)) {
        TN >>= 1;
        --logTN;
    }
    const int lds = lds_for(TN);
    TORCH_CHECK(lds <= kIngestLdsBudget,
                "ingest_chunk: C=", C, " needs ", lds,
                " B of LDS per point, over the ", kIngestLdsBudget,
                " B budget");

    IngestArgs a;
    a.wire = wire.data_ptr();
    a.preds = preds_out.data_ptr();
    a.preds_t = pt;
    a.classes = reinterpret_cast<long long*>(classes_out.data_ptr<int64_t>());
    a.ens = ens_out.data_ptr<float>();
    a.hc = (int)hc; a.nc = (int)nc; a.C = (int)C;
    a.N = N; a.h0 = (int)h0; a.n0 = n0;
    a.TN = TN; a.logTN = logTN; a.RS = row_bytes / elem;
    a.blocks = (int)((nc + TN - 1) / TN);
    a.lds = (int)lds;
    a.vec = (C % 4 == 0) && aligned16(a.wire) && aligned16(a.preds)
            && aligned16(a.ens);
    a.stream = c10::hip::getCurrentHIPStream().stream();

    if (wt == torch::kFloat32) launch_storage<F32>(a, st);
    else if (wt == torch::kFloat16) launch_storage<F16>(a, st);
    else if (wt == torch::kBFloat16) launch_storage<BF16>(a, st);
    else launch_storage<FP8>(a, st);
    C10_HIP_CHECK(hipGetLastError());
}

void register_ingest_ops(pybind11::module_& m) {
    m.def("ingest_chunk", &ingest_chunk,
          "Fused pool ingest: storage rounding + argmax classes + consensus "
          "sum + optional class-major mirror (CDNA4 HIP)",
          pybind11::arg("wire"), pybind11::arg("h0"), pybind11::arg("n0"),
          pybind11::arg("preds_out"), pybind11::arg("classes_out"),
          pybind11::arg("ens_out"),
          pybind11::arg("preds_t_out") = pybind11::none());
}
