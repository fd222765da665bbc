// CDNA4 (gfx950) HIP kernel: fused prediction-pool ingest of LOGITS.
//
// The logits twin of ingest.hip (same outputs, same tile geometry, codecs
// and IngestArgs from ingest_kernel.h): one pass over a host-wire chunk
// (hc, nc, C) of logits in fp32 / fp16 / bf16 applies a per-model
// temperature softmax before the storage rounding. Per model h, point n,
// with k_h = float32(log2(e) / T_h) from the host:
//   m   = max_c x[c]                  fp32, exact
//   t_c = (x[c] - m) * k_h            fp32 (-inf stays -inf)
//   e_c = exp2(t_c)                   native v_exp_f32: a tied maximum is 1
//   Z   = sum_c e_c                   fp32, one fixed order (below)
//   p_c = e_c / Z                     IEEE fp32 divide
//   s_c = S::enc(p_c)                 the storage codecs, unchanged
// and from s on everything is ingest.hip's contract: preds_out and the
// mirror get s, classes_out the lowest-index argmax of float(s), ens_out
// advances by one fp32 add per model, h ascending. v_exp_f32 is a 1-ulp
// unit and flushes results below 2^-126, so the pool is NOT bit-equal to
// the eager twin (reference.ingest_chunk with logit_scale); classes, the
// consensus and the mirror are exact functions of the kernel's own pool.
//
// Stage: ONE fp32 tile in LDS per block (row pitch an odd multiple of
// 16 B, like ingest.hip's storage tile) holds, in turn, the decoded logits
// x, the exponentials e, and the decoded stored values f = float(s); the
// mirror re-encodes f (S::enc(S::dec(s)) == s). With the fp32 consensus
// tile next to it a point costs 8*C + 20 B whatever the storage dtype:
// C = 1000 gives TN = 8 points (64 160 B) for fp32, fp16, bf16 and fp8
// alike, inside the 80 KB budget that lets two blocks share a CU.
//
// Per model: (A) a wave per point loads the point's row into the stage
// (V=4: 4-element vector loads) taking the max, combines it over the
// wave with the xor butterfly, then walks the row again lane-strided
// (class c on lane c % 64, ascending) replacing x by e and summing; the
// butterfly combines the 64 partial sums. The walk reads the stage, not
// the registers of the load, so the order of the sum - and with it every
// output bit - is the same on the vector and the scalar path and for any
// chunking. (B) the flat pass of ingest.hip: thread t owns the same flat
// elements in every model, divides by its point's Z, encodes, stores to
// preds_out with vector stores, advances the consensus tile and leaves f
// in the stage. (C) argmax and mirror as in ingest.hip. No atomics.

#include "ingest_kernel.h"
#include <c10/hip/HIPStream.h>
#include <c10/util/Optional.h>

namespace {

using namespace coda_ingest;

bool aligned16(const void* p) {
    return (reinterpret_cast<uintptr_t>(p) & 15u) == 0;
}

template <typename W, typename S, int V>
__global__ __launch_bounds__(kIngestThreads) void ingest_logits_kernel(
    const typename W::T* __restrict__ wire,
    const float* __restrict__ scale,       // (hc,) log2(e) / T_h
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
    float* stage_s = reinterpret_cast<float*>(
        ingest_smem + round_up16(TN * C * 4));
    float* z_s = stage_s + TN * RS;        // RS * 4 is a multiple of 16

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
        const float k = scale[h];

        // (A) row max, exponentials and their sum: a wave per point
        for (int q = wave; q < tn; q += nwaves) {
            const WT* wrow = wbase + (long long)q * C;
            float* row = stage_s + q * RS;
            float m = -INFINITY;
            for (int cc = lane * V; cc < C; cc += 64 * V) {
                const Vec<WT, V> w =
                    *reinterpret_cast<const Vec<WT, V>*>(wrow + cc);
                Vec<float, V> x;
#pragma unroll
                for (int j = 0; j < V; ++j) {
                    x.v[j] = W::dec(w.v[j]);
                    m = fmaxf(m, x.v[j]);
                }
                *reinterpret_cast<Vec<float, V>*>(row + cc) = x;
            }
#pragma unroll
            for (int off = 32; off > 0; off >>= 1)
                m = fmaxf(m, __shfl_xor(m, off, 64));
            // the row was written by this wave only
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            float z = 0.0f;
            for (int cc = lane; cc < C; cc += 64) {
                const float t = (row[cc] - m) * k;
                const float ex = __builtin_amdgcn_exp2f(t);
                row[cc] = ex;
                z = z + ex;                // ascending cc per lane
            }
#pragma unroll
            for (int off = 32; off > 0; off >>= 1)
                z = z + __shfl_xor(z, off, 64);   // a + b == b + a: all lanes agree
            if (lane == 0) z_s[q] = z;
        }
        __syncthreads();

        // (B) normalise, encode, store, accumulate: flat, fixed ownership
        int p = p_first, c = c_first;
        for (int e = tid * V; e < ne; e += step) {
            float* sp = stage_s + p * RS + c;
            const float z = z_s[p];
            Vec<float, V> ex = *reinterpret_cast<Vec<float, V>*>(sp);
            Vec<float, V> acc = *reinterpret_cast<Vec<float, V>*>(ens_s + e);
            Vec<ST, V> s;
#pragma unroll
            for (int j = 0; j < V; ++j) {
                s.v[j] = S::enc(ex.v[j] / z);
                ex.v[j] = S::dec(s.v[j]);
                acc.v[j] = acc.v[j] + ex.v[j];
            }
            *reinterpret_cast<Vec<float, V>*>(ens_s + e) = acc;
            *reinterpret_cast<Vec<ST, V>*>(obase + e) = s;
            *reinterpret_cast<Vec<float, V>*>(sp) = ex;
            c += dr;
            p += dq;
            if (c >= C) { c -= C; ++p; }
        }
        __syncthreads();

        // (C) argmax on the storage-rounded values, lowest index on ties
        for (int q = wave; q < tn; q += nwaves) {
            const float* row = stage_s + q * RS;
            float bv = -INFINITY;
            int bi = INT_MAX;
            for (int cc = lane; cc < C; cc += 64) {
                const float v = row[cc];
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
                if (q < tn)
                    tbase[(long long)cc * N + q] = S::enc(stage_s[q * RS + cc]);
            }
        }
        __syncthreads();   // stage is rewritten by the next model
    }

    for (int e = tid * V; e < ne; e += step) {
        *reinterpret_cast<Vec<float, V>*>(ens_g + e) =
            *reinterpret_cast<const Vec<float, V>*>(ens_s + e);
    }
}

template <typename W, typename S, int V>
void launch_logits_one(const IngestArgs& a, const float* scale) {
    auto kern = ingest_logits_kernel<W, S, V>;
    if (a.lds > 64 * 1024) {
        C10_HIP_CHECK(hipFuncSetAttribute(
            reinterpret_cast<const void*>(kern),
            hipFuncAttributeMaxDynamicSharedMemorySize, a.lds));
    }
    hipLaunchKernelGGL(kern, dim3(a.blocks), dim3(kIngestThreads), a.lds,
                       a.stream,
                       reinterpret_cast<const typename W::T*>(a.wire), scale,
                       reinterpret_cast<typename S::T*>(a.preds),
                       reinterpret_cast<typename S::T*>(a.preds_t),
                       a.classes, a.ens, a.hc, a.nc, a.C, a.N, a.h0, a.n0,
                       a.TN, a.logTN, a.RS);
}

template <typename W, typename S>
void launch_logits_vec(const IngestArgs& a, const float* scale) {
    if (a.vec) launch_logits_one<W, S, 4>(a, scale);
    else launch_logits_one<W, S, 1>(a, scale);
}

// wire dtype dispatch for one storage codec S; the caller has checked wt
template <typename S>
void launch_logits_wire(const IngestArgs& a, const float* scale,
                        torch::ScalarType wt) {
    if (wt == torch::kFloat32) launch_logits_vec<F32, S>(a, scale);
    else if (wt == torch::kFloat16) launch_logits_vec<F16, S>(a, scale);
    else launch_logits_vec<BF16, S>(a, scale);
}

}  // namespace

void ingest_logits_chunk(torch::Tensor wire, torch::Tensor logit_scale,
                         int64_t h0, int64_t n0,
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
                || wt == torch::kBFloat16,
                "logits wire dtype must be fp32/fp16/bf16");
    TORCH_CHECK(st == torch::kFloat32 || st == torch::kFloat16
                || st == torch::kBFloat16 || st == torch::kFloat8_e4m3fn,
                "storage dtype must be fp32/fp16/bf16/fp8-e4m3fn");
    const int64_t hc = wire.size(0), nc = wire.size(1), C = wire.size(2);
    const int64_t Hl = preds_out.size(0), N = preds_out.size(1);
    TORCH_CHECK(logit_scale.is_cuda() && logit_scale.is_contiguous()
                && logit_scale.scalar_type() == torch::kFloat32
                && logit_scale.dim() == 1 && logit_scale.size(0) == hc
                && logit_scale.device() == wire.device(),
                "logit_scale must be a contiguous (hc,) fp32 tensor on the "
                "wire's device");
    TORCH_CHECK(preds_out.device() == wire.device()
                && classes_out.device() == wire.device()
                && ens_out.device() == wire.device(),
                "all tensors must live on the wire's device");
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
                    && t.size(2) == N && t.device() == wire.device(),
                    "preds_t_out must be a contiguous (Hl, C, N) device "
                    "tensor in the storage dtype");
        pt = t.data_ptr();
    }
    if (hc == 0 || nc == 0 || C == 0) return;
    TORCH_CHECK(hc < INT_MAX && nc < INT_MAX && Hl < INT_MAX,
                "chunk dimensions exceed int range");

    // one point: consensus row + stage row + Z
    TORCH_CHECK(C <= kIngestLdsBudget / 8 - 8,
                "ingest_chunk: C=", C, " does not fit one logits point in LDS");
    const int row_bytes = tile_row_bytes((int)C, 4);
    auto lds_for = [&](int tn) {
        return round_up16(tn * (int)C * 4) + tn * row_bytes + tn * 4;
    };
    // largest power-of-two tile (<= the chunk) whose accumulator + stage
    // fit the budget
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
    a.TN = TN; a.logTN = logTN; a.RS = row_bytes / 4;
    a.blocks = (int)((nc + TN - 1) / TN);
    a.lds = (int)lds;
    a.vec = (C % 4 == 0) && aligned16(a.wire) && aligned16(a.preds)
            && aligned16(a.ens);
    a.stream = c10::hip::getCurrentHIPStream().stream();
    const float* scale = logit_scale.data_ptr<float>();

    if (st == torch::kFloat32) launch_logits_wire<F32>(a, scale, wt);
    else if (st == torch::kFloat16) launch_logits_wire<F16>(a, scale, wt);
    else if (st == torch::kBFloat16) launch_logits_wire<BF16>(a, scale, wt);
    else launch_logits_wire<FP8>(a, scale, wt);
    C10_HIP_CHECK(hipGetLastError());
}

void register_ingest_logits_ops(pybind11::module_& m) {
    m.def("ingest_logits_chunk", &ingest_logits_chunk,
          "Fused logits ingest: temperature softmax + storage rounding + "
          "argmax classes + consensus sum + optional class-major mirror "
          "(CDNA4 HIP)",
          pybind11::arg("wire"), pybind11::arg("logit_scale"),
          pybind11::arg("h0"), pybind11::arg("n0"),
          pybind11::arg("preds_out"), pybind11::arg("classes_out"),
          pybind11::arg("ens_out"),
          pybind11::arg("preds_t_out") = pybind11::none());
}
