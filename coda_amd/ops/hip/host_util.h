// Host-side helpers of the pbest / table / label bindings: argument
// checks, the storage-dtype dispatch and the v1 launch geometry.
#pragma once

#include <torch/extension.h>
#include <hip/hip_runtime.h>
#include <c10/hip/HIPStream.h>
#include <hip/hip_bfloat16.h>
#include <hip/hip_fp8.h>  // __hip_fp8_e4m3 (OCP = torch.float8_e4m3fn)
#include <type_traits>
#include "beta_grid.h"

static inline void check_f32_cuda(const torch::Tensor& t, const char* name) {
    TORCH_CHECK(t.is_cuda(), name, " must be on a ROCm device");
    TORCH_CHECK(t.scalar_type() == torch::kFloat32, name, " must be fp32");
    TORCH_CHECK(t.is_contiguous(), name, " must be contiguous");
}

// (R, H) Beta rows of the v1 phase kernels
static inline void check_beta_rows(const torch::Tensor& alpha,
                                   const torch::Tensor& beta) {
    check_f32_cuda(alpha, "alpha");
    check_f32_cuda(beta, "beta");
    TORCH_CHECK(alpha.dim() == 2 && alpha.sizes() == beta.sizes(),
                "alpha/beta must be (R, H)");
}

// the H-coupling term a phase-2 kernel reads: one 256-point row per
// P(best) row
static inline void check_slog2(const torch::Tensor& slog2, int64_t rows) {
    check_f32_cuda(slog2, "slog2");
    TORCH_CHECK(slog2.dim() == 2 && slog2.size(0) == rows &&
                slog2.size(1) == P_POINTS,
                "slog2 must be (R, 256), R = ", rows);
}

// (H, C) diagonal Betas + the (B, H) int32 argmax classes of the v1 EIG
// kernels (stage_hyp indexes cls[b * H + h] and alpha_t[c * H + h])
static inline void check_hyp_inputs(const torch::Tensor& alpha_cc,
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

// cls of the v2 assemble kernels: (B, H) int32 next to m (C, B, 2H)
static inline void check_cls_for_m(const torch::Tensor& m,
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

// Storage-dtype dispatch: f(typed pointer to t's data) for a prediction
// pool held as fp32, bf16, fp16 or fp8 (e4m3fn); `unsupported` is the
// error for any other dtype. f is a generic lambda [&](auto* p) that
// launches the kernel instantiated for elem_t<decltype(p)>.
template <typename P>
using elem_t = std::remove_pointer_t<P>;

template <typename F>
static inline void dispatch_storage(const torch::Tensor& t,
                                    const char* unsupported, F&& f) {
    switch (t.scalar_type()) {
    case torch::kFloat32: f(t.data_ptr<float>()); break;
    case torch::kBFloat16:
        f(reinterpret_cast<hip_bfloat16*>(t.data_ptr())); break;
    case torch::kFloat16:
        f(reinterpret_cast<_Float16*>(t.data_ptr())); break;
    case torch::kFloat8_e4m3fn:
        f(reinterpret_cast<__hip_fp8_e4m3*>(t.data_ptr())); break;
    default: TORCH_CHECK(false, unsupported);
    }
}

// The v2 m / es tensors: bf16, else fp32 (data_ptr<float> rejects the rest).
template <typename F>
static inline void dispatch_bf16_f32(const torch::Tensor& t, F&& f) {
    if (t.scalar_type() == torch::kBFloat16)
        f(reinterpret_cast<hip_bfloat16*>(t.data_ptr()));
    else
        f(t.data_ptr<float>());
}

// Launch kern over grid with BLOCK threads and smem bytes of dynamic LDS
// on the current stream.
template <typename K, typename... Args>
static inline void launch(K kern, dim3 grid, size_t smem, Args... args) {
    hipLaunchKernelGGL(kern, grid, dim3(BLOCK), smem,
                       c10::hip::getCurrentHIPStream().stream(), args...);
    C10_HIP_CHECK(hipGetLastError());
}

// One wave per row, ROWS_PER_BLOCK rows per workgroup.
static inline int row_blocks(int R) {
    return (R + ROWS_PER_BLOCK - 1) / ROWS_PER_BLOCK;
}

// LDS of the v1 kernels' staged Beta rows. per row: lnB (f64 H) + a, b,
// pb (f32 H each)
constexpr size_t lds_bytes(int H) {
    return (size_t)ROWS_PER_BLOCK * ((size_t)H * 8 + 3 * (size_t)H * 4);
}

// v1 launch geometry for R rows of H staged models: blocks along x and
// the dynamic LDS, held to the CU's 160 KiB. hname names H in the error.
struct V1Geometry {
    int blocks;
    size_t smem;
};
static inline V1Geometry v1_geometry(int R, int H, const char* hname = "H") {
    const size_t smem = lds_bytes(H);
    TORCH_CHECK(smem <= 160 * 1024, hname, " too large for LDS: ", H);
    return {row_blocks(R), smem};
}
