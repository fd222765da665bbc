// CDNA4 (gfx950) HIP kernel: fused prediction-pool ingest.
//
// One pass over a host-wire chunk (hc, nc, C) in the file's own dtype
// (fp32 / fp16 / bf16 / fp8-e4m3fn) produces everything the selector
// needs from the pool before its first step:
//   preds_out[h0+h, n0+n, c]   storage-rounded value s (fp32/fp16/bf16/fp8)
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
// The fp8 / bf16 / fp16 encoders are the integer round-to-nearest-even
// sequences torch's CPU conversion uses, so stored bytes match the
// legacy loader's bit for bit, subnormals included (fp8 below 2^-6 - most
// of a softmax row at C >= 64; fp16 below 2^-14 - most of one at C=1000).
//
// The kernel template and the codecs live in ingest_kernel.h. This file
// instantiates the fp32 / bf16 / fp8 storage kernels; the fp16 storage
// ones are compiled in ingest_f16.hip.

#include "ingest_kernel.h"
#include <c10/hip/HIPStream.h>
#include <c10/util/Optional.h>

namespace {

using namespace coda_ingest;

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
    TORCH_CHECK(st == torch::kFloat32 || st == torch::kFloat16
                || st == torch::kBFloat16 || st == torch::kFloat8_e4m3fn,
                "storage dtype must be fp32/fp16/bf16/fp8-e4m3fn");
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

    if (st == torch::kFloat32) launch_wire<F32>(a, wt);
    else if (st == torch::kFloat16) launch_f16_storage(a, wt);
    else if (st == torch::kBFloat16) launch_wire<BF16>(a, wt);
    else launch_wire<FP8>(a, wt);
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
