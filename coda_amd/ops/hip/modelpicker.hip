// CDNA4 (gfx950) HIP kernel: hit-sparse ModelPicker expected entropy.
//
// ModelPicker scores a point n by the posterior entropy it expects after
// labelling n, averaged over the C hypothesised classes. A class that no
// model predicts on n leaves the posterior where it is, and a class c
// that is hit changes the entropy by a closed form in two sums over the
// models A that predict it (S = sum_A p_h, T = sum_A p_h log2 p_h):
//
//   ent_c - E0 = log2(1 + (g-1) S)
//                - [ (g-1) S E0 + (g-1) T + g log2(g) S ] / (1 + (g-1) S)
//
// S E0 and T nearly cancel (exactly, for a uniform posterior), and the
// result moves by (g-1) times any error in E0. The prologue
// (reference.modelpicker_prologue, fp64 on the (H,) vector) therefore
// hands over the centred q_h = p_h (log2 p_h + E0), and the kernel sums
// T' = sum_A q_h = S E0 + T directly:
//
//   ent_c - E0 = log2(1 + (g-1) S) - [ (g-1) T' + g log2(g) S ] / (1 + (g-1) S)
//
// so dev[n] = sum over the distinct classes hit on n of that term costs
// O(H) per point instead of the dense formula's O(C*H) (see
// coda_amd/baselines/modelpicker.py; entropies[n] = e0 + dev[n] / C).
//
// Static input (ops.modelpicker_build): per point the models sorted by
// predicted class, stable, as one (N, H) int16 row. Bits 0..14 hold the
// model index; bit 15 marks a position whose class differs from the
// previous position's (position 0 carries no mark). Every class's model
// set is then a contiguous segment in a fixed order.
//
// One wave64 owns one point. Lane l owns the R = ceil(H/64) consecutive
// sorted positions [l*R, l*R+R): the wave's R loads cover the row as one
// contiguous run (V positions per load where R and H allow it). The
// block stages (p_h, q_h) in LDS once and then walks points in
// a grid-stride loop, the next row's loads in flight under the current
// row's math. Per point:
//   1. each lane folds its positions into (seen-a-mark, sums since the
//      last mark);
//   2. a segmented inclusive scan on the DPP row_shr/row_bcast ladder
//      (the ladder of wave.h, with the segmented operator) hands each
//      lane the open segment's sums from the lanes before it;
//   3. each lane walks its positions again, closing a segment - one
//      closed-form evaluation - at every mark; the lane that owns
//      position H-1 closes the last one;
//   4. a DPP wave sum yields dev[n].
// A point on which all models agree has one segment and no mark: its
// term is 0 by the identity S = 1, T' = 0 and is written as exactly 0.
// Every sum has one fixed order - no atomics - so two launches are
// bit-equal. The epilogue is fp32 with log1pf: log2(1 + x) through a
// plain v_log_f32 of the rounded 1 + x loses the low bits of a small S.

#include <torch/extension.h>
#include <hip/hip_runtime.h>
#include <c10/hip/HIPStream.h>
#include "wave.h"  // dpp_mov, wave_reduce_sum

namespace mpops {

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / 64;
constexpr int kMaxH = 1024;
constexpr int kMaxR = kMaxH / 64;
constexpr int kMaxBlocks = 2048;   // 8 blocks of 4 waves per CU
constexpr float kInvLn2 = 1.4426950408889634f;

// One ladder step of the segmented scan: (f, s, t) <- moved (+) own with
// (f1, v1) (+) (f2, v2) = (f1 | f2, f2 ? v2 : v1 + v2). A lane without a
// source moves in (0, 0, 0), the identity.
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ void seg_step(int& f, float& s, float& t) {
    const int mf = dpp_mov<CTRL, ROW_MASK>(f);
    const float ms = __int_as_float(dpp_mov<CTRL, ROW_MASK>(__float_as_int(s)));
    const float mt = __int_as_float(dpp_mov<CTRL, ROW_MASK>(__float_as_int(t)));
    s = f ? s : ms + s;
    t = f ? t : mt + t;
    f |= mf;
}

__device__ __forceinline__ void seg_scan(int& f, float& s, float& t) {
    seg_step<0x111, 0xf>(f, s, t);
    seg_step<0x112, 0xf>(f, s, t);
    seg_step<0x114, 0xf>(f, s, t);
    seg_step<0x118, 0xf>(f, s, t);
    seg_step<0x142, 0xa>(f, s, t);
    seg_step<0x143, 0xc>(f, s, t);
}

struct Consts {
    float gm1;   // g - 1
    float glg;   // g log2 g
};

__device__ __forceinline__ float closed_form(float S, float T,
                                             const Consts& k) {
    const float x = k.gm1 * S;
    const float num = fmaf(k.glg, S, k.gm1 * T);
    return log1pf(x) * kInvLn2 - num / (1.0f + x);
}

template <int V> struct RowVec;
template <> struct RowVec<1> { typedef unsigned short type; };
template <> struct RowVec<2> {
    typedef unsigned short type __attribute__((ext_vector_type(2)));
};
template <> struct RowVec<4> {
    typedef unsigned short type __attribute__((ext_vector_type(4)));
};
template <> struct RowVec<8> {
    typedef unsigned short type __attribute__((ext_vector_type(8)));
};

// The lane's R positions of one row. V > 1 needs H % V == 0 (and R % V
// == 0, by construction): every V-group is then wholly inside or wholly
// outside the row and 2V-byte aligned.
template <int R, int V>
__device__ __forceinline__ void load_row(const unsigned short* __restrict__ row,
                                         int j0, int H,
                                         unsigned short (&raw)[R]) {
    if constexpr (V == 1) {
#pragma unroll
        for (int r = 0; r < R; ++r)
            raw[r] = (j0 + r < H) ? row[j0 + r] : (unsigned short)0;
    } else {
        typedef typename RowVec<V>::type vec_t;
#pragma unroll
        for (int g = 0; g < R / V; ++g) {
            vec_t v = {};
            if (j0 + g * V < H)
                v = *reinterpret_cast<const vec_t*>(row + j0 + g * V);
#pragma unroll
            for (int e = 0; e < V; ++e) raw[g * V + e] = v[e];
        }
    }
}

template <int R, int V>
__global__ void __launch_bounds__(kBlock, 4)
modelpicker_dev_kernel(const unsigned short* __restrict__ packed,  // (N, H)
                       const float* __restrict__ p,                // (H,)
                       const float* __restrict__ q,                // (H,)
                       const unsigned char* __restrict__ active,   // (N,)
                       float* __restrict__ dev,                    // (N,)
                       float gm1, float glg, int N, int H) {
    __shared__ float2 s_pq[kMaxH];
    for (int h = threadIdx.x; h < H; h += kBlock)
        s_pq[h] = make_float2(p[h], q[h]);
    __syncthreads();

    Consts k;
    k.gm1 = gm1;
    k.glg = glg;

    const int lane = threadIdx.x & 63;
    const int j0 = lane * R;
    const int last_lane = (H - 1) / R;
    const int stride = gridDim.x * kWaves;
    const float inf = __int_as_float(0x7f800000);

    int n = blockIdx.x * kWaves + (threadIdx.x >> 6);
    unsigned short raw[R], nxt[R];
    bool act = false, act_nxt = false;
    if (n < N) {
        act = active[n] != 0;
        if (act) load_row<R, V>(packed + (size_t)n * H, j0, H, raw);
    }
    for (; n < N; n += stride) {
        const int nn = n + stride;
        act_nxt = false;
        if (nn < N) {
            act_nxt = active[nn] != 0;
            if (act_nxt) load_row<R, V>(packed + (size_t)nn * H, j0, H, nxt);
        }
        if (!act) {
            if (lane == 0) dev[n] = inf;
        } else {
            float pv[R], qv[R];
            // pass 1: (mark seen, sums since the last mark) of my positions
            int f = 0;
            float s = 0.0f, t = 0.0f;
#pragma unroll
            for (int r = 0; r < R; ++r) {
                if (j0 + r < H) {
                    const int m = min((int)(raw[r] & 0x7fff), H - 1);
                    const float2 v = s_pq[m];
                    pv[r] = v.x;
                    qv[r] = v.y;
                    if (raw[r] & 0x8000) {
                        f = 1;
                        s = 0.0f;
                        t = 0.0f;
                    }
                    s += v.x;
                    t += v.y;
                } else {
                    pv[r] = 0.0f;
                    qv[r] = 0.0f;
                }
            }
            // open segment handed over by the lanes before me
            seg_scan(f, s, t);
            int cf = __shfl_up(f, 1, 64);
            float rs = __shfl_up(s, 1, 64);
            float rt = __shfl_up(t, 1, 64);
            if (lane == 0) {
                cf = 0;
                rs = 0.0f;
                rt = 0.0f;
            }
            // pass 2: close a segment at every mark
            float acc = 0.0f;
#pragma unroll
            for (int r = 0; r < R; ++r) {
                if (j0 + r < H) {
                    if (raw[r] & 0x8000) {
                        acc += closed_form(rs, rt, k);
                        rs = 0.0f;
                        rt = 0.0f;
                        cf = 1;
                    }
                    rs += pv[r];
                    rt += qv[r];
                }
            }
            // the last segment; a row without any mark is one class on
            // all models and contributes exactly 0
            if (lane == last_lane && cf) acc += closed_form(rs, rt, k);
            const float total = wave_reduce_sum(acc);
            if (lane == 0) dev[n] = total;
        }
        act = act_nxt;
#pragma unroll
        for (int r = 0; r < R; ++r) raw[r] = nxt[r];
    }
}

struct LaunchArgs {
    const unsigned short* packed;
    const float *p, *q;
    const unsigned char* active;
    float* dev;
    float gm1, glg;
    int N, H, blocks;
    hipStream_t stream;
};

template <int R, int V>
void launch(const LaunchArgs& a) {
    hipLaunchKernelGGL((modelpicker_dev_kernel<R, V>), dim3(a.blocks),
                       dim3(kBlock), 0, a.stream, a.packed, a.p, a.q,
                       a.active, a.dev, a.gm1, a.glg, a.N, a.H);
}

constexpr int vec_width(int R) {
    const int low = R & -R;
    return low > 8 ? 8 : low;
}

template <int R>
void launch_r(const LaunchArgs& a, bool vec) {
    if (vec) launch<R, vec_width(R)>(a);
    else launch<R, 1>(a);
}

}  // namespace mpops

torch::Tensor modelpicker_dev(torch::Tensor packed, torch::Tensor p,
                              torch::Tensor q, double gamma, torch::Tensor active) {
    using namespace mpops;
    TORCH_CHECK(packed.is_cuda() && packed.is_contiguous()
                && packed.dim() == 2
                && packed.scalar_type() == torch::kInt16,
                "packed must be a contiguous (N, H) int16 device tensor");
    const int64_t N = packed.size(0), H = packed.size(1);
    TORCH_CHECK(H >= 1 && H <= kMaxH, "modelpicker_dev: H=", H,
                " outside [1, ", kMaxH, "]");
    TORCH_CHECK(N < (int64_t)INT_MAX - kMaxBlocks * kWaves,
                "modelpicker_dev: N exceeds int range");
    auto vec_ok = [&](const torch::Tensor& t, int64_t len) {
        return t.is_cuda() && t.is_contiguous() && t.dim() == 1
            && t.size(0) == len && t.scalar_type() == torch::kFloat32
            && t.device() == packed.device();
    };
    TORCH_CHECK(vec_ok(p, H) && vec_ok(q, H),
                "p and q must be contiguous (H,) fp32 tensors on packed's "
                "device");
    TORCH_CHECK(active.is_cuda() && active.is_contiguous()
                && active.dim() == 1 && active.size(0) == N
                && active.scalar_type() == torch::kUInt8
                && active.device() == packed.device(),
                "active must be a contiguous (N,) uint8 tensor on packed's "
                "device");
    TORCH_CHECK(gamma > 0.0, "gamma must be positive");
    auto dev = torch::empty({N}, p.options());
    if (N == 0) return dev;

    LaunchArgs a;
    a.packed = reinterpret_cast<const unsigned short*>(
        packed.data_ptr<int16_t>());
    a.p = p.data_ptr<float>();
    a.q = q.data_ptr<float>();
    a.active = active.data_ptr<uint8_t>();
    a.dev = dev.data_ptr<float>();
    a.gm1 = (float)(gamma - 1.0);
    a.glg = (float)(gamma * std::log2(gamma));
    a.N = (int)N;
    a.H = (int)H;
    const int64_t want = (N + kWaves - 1) / kWaves;
    a.blocks = (int)(want < kMaxBlocks ? want : kMaxBlocks);
    a.stream = c10::hip::getCurrentHIPStream().stream();

    const int R = (int)((H + 63) / 64);
    const int V = vec_width(R);
    const bool vec = V > 1 && H % V == 0
        && (reinterpret_cast<uintptr_t>(a.packed) & 15u) == 0;
    switch (R) {
#define MP_CASE(r) case r: launch_r<r>(a, vec); break;
        MP_CASE(1) MP_CASE(2) MP_CASE(3) MP_CASE(4)
        MP_CASE(5) MP_CASE(6) MP_CASE(7) MP_CASE(8)
        MP_CASE(9) MP_CASE(10) MP_CASE(11) MP_CASE(12)
        MP_CASE(13) MP_CASE(14) MP_CASE(15) MP_CASE(16)
#undef MP_CASE
        default: TORCH_CHECK(false, "modelpicker_dev: unsupported H=", H);
    }
    C10_HIP_CHECK(hipGetLastError());
    return dev;
}

void register_modelpicker_ops(pybind11::module_& m) {
    m.def("modelpicker_dev", &modelpicker_dev,
          "hit-sparse ModelPicker entropy deviation per point (N,)",
          pybind11::arg("packed"), pybind11::arg("p"), pybind11::arg("q"),
          pybind11::arg("gamma"),
          pybind11::arg("active"));
}
