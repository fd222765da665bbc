// Wave64 cross-lane primitives (gfx950), shared by every kernel source:
// the GCN DPP row_shr/row_bcast ladder. Each step is one VALU op at 1-2
// cycle dependent latency, against ~50 cycles per dependent ds_bpermute
// round of a __shfl ladder.
// dpp_ctrl: row_shr:N = 0x110|N, row_bcast15 = 0x142, row_bcast31 = 0x143.
#pragma once

#include <hip/hip_runtime.h>

// moved-in value; 0 where the lane has no source or its row is masked
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ int dpp_mov(int x) {
    return __builtin_amdgcn_update_dpp(0, x, CTRL, ROW_MASK, 0xf, true);
}

template <int CTRL, int ROW_MASK>
__device__ __forceinline__ float dpp_add(float x) {
    return x + __int_as_float(dpp_mov<CTRL, ROW_MASK>(__float_as_int(x)));
}

// Wave64 inclusive add-scan in 6 DPP ops.
__device__ __forceinline__ float wave_inclusive_scan(float v) {
    v = dpp_add<0x111, 0xf>(v);  // row_shr:1
    v = dpp_add<0x112, 0xf>(v);  // row_shr:2
    v = dpp_add<0x114, 0xf>(v);  // row_shr:4
    v = dpp_add<0x118, 0xf>(v);  // row_shr:8  (rows of 16 complete)
    v = dpp_add<0x142, 0xa>(v);  // row_bcast:15 -> rows 1, 3
    v = dpp_add<0x143, 0xc>(v);  // row_bcast:31 -> rows 2, 3
    return v;
}

// Wave64 sum, in every lane.
__device__ __forceinline__ float wave_reduce_sum(float v) {
    return __int_as_float(__builtin_amdgcn_readlane(
        __float_as_int(wave_inclusive_scan(v)), 63));
}

// Sum over each row of 16 lanes, in all 16 lanes of the row.
__device__ __forceinline__ float row16_reduce(float v) {
    v = dpp_add<0x111, 0xf>(v);  // row_shr:1
    v = dpp_add<0x112, 0xf>(v);  // row_shr:2
    v = dpp_add<0x114, 0xf>(v);  // row_shr:4
    v = dpp_add<0x118, 0xf>(v);  // row_shr:8 -> lane15 of each row
    return __shfl(v, 15, 16);    // broadcast row total to all 16 lanes
}

// Sum over each aligned group of 8 lanes, valid in the group's LAST lane
// only. With v[m] = x[2m+1] + x[2m] this is row16_reduce's tree over the
// 16 values x, level for level: its first row_shr:1 step forms exactly
// those pair sums in the odd lanes, and the last lane of a group reads
// nothing from outside the group.
__device__ __forceinline__ float row8_reduce_last(float v) {
    v = dpp_add<0x111, 0xf>(v);  // row_shr:1
    v = dpp_add<0x112, 0xf>(v);  // row_shr:2
    v = dpp_add<0x114, 0xf>(v);  // row_shr:4 -> lanes 7 and 15 of each row
    return v;
}
