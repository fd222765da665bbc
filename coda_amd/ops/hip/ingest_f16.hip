// CDNA4 (gfx950) HIP kernel: fp16 storage instantiations of the fused
// prediction-pool ingest (design: ingest.hip, template: ingest_kernel.h).
//
// fp16 is the dtype the benchmark pools ship in, so fp16 wire -> fp16
// storage is a bit copy and the pool stays lossless at half the fp32
// bytes. From the other wire dtypes the integer encoder F16::enc rounds
// to nearest even exactly as torch's CPU fp32 -> fp16 conversion does,
// in the subnormal range (below 2^-14) and at the 65504 / 65520 overflow
// boundary too.

#include "ingest_kernel.h"

namespace coda_ingest {

void launch_f16_storage(const IngestArgs& a, torch::ScalarType wt) {
    launch_wire<F16>(a, wt);
}

}  // namespace coda_ingest
