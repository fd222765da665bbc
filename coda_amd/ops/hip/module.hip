// The extension module: what _coda_hip exports, one register call per
// source. Each register_*_ops holds the m.def lines of its own file.

#include <torch/extension.h>

void register_pbest_ops(pybind11::module_& m);   // pbest.hip (v1 engine)
void register_table_ops(pybind11::module_& m);   // table.hip (v2 engine)
void register_label_ops(pybind11::module_& m);   // label.hip (label update)
void register_pair_ops(pybind11::module_& m);    // pair.hip (v3 engine)
void register_ingest_ops(pybind11::module_& m);  // ingest.hip (pool ingest)
void register_ingest_logits_ops(pybind11::module_& m);  // ingest_logits.hip
void register_modelpicker_ops(pybind11::module_& m);    // modelpicker.hip

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
    m.doc() = "coda_amd fused gfx950 kernels";
    register_pbest_ops(m);
    register_table_ops(m);
    register_label_ops(m);
    register_pair_ops(m);
    register_ingest_ops(m);
    register_ingest_logits_ops(m);
    register_modelpicker_ops(m);
}
