"""What the HIP extension exports, read from the sources as text (CPU).

The ops live in several translation units, each with its own
register_*_ops; an m.def lost or doubled in a move would only show up on
a GPU, as an AttributeError or an import failure. This reads the names
given to m.def across coda_amd/ops/hip/*.hip and holds them to the list
below, and holds every call through the extension handle in the package,
the tests, the scripts and the benchmark to that list. No compiler.
"""
import glob
import os
import re

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

EXPORTS = [
    "acq_select",
    "beta_row_tables",
    "col_add",
    "dirichlet_add",
    "eig_assemble_k",
    "eig_chunk",
    "eig_entropy",
    "eig_phase1",
    "eig_phase2",
    "eig_totals",
    "es_build",
    "es_build_gathered",
    "ingest_chunk",
    "ingest_logits_chunk",
    "mfma_probe",
    "mixture_entropy",
    "modelpicker_dev",
    "pair_dsum_es",
    "pair_dsum_es_cls",
    "pair_eig_finalize",
    "pair_entropy_cached",
    "pair_gemm_entropy",
    "pair_gemm_entropy_cls",
    "pair_gemm_pbn",
    "pbest_from_beta",
    "pbest_phase1",
    "pbest_phase1_wide",
    "pbest_phase2",
    "pbest_phase2_wide",
    "pi_hat_delta",
    "pi_hat_delta_part",
    "pi_hat_delta_t_part",
    "pi_marginal",
    "table_commit_cols",
    "table_commit_row",
]

# ops of the stand-alone probe module that scripts/pi_marginal_probe.py
# builds from scripts/pi_marginal_probe.hip; no shipped source has them
PROBE_ONLY = {"pim_twostage", "pim_atomic"}

DEF = re.compile(r'\bm\.def\(\s*"(\w+)"')
CALL = re.compile(r"\b_?ext\.(\w+)\(")


def _read(path):
    with open(path, encoding="utf-8") as f:
        return f.read()


def _defined():
    names = []
    for src in sorted(glob.glob(
            os.path.join(REPO, "coda_amd", "ops", "hip", "*.hip"))):
        names += DEF.findall(_read(src))
    return names


def test_extension_exports():
    # no m.def lost, none doubled
    names = _defined()
    assert sorted(set(names)) == sorted(names), \
        sorted(n for n in set(names) if names.count(n) > 1)
    assert len(EXPORTS) == 35 and EXPORTS == sorted(set(EXPORTS))
    assert sorted(names) == EXPORTS
    assert not PROBE_ONLY & set(names)

    # every call through the extension handle names an export
    files = [os.path.join(REPO, "bench.py")]
    for top in ("coda_amd", "tests", "scripts"):
        files += glob.glob(os.path.join(REPO, top, "**", "*.py"),
                           recursive=True)
    known = set(EXPORTS) | PROBE_ONLY
    seen, unknown = set(), []
    for path in files:
        for name in CALL.findall(_read(path)):
            seen.add(name)
            if name not in known:
                unknown.append((os.path.relpath(path, REPO), name))
    assert not unknown, unknown
    assert len(seen & set(EXPORTS)) > 20   # the pattern does find the calls
