"""Batch acquisition on the CPU: the numpy contract (tests/acq_topk_ref.py)
against an independent pure-Python ranking, the eager torch twin against
the contract, the mutations the generated cases must see, and the selector,
harness and serving layers above them. Every comparison is exact.
"""
from __future__ import annotations

import functools
import os
import random
import sqlite3

import numpy as np
import pytest
import torch

from tests import acq_topk_ref as TR

from coda_amd import CODA, Oracle, ops
from coda_amd.datasets import (Dataset, make_synthetic_task,
                               write_synthetic_task)
from coda_amd.options import LOSS_FNS

CASES = TR.all_cases()


# ---------------------------------------------------------------------
# 1. the contract against sorted() over tuples
# ---------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _python_ranking(case) -> tuple:
    """Every competing candidate's slot word, best first, with no numpy
    in the ordering: Python floats compare -0.0 == 0.0 and order the
    infinities, tuples break ties by position."""
    qbuf = case.qbuf
    vals = qbuf.tolist()
    bits = qbuf.view(np.uint32).tolist()
    act = case.active.tolist()
    cand = [(-vals[i], i) for i in range(case.B) if act[i]]
    if case.group_of is not None:
        g = case.group_of.tolist()
        best = {}
        for key in cand:
            if g[key[1]] not in best or key < best[g[key[1]]]:
                best[g[key[1]]] = key
        cand = list(best.values())
    return tuple((i << 32) | bits[i] for _, i in sorted(cand))


def _python_slots(case, K: int) -> list:
    r = _python_ranking(case)[:K]
    return list(r) + [-1] * (K - len(r))


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_contract_against_sorted(case):
    for K in case.ks:
        got = TR.ref_of(case, K)
        assert got.dtype == np.int64 and got.shape == (K,)
        assert got.tolist() == _python_slots(case, K), (case.name, K)


def test_cases_cover_what_they_claim():
    kinds = {c.kind for c in CASES}
    assert {"acq", "group", "cut", "zero", "inf", "few", "none",
            "sweep"} <= kinds
    for c in CASES:
        if c.group_of is not None:
            assert c.group_of.dtype == np.int32
            assert 0 <= c.group_of.min() and c.group_of.max() < c.G
    # the cut cases: exactly K - 1, K, K + 1 equal maxima, on both sides
    # of a slice boundary
    for c in TR.cut_cases():
        K = c.ks[0]
        q = c.qbuf
        top = np.flatnonzero(q == q.max())
        assert top.size in (K - 1, K, K + 1)
        per = TR.AR.per_block(c.B)
        assert len({int(p) // per for p in top}) >= 2 or top.size == 1
    # the padding is checked to the last slot
    few = [c for c in CASES if c.kind in ("few", "none")]
    assert any(TR.ref_of(c, 1024)[-1] == -1 for c in few)
    assert all((TR.ref_of(c, 1024) == -1).all() for c in CASES
               if c.kind == "none")
    # -inf entries ranked behind the finite ones, then padding
    c = next(c for c in CASES if c.name == "neg-inf-B300")
    pos, vals = TR.unpack(TR.ref_of(c, 64))
    assert pos.size == 30 and vals[0] == np.inf
    assert np.isfinite(vals[1:11]).all() and (vals[11:] == -np.inf).all()
    assert (np.diff(pos[11:]) > 0).all()


# ---------------------------------------------------------------------
# 2. the eager twin
# ---------------------------------------------------------------------

@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_eager_twin_is_the_contract(case):
    q = torch.from_numpy(case.qbuf)
    active = torch.from_numpy(case.active)
    group_of = None if case.group_of is None \
        else torch.from_numpy(case.group_of)
    for K in case.ks:
        pos, vals = ops.reference.acq_topk(q, active, group_of, K)
        assert pos.dtype == torch.int64 and vals.dtype == torch.float32
        got = np.full(K, -1, dtype=np.int64)
        got[:pos.numel()] = (pos.numpy() << 32) \
            | vals.numpy().view(np.uint32).astype(np.int64)
        assert np.array_equal(got, TR.ref_of(case, K)), (case.name, K)


# ---------------------------------------------------------------------
# 3. mutation floors
# ---------------------------------------------------------------------

@pytest.mark.parametrize("mutate", TR.MUTATIONS)
def test_cases_see_the_mutation(mutate):
    seen = []
    for c in CASES:
        if c.B > 10_000:
            continue            # the small cases must suffice
        for K in c.ks:
            bad = TR.select(c.qbuf, c.active, c.group_of, K, mutate)
            if not np.array_equal(bad, TR.ref_of(c, K)):
                seen.append((c.name, K))
                break
    print(f"{mutate}: seen by {len(seen)} cases, e.g. {seen[:3]}")
    assert seen, f"no generated case can tell '{mutate}' from the contract"


# ---------------------------------------------------------------------
# 4. the selector
# ---------------------------------------------------------------------

def _selector(H, N, C, seed, **kw):
    preds, labels = make_synthetic_task(H=H, N=N, C=C, seed=seed)
    ds = Dataset.from_tensors(preds, labels, "cpu")
    random.seed(0)
    torch.manual_seed(0)
    return CODA(ds, chunk_size=64, **kw), Oracle(ds, LOSS_FNS["acc"])


def _contract_batch(sel, k, distinct):
    """The contract applied to eig_batched()'s scores and the candidates'
    class rows."""
    q, cand = sel.eig_batched()
    cand = list(cand)
    q = q.numpy()
    rows = sel.classes[:, cand].t().numpy()
    group_of = None
    if distinct:
        _, group_of = np.unique(rows, axis=0, return_inverse=True)
        group_of = group_of.reshape(-1).astype(np.int32)
    slots = TR.select(q, np.ones(len(cand), dtype=bool), group_of, k)
    pos, vals = TR.unpack(slots)
    return [(cand[p], float(v)) for p, v in zip(pos.tolist(), vals)], rows


SHAPES = [(8, 300, 5, 0), (3, 200, 4, 7), (6, 400, 4, 1)]


@pytest.mark.parametrize("H,N,C,seed", SHAPES)
@pytest.mark.parametrize("distinct", [True, False])
def test_selector_batches_are_the_contract(H, N, C, seed, distinct):
    sel, oracle = _selector(H, N, C, seed)
    labeled = set()
    for rnd in range(3):
        k = (4, 7, 16)[rnd]
        want, _ = _contract_batch(sel, k, distinct)
        state = random.getstate()
        stochastic = sel.stochastic
        got = sel.get_next_items_to_label(k, distinct=distinct)
        assert random.getstate() == state
        assert sel.stochastic == stochastic
        assert got == want, (rnd, got, want)
        ids = [i for i, _ in got]
        assert len(set(ids)) == len(ids) and not set(ids) & labeled
        assert all(i in sel.unlabeled_idxs for i in ids)
        rows = {tuple(sel.classes[:, i].tolist()) for i in ids}
        if distinct:
            assert len(rows) == len(ids)    # one pick per pattern
        sel.add_labels(ids, [oracle(i) for i in ids], [p for _, p in got])
        labeled |= set(ids)
        assert sel.labeled_idxs[-len(ids):] == ids
    nxt = sel.get_next_items_to_label(8, distinct=distinct)
    assert not {i for i, _ in nxt} & labeled


def test_fewer_patterns_than_k():
    """H = 3, C = 4: at most 64 patterns, fewer among 200 points."""
    sel, _ = _selector(3, 200, 4, 7)
    cand = list(sel._active_candidates)
    patterns = {tuple(sel.classes[:, i].tolist()) for i in cand}
    assert len(patterns) < 100 < len(cand)
    got = sel.get_next_items_to_label(100)
    assert len(got) == len(patterns)
    assert {tuple(sel.classes[:, i].tolist()) for i, _ in got} == patterns
    # regardless of pattern: the 100 best, with repeats among them
    flat = sel.get_next_items_to_label(100, distinct=False)
    assert len(flat) == 100
    want, rows = _contract_batch(sel, 100, False)
    assert flat == want
    assert len({tuple(sel.classes[:, i].tolist()) for i, _ in flat}) < 100
    qs = [q for _, q in flat]
    assert qs == sorted(qs, reverse=True)


def test_k1_is_the_single_pick():
    a, _ = _selector(8, 300, 5, 0)
    b, _ = _selector(8, 300, 5, 0)
    random.seed(5)
    one = a.get_next_item_to_label()
    state_a = random.getstate()
    random.seed(5)
    batch = b.get_next_items_to_label(1)
    assert batch == [one]
    assert random.getstate() == state_a
    assert a.stochastic == b.stochastic


def test_k1_keeps_the_seeded_tie_break():
    """A doubled pool: every point has an exact copy, so the maximum is
    tied and k = 1 draws from the RNG as the single pick does, while
    k = 2 draws nothing and takes the lower point id first."""
    preds, labels = make_synthetic_task(H=5, N=120, C=4, seed=3)
    preds = torch.cat([preds, preds], dim=1).contiguous()
    labels = torch.cat([labels, labels])
    sels = []
    for _ in range(2):
        ds = Dataset.from_tensors(preds, labels, "cpu")
        random.seed(0)
        torch.manual_seed(0)
        sels.append(CODA(ds, chunk_size=64))
    a, b = sels
    random.seed(11)
    one = a.get_next_item_to_label()
    state_a = random.getstate()
    random.seed(11)
    assert b.get_next_items_to_label(1) == [one]
    assert random.getstate() == state_a
    assert a.stochastic and b.stochastic
    b.stochastic = False
    random.seed(11)
    state = random.getstate()
    two = b.get_next_items_to_label(2, distinct=False)
    assert random.getstate() == state and not b.stochastic
    assert two[0][1] == two[1][1] and two[1][0] == two[0][0] + 120
    # per pattern, the copy is the same pattern: it does not compete
    two = b.get_next_items_to_label(2)
    assert two[1][0] != two[0][0] + 120


@pytest.mark.parametrize("k", [0, 1025, -3])
def test_k_out_of_range(k):
    sel, _ = _selector(4, 60, 3, 2)
    with pytest.raises(ValueError):
        sel.get_next_items_to_label(k)


def test_other_acquisitions_have_no_batch():
    sel, _ = _selector(4, 60, 3, 2, q="uncertainty")
    assert len(sel.get_next_items_to_label(1)) == 1
    with pytest.raises(NotImplementedError):
        sel.get_next_items_to_label(2)


def test_supports_batch_flag():
    from coda_amd.base import ModelSelector
    from coda_amd.baselines import IID
    assert ModelSelector.supports_batch is False
    assert IID.supports_batch is False and CODA.supports_batch is True


def test_model_sharded_ranks_refuse_distinct():
    """A process holding a shard of the model axis cannot see patterns."""
    sel, _ = _selector(4, 60, 3, 2)

    class Sharded:
        is_distributed = True
    sel.comm = Sharded()
    assert not sel._replicated
    with pytest.raises(ValueError, match="distinct=False"):
        sel.get_next_items_to_label(2)


# ---------------------------------------------------------------------
# 5. the harness
# ---------------------------------------------------------------------

@pytest.fixture()
def task_dir(tmp_path):
    write_synthetic_task(str(tmp_path / "data"), name="synthtask",
                         H=6, N=200, C=4, seed=0)
    return tmp_path


def _run_cli(tmp_path, extra):
    import main as harness
    from coda_amd import tracking
    cwd = os.getcwd()
    os.chdir(tmp_path)
    try:
        tracking.set_tracking_uri("sqlite:///coda.sqlite")
        tracking._EXPERIMENT = None
        tracking._RUN_STACK.clear()
        harness.main(["--task", "synthtask", "--data-dir", "data",
                      "--device", "cpu", "--chunk-size", "64"] + extra)
    finally:
        os.chdir(cwd)


def _metric(tmp_path, exp, key):
    conn = sqlite3.connect(str(tmp_path / "coda.sqlite"))
    rows = conn.execute(
        "SELECT m.step, m.value FROM metrics m "
        "JOIN runs r ON m.run_uuid=r.run_uuid "
        "JOIN experiments e ON r.experiment_id=e.experiment_id "
        "WHERE e.name=? AND m.key=? ORDER BY m.step", (exp, key)).fetchall()
    conn.close()
    return rows


def _params(tmp_path, exp):
    conn = sqlite3.connect(str(tmp_path / "coda.sqlite"))
    rows = conn.execute(
        "SELECT p.key, p.value FROM params p "
        "JOIN runs r ON p.run_uuid=r.run_uuid "
        "JOIN experiments e ON r.experiment_id=e.experiment_id "
        "WHERE e.name=?", (exp,)).fetchall()
    conn.close()
    return dict(rows)


def test_batch_run_holds_the_regret_inside_a_round(task_dir, capsys):
    _run_cli(task_dir, ["--method", "coda", "--iters", "10", "--seeds", "1",
                        "--batch-size", "4", "--experiment-name", "b4"])
    out = capsys.readouterr().out
    r0 = float(out.split("Regret at 0:")[1].split()[0])
    regret = _metric(task_dir, "b4", "regret")
    assert [s for s, _ in regret] == list(range(1, 11))
    v = [x for _, x in regret]
    # rounds of 4, 4, 2: the labels before a round's last carry the
    # previous round's regret
    assert v[0] == v[1] == v[2] == pytest.approx(r0, abs=0)
    assert v[4] == v[5] == v[6] == v[3]
    assert v[8] == v[7]
    cum = [x for _, x in _metric(task_dir, "b4", "cumulative regret")]
    assert cum == pytest.approx(np.cumsum(v).tolist(), rel=1e-12)
    secs = [x for _, x in _metric(task_dir, "b4", "step_seconds")]
    assert len(secs) == 10
    assert secs[0] == secs[1] == secs[2] == secs[3]
    assert secs[8] == secs[9]
    assert _params(task_dir, "b4")["batch_size"] == "4"

    # what the rounds' last rows must hold: the same selector driven by
    # hand
    preds = torch.load(task_dir / "data" / "synthtask.pt")
    labels = torch.load(task_dir / "data" / "synthtask_labels.pt")
    ds = Dataset.from_tensors(preds, labels, "cpu")
    oracle = Oracle(ds, LOSS_FNS["acc"])
    import main as harness
    harness.seed_all(0)
    losses = oracle.true_losses(ds.preds)
    sel = CODA(ds, chunk_size=64)
    sel.get_best_model_prediction()
    want = []
    for n in (4, 4, 2):
        items = sel.get_next_items_to_label(n)
        ids = [i for i, _ in items]
        sel.add_labels(ids, [oracle(i) for i in ids], [p for _, p in items])
        want.append(float(losses[sel.get_best_model_prediction()]
                          - losses.min()))
    assert [v[3], v[7], v[9]] == want


def test_batch_size_one_is_the_default_run(task_dir):
    common = ["--method", "coda", "--iters", "6", "--seeds", "1"]
    _run_cli(task_dir, common + ["--experiment-name", "plain"])
    _run_cli(task_dir, common + ["--experiment-name", "one",
                                 "--batch-size", "1"])
    for key in ("regret", "cumulative regret"):
        a = _metric(task_dir, "plain", key)
        assert len(a) == 6 and a == _metric(task_dir, "one", key)
    assert len(_metric(task_dir, "one", "step_seconds")) == 6
    assert "batch_size" not in _params(task_dir, "plain")
    assert "batch_size" not in _params(task_dir, "one")


def test_baseline_runs_in_rounds(task_dir):
    _run_cli(task_dir, ["--method", "iid", "--iters", "10", "--seeds", "1",
                        "--batch-size", "4", "--experiment-name", "iid4"])
    v = [x for _, x in _metric(task_dir, "iid4", "regret")]
    assert len(v) == 10
    assert v[0] == v[1] == v[2] and v[4] == v[5] == v[6] == v[3]
    assert v[8] == v[7]


def test_checkpoint_every_must_be_whole_rounds(task_dir, capsys):
    with pytest.raises(SystemExit):
        _run_cli(task_dir, ["--method", "coda", "--iters", "8",
                            "--batch-size", "4", "--checkpoint-every", "6"])
    assert "multiple" in capsys.readouterr().err
    _run_cli(task_dir, ["--method", "coda", "--iters", "8", "--seeds", "1",
                        "--no-mlflow", "--batch-size", "4",
                        "--checkpoint-every", "4",
                        "--checkpoint-dir", str(task_dir / "ck")])


# ---------------------------------------------------------------------
# 6. serving
# ---------------------------------------------------------------------

def test_serve_next_batch():
    pytest.importorskip("fastapi")
    from fastapi.testclient import TestClient
    from coda_amd.serve import create_app
    preds, labels = make_synthetic_task(H=5, N=150, C=4, seed=3)
    ds = Dataset.from_tensors(preds, labels, "cpu")
    oracle = Oracle(ds, LOSS_FNS["acc"])
    c = TestClient(create_app(ds, method="coda", oracle=oracle,
                              chunk_size=64))
    items = c.get("/next_batch", params={"k": 3}).json()["items"]
    assert len(items) == 3
    ids = [it["index"] for it in items]
    assert len(set(ids)) == 3 and all(0 <= i < 150 for i in ids)
    assert all(isinstance(it["prob"], float) for it in items)
    for n, i in enumerate(ids):
        st = c.post("/answer", json={"index": i, "label": oracle(i)}).json()
        assert st["step"] == n + 1
    nxt = c.get("/next_batch", params={"k": 3}).json()["items"]
    assert len(nxt) == 3 and not {it["index"] for it in nxt} & set(ids)
    # a skipped item leaves the pool as after /next
    c.post("/skip", json={"index": nxt[0]["index"]})
    again = c.get("/next_batch", params={"k": 3}).json()["items"]
    assert nxt[0]["index"] not in {it["index"] for it in again}
    assert c.get("/next_batch", params={"k": 0}).status_code == 400
    assert "index" in c.get("/next").json()      # /next is unchanged
