"""-m gpu: numeric embedding columns in the one-launch step (csrc/train_fused.hip through mi_train_step_model_numeric,
mi_train_group_step_numeric and mi_eval_group_numeric): engine.DeepFM.fused_train_step with x_num and FusedPopulation against
the oracle, the layered step and fp64, over the case table tests/fused_numeric_cases.py (bars and shapes: its docstring),
which test_fused_numeric_cpu.py runs on the numpy stand-in."""
import numpy as np
import pytest
import torch

from mi355x_rec import _lib
from mi355x_rec.population import FusedPopulation
from tests import fused_numeric_cases as NC
from tests.util import dev, guarded_nan, guards_intact, max_err_scaled

pytestmark = pytest.mark.gpu

STATE = ("t_rec", "lin_state", "dense", "d_s0", "d_s1", "dl_s0", "dl_s1", "last_step")


def _snapshot(m):
    return {n: getattr(m, n).clone() for n in STATE if getattr(m, n, None) is not None}


def _same(a, b):
    return sorted(a) == sorted(b) and all(torch.equal(a[n], b[n]) for n in a)


def _batch(rng, vocab, B, nd, zero_x=False, plain_x=False):
    x = np.zeros((B, nd), np.float32) if zero_x else NC.draw_x(rng, B, nd)
    if plain_x:
        x = rng.standard_normal((B, nd)).astype(np.float32)
    return dev(NC.draw_ids(rng, vocab, B)), dev(x), dev((rng.random(B) < 0.3).astype(np.uint8))


def _engine(shape="three_and_two", E=4, seed=40, **kw):
    vocab, nd, hidden, flags = NC.SHAPES[shape]
    m = NC.make_engine(vocab, E, hidden, nd, flags, "cuda", **kw)
    m.load_oracle_params(NC.make_params(seed, vocab, E, hidden, nd, flags[2]))
    return m


def _raw_step(m, ids, x, y, logits, loss, sweep_blocks=0, nd=None):
    """mi_train_step_model_numeric through the binding, as engine.fused_train_step calls it, with overrides"""
    B = ids.shape[0]
    ws = torch.empty(max(m.fused_workspace_bytes(B), 16), dtype=torch.uint8, device="cuda")
    step = m.step + 1
    model, held = m.fused_model(B, ws, m.sched.lr_t(step) if m.sched else 0.0, m.lin_sched.lr_t(step) if m.lin_sched else 0.0)
    num = m.fused_numeric()
    if nd is not None:
        num.n_numeric = nd
    m.k.mi_train_step_model_numeric(model, num, m.field_off, ids, x, y, B, m.F, m._layer_seed(0), step, logits, loss, sweep_blocks)


# ---- 1. the trajectory against the oracle ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", NC.CASES, ids=NC.CASE_IDS)
def test_trajectory_matches_oracle(case):
    NC.run_trajectory(case, "cuda")


# ---- 2. against the layered step on equal state ---------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,E,B", [("three_and_two", 4, 33), ("budget_26_13", 4, 32), ("budget_exact", 4, 128)])
def test_against_the_layered_step_on_equal_state(shape, E, B):
    """x_num of order 1 here (no column scaled by 100): the bar on the slots is ABSOLUTE, 2e-6, and a column of values near
    100 gives num_emb's m and v magnitudes of 1e2 and more, where one fp32 ulp (7.6e-6 at 100) is already above it."""
    vocab, nd, hidden, flags = NC.SHAPES[shape]
    a = _engine(shape, E, gemm="fp32")                         # (exact fp32 products, as the fused step's; catchup="exact")
    rng = np.random.default_rng(41)
    for _ in range(3):                                         # slots of many rows and of the dense variables are non-zero afterwards
        ids, x, y = _batch(rng, vocab, B, nd, plain_x=True)
        a.train_step(ids, y, x)
    b = _engine(shape, E)
    b.load_state_dict(a.state_dict())                          # (state_dict brings every row up to date: both start current)
    assert torch.equal(a.t_rec, b.t_rec) and torch.equal(a.lin_state, b.lin_state) and torch.equal(a.dense, b.dense)
    ids, x, y = _batch(rng, vocab, B, nd, plain_x=True)
    la, za = a.train_step(ids, y, x)
    a.finalize_rows()
    lb, zb = b.fused_train_step(ids, y, x)
    touched = torch.zeros(a.R, dtype=torch.bool, device="cuda")
    touched[(ids.long() + a.field_off[None, :]).reshape(-1)] = True
    u = ~touched
    if int(u.sum()):
        assert torch.equal(a.t_rec[u], b.t_rec[u]) and torch.equal(a.lin_state[u], b.lin_state[u])     # bit for bit
    assert torch.equal(a.last_step, b.last_step)
    figures = {"t_rec": float((a.t_rec[touched] - b.t_rec[touched]).abs().max()),
               "lin_state": float((a.lin_state[touched][:, :3] - b.lin_state[touched][:, :3]).abs().max())}
    for n in ("dense", "d_s0", "d_s1"):
        figures[n] = float((getattr(a, n) - getattr(b, n)).abs().max())
    sl = slice(a.num_emb_off, a.num_emb_off + nd * E)
    figures["num_emb m"] = float((a.d_s0[sl] - b.d_s0[sl]).abs().max())
    le, ze = abs(la.item() - lb.item()) / abs(la.item()), max_err_scaled(zb.cpu().numpy(), za.cpu().numpy())
    print("FNUM layered %s-E%d-B%d: loss %.2e logits %.2e %s (bar 2e-06)" % (shape, E, B, le, ze, figures))
    assert all(v < 2e-6 for v in figures.values()), figures
    assert le < 2e-5 and ze < 5e-5
    assert bool((b.d_s0[sl] != 0).any())                       # the numeric embeddings did get a gradient


# ---- 3. the gradients' window -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", NC.GRAD_CASES, ids=NC.GRAD_IDS)
def test_numeric_gradients_against_fp64(case):
    NC.check_gradient_window(case, "cuda")


# ---- 4. exactness ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,E,B", [("three_and_two", 4, 33), ("budget_26_13", 4, 32)])
def test_same_bits_twice_and_for_every_sweep_grid(shape, E, B):
    vocab, nd, hidden, flags = NC.SHAPES[shape]
    a = _engine(shape, E, dropout=0.1, seed=2)
    rng = np.random.default_rng(51)
    for _ in range(3):
        ids, x, y = _batch(rng, vocab, B, nd)
        a.fused_train_step(ids, y, x)
    sd = a.state_dict()
    ids, x, y = _batch(rng, vocab, B, nd)
    results = []
    for blocks in (0, 0, 1, 7, 64):
        m = _engine(shape, E, dropout=0.1, seed=2)
        m.load_state_dict(sd)
        gl, logits = guarded_nan(B)
        gs, loss = guarded_nan(1)
        _raw_step(m, ids, x, y, logits, loss, sweep_blocks=blocks)
        torch.cuda.synchronize()
        assert guards_intact(gl) and guards_intact(gs)
        assert bool(torch.isfinite(logits).all()) and bool(torch.isfinite(loss).all()) and bool((m.last_step == 4).all())
        results.append((_snapshot(m), logits.clone(), loss.clone()))
    for s, z, l in results[1:]:
        assert _same(results[0][0], s) and torch.equal(results[0][1], z) and torch.equal(results[0][2], l)
    m = _engine(shape, E, dropout=0.1, seed=2)                 # and the engine's own call is that step
    m.load_state_dict(sd)
    loss, logits = m.fused_train_step(ids, y, x)
    assert _same(results[0][0], _snapshot(m)) and torch.equal(logits, results[0][1]) and torch.equal(loss, results[0][2])


def _members(M, shape="three_and_two", **kw):
    out = []
    for i in range(M):
        m = _engine(shape, 4 if i % 2 == 0 else 8, seed=60 + i, dropout=0.1 * (i % 2), **kw)
        out.append(m)
    return out


@pytest.mark.parametrize("per_member", [False, True], ids=["shared x_num", "x_num per member"])
def test_a_population_member_equals_its_solo_step(per_member):
    M, B = 4, 33
    vocab, nd, _, _ = NC.SHAPES["three_and_two"]
    pop_e, solo_e = _members(M), _members(M)
    pop = FusedPopulation(pop_e)
    rng = np.random.default_rng(5)
    for s in range(3):
        batches = [_batch(rng, vocab, B, nd) for _ in range(M if per_member else 1)]
        if per_member:
            ids, x = torch.stack([b[0] for b in batches]), torch.stack([b[1] for b in batches])
        else:
            ids, x = batches[0][:2]
        y = batches[0][2]
        loss, logits = pop.train_step(ids, y, x_num=x)
        for i, e in enumerate(solo_e):
            l1, z1 = e.fused_train_step(ids[i] if per_member else ids, y, x[i] if per_member else x)
            assert torch.equal(z1, logits[i]) and torch.equal(l1[0], loss[i]), (s, i)
            assert _same(_snapshot(e), _snapshot(pop_e[i])), (s, i)


def test_evaluation_logits_are_the_steps_logits():
    M, B, N = 3, 32, 32 * 3 + 5
    vocab, nd, _, _ = NC.SHAPES["three_and_two"]
    es = [_engine(E=4 if i else 8, seed=70 + i) for i in range(M)]          # (no dropout: keep_prob = 1)
    pop = FusedPopulation(es)
    rng = np.random.default_rng(6)
    ids, x, y = _batch(rng, vocab, N, nd)
    before = [_snapshot(e) for e in es]
    metrics, z = pop.evaluate(ids, y, batch_size=B, return_logits=True, x_num=x)
    torch.cuda.synchronize()
    assert all(_same(b, _snapshot(e)) for b, e in zip(before, es))          # nothing of any member is written
    assert all(np.isfinite(m["loss"]) for m in metrics)
    # a full tile and the short last tile, each as a training batch on the same state
    for lo, hi in ((B, 2 * B), (3 * B, N)):
        clones = [_engine(E=4 if i else 8, seed=70 + i) for i in range(M)]
        _, logits = FusedPopulation(clones).train_step(ids[lo:hi].contiguous(), y[lo:hi].contiguous(), x_num=x[lo:hi].contiguous())
        assert torch.equal(logits, z[:, lo:hi]), (lo, hi)


def test_without_numeric_columns_the_new_entries_give_the_existing_entries_bits():
    vocab, hidden, B = [9, 13, 5], [16, 16], 33
    rng = np.random.default_rng(8)
    ids, _, y = _batch(rng, vocab, B, 1)

    def fresh():
        m = NC.make_engine(vocab, 4, hidden, 0, (True, True, True), "cuda", hp=("Adagrad", 0.05))
        m.load_oracle_params(NC.make_params(80, vocab, 4, hidden, 0))
        return m
    a, b = fresh(), fresh()
    la, za = a.fused_train_step(ids, y)                                       # mi_train_step_model
    zb, lb = torch.empty(B, device="cuda"), torch.empty(1, device="cuda")
    ws = torch.empty(max(b.fused_workspace_bytes(B), 16), dtype=torch.uint8, device="cuda")
    model, held = b.fused_model(B, ws, 0.0, 0.0)
    b.k.mi_train_step_model_numeric(model, None, b.field_off, ids, None, y, B, b.F, b._layer_seed(0), 1, zb, lb, 0)
    assert torch.equal(za, zb) and torch.equal(la, lb)
    b.step = b._final_step = 1
    assert _same(_snapshot(a), _snapshot(b))
    # the group: a plan of mi_train_group_plan_models_numeric with no numeric description, stepped and evaluated by the
    # numeric entries, against FusedPopulation's own calls
    c, d = fresh(), fresh()
    lc, zc = FusedPopulation([c]).train_step(ids, y)
    pop = FusedPopulation([d])
    keep = []
    members = (_lib.FusedModel * 1)(pop._describe(d, B, keep))
    table = torch.empty(int(d.k.query("mi_train_group_plan_bytes", 1)), dtype=torch.uint8, device="cuda")
    plan = _lib.FusedGroupPlan()
    d.k.mi_train_group_plan_models_numeric(members, None, 1, B, d.F, d.field_off, table, table.numel(), plan)
    zd, ld = torch.empty(1, B, device="cuda"), torch.empty(1, device="cuda")
    d.k.mi_train_group_step_numeric(plan, 1, ids, 0, None, 0, y, 0, B, 1, zd, ld, 0)
    d.step = d._final_step = 1
    assert torch.equal(zc, zd) and torch.equal(lc, ld) and _same(_snapshot(c), _snapshot(d))
    assert torch.equal(FusedPopulation([c]).evaluate(ids, y, batch_size=B, return_logits=True)[1],
                       FusedPopulation([d]).evaluate(ids, y, batch_size=B, return_logits=True)[1])


def test_with_x_num_all_zero_the_numeric_variables_keep_their_bits():
    vocab, nd, _, _ = NC.SHAPES["three_and_two"]
    m = _engine()
    ids, x, y = _batch(np.random.default_rng(9), vocab, 33, nd, zero_x=True)
    before = _snapshot(m)
    m.fused_train_step(ids, y, x)
    E = m.E
    for sl in (slice(m.num_emb_off, m.num_emb_off + nd * E), slice(m.lin_num_off, m.lin_num_off + nd)):
        for n in ("dense", "d_s0", "d_s1"):
            assert torch.equal(getattr(m, n)[sl], before[n][sl]), n
    assert not torch.equal(m.dense, before["dense"])           # (the MLP did move)


# ---- 5. the other rules -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(NC.RULES))
def test_other_rules_against_the_oracle(name):
    m, _ = NC.run_rule(name, "cuda")
    if m.lin_opt is not None:                                  # lin_num moved by the WIDE rule: its slots are the wide part's
        sl = slice(m.lin_num_off, m.lin_num_off + m.n_numeric)
        assert bool((m.dl_s0[sl] != 0.1).all()) and bool((m.d_s0[sl] == 0.1).all())
        se = slice(m.num_emb_off, m.num_emb_off + m.n_numeric * m.E)
        assert bool((m.d_s0[se] != 0.1).any()) and bool((m.dl_s0[se] == 0.1).all())


# ---- 6. refusals through the entry: nothing is launched or written --------------------------------------------------------------
def test_refusals_through_the_entries_launch_nothing():
    vocab, nd, hidden, flags = NC.SHAPES["budget_exact"]       # 26 + 6 columns at E = 4
    m = _engine("budget_exact", 4)
    rng = np.random.default_rng(3)
    for B, over, null_x, status, text in ((8, 17, False, r"\(-2\)", "17 numeric columns"),
                                          (128, 7, False, r"\(-2\)", r"B \(F \+ n_numeric\) E = 16896"),
                                          (8, None, True, r"\(-1\)", "x_num")):
        ids, _, y = _batch(rng, vocab, B, nd)
        x = torch.zeros(B, 17, device="cuda")
        gl, logits = guarded_nan(B)
        gs, loss = guarded_nan(1)
        before = _snapshot(m)
        with pytest.raises(_lib.MiError, match=status + ".*" + text):
            _raw_step(m, ids, None if null_x else x, y, logits, loss, nd=over)
        torch.cuda.synchronize()
        assert _same(before, _snapshot(m)) and bool((m.last_step == 0).all())
        assert guards_intact(gl) and guards_intact(gs) and bool(torch.isnan(logits).all()) and bool(torch.isnan(loss).all())
    # a plan that holds numeric columns, handed to the entries that bring no x_num
    es = _members(2)
    pop = FusedPopulation(es)
    vocab, nd, _, _ = NC.SHAPES["three_and_two"]
    B = 16
    ids, x, y = _batch(rng, vocab, B, nd)
    pop.train_step(ids, y, x_num=x)
    plan = pop._plans[B][1]
    before = [_snapshot(e) for e in es]
    gl, logits = guarded_nan(2, B)
    gs, loss = guarded_nan(2)
    with pytest.raises(_lib.MiError, match="numeric columns and this entry brings no x_num"):
        pop.k.mi_train_group_step(plan, 2, ids, 0, y, 0, B, 2, logits, loss, 0)
    gb, batch_loss = guarded_nan(2, 1)
    hist = torch.zeros(2, 2, 201, dtype=torch.int64, device="cuda")
    counts = torch.zeros(2, 8, dtype=torch.int64, device="cuda")
    partials = torch.full((2, 1, 3), float("nan"), dtype=torch.float64, device="cuda")
    with pytest.raises(_lib.MiError, match="numeric columns and this entry brings no x_num"):
        pop.k.mi_eval_group(plan, 2, ids, y, B, None, logits, batch_loss, hist, counts, partials, 0)
    with pytest.raises(_lib.MiError, match="x_num"):
        pop.k.mi_train_group_step_numeric(plan, 2, ids, 0, None, 0, y, 0, B, 2, logits, loss, 0)
    with pytest.raises(_lib.MiError, match="x_num_member_stride"):
        pop.k.mi_train_group_step_numeric(plan, 2, ids, 0, x, 5, y, 0, B, 2, logits, loss, 0)
    torch.cuda.synchronize()
    assert all(_same(b, _snapshot(e)) for b, e in zip(before, es))
    assert guards_intact(gl) and guards_intact(gs) and guards_intact(gb)
    assert bool(torch.isnan(logits).all()) and bool(torch.isnan(loss).all()) and bool(torch.isnan(batch_loss).all())
    assert not bool(hist.any()) and not bool(counts.any()) and bool(torch.isnan(partials).all())
