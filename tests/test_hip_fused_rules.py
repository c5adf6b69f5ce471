"""GPU: the one-launch train step under every optimizer, with two rules and with the canned estimators' columns
(mi_train_step_model, mi_train_group_plan_models; csrc/train_fused.hip) — trajectories against the oracle, untouched rows,
zeros that stay zero, gradients against fp64, bits, and refusals that launch nothing.  Cases, bars and the printed figures:
tests/fused_rules_cases.py.  The same trajectories run on the numpy stand-in in test_fused_rules_cpu.py."""
import math

import numpy as np
import pytest
import torch

from mi355x_rec import _lib
from tests import fused_rules_cases as FC
from tests.cases import ML100K_VOCAB
from tests.util import dev

pytestmark = pytest.mark.gpu

STATE = ("t_rec", "lin_state", "dense", "d_s0", "d_s1", "dl_s0", "dl_s1", "last_step")
WIDE_DEEP = FC.CASES["wide_deep_two_optimizers"]
# one part under Adam, the other not (a DeepFM handed a linear_optimizer)
ADAM_TABLE = dict(flags=(True, True, True), hp=("Adam", 0.001), lin_hp=("Ftrl", 0.1))
ADAM_WIDE = dict(flags=(True, True, True), hp=("Adagrad", 0.05), lin_hp=("Adam", 0.02))


def _state(m):
    return {n: getattr(m, n).clone() for n in STATE if getattr(m, n, None) is not None}


def _same(a, b):
    """the first state tensor in which engines (or snapshots) a and b differ, or None"""
    a, b = (x if isinstance(x, dict) else _state(x) for x in (a, b))
    assert sorted(a) == sorted(b)
    return next((n for n in a if not torch.equal(a[n], b[n])), None)


def _started(case, vocab=FC.VOCAB, emb=FC.E, gen_seed=7):
    """an engine of the case with drawn variables"""
    m = FC.make_engine(case, "cuda", vocab=vocab, emb=emb)
    m.load_oracle_params(FC.make_params(case, vocab, emb, seed=gen_seed))
    return m


def _touched(m, ids):
    t = torch.zeros(m.R, dtype=torch.bool, device="cuda")
    t[(torch.from_numpy(ids).long() + torch.from_numpy(m.field_off_host[:-1])[None, :]).reshape(-1).cuda()] = True
    return t


# ---- trajectories ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", FC.TRAJECTORY_NAMES)
def test_trajectory_against_the_oracle(name):
    m, _ = FC.run_trajectory(name, name, "cuda")
    assert "mi_train_step_model" in m.k.__dict__ and "mi_train_step_fused" not in m.k.__dict__       # (the entry that ran)


def test_trajectory_at_the_cli_default_shape():
    """trainers.linear_deep's defaults: the MovieLens columns, E 4, [16, 16], B 32, Ftrl(min(0.2, 1 / sqrt(26))) + Adagrad(0.05)"""
    case = dict(WIDE_DEEP, hidden=[16, 16], lin_hp=("Ftrl", min(0.2, 1.0 / math.sqrt(len(ML100K_VOCAB)))))
    FC.run_trajectory("cli default wide & deep", case, "cuda", vocab=ML100K_VOCAB, emb=4, batch=32)


@pytest.mark.parametrize("name,case,emb,batch", [
    ("B = 1", WIDE_DEEP, 8, 1), ("B = 128", WIDE_DEEP, 8, 128),
    ("E = 12 Adagrad: stride 24, three chunks", FC.CASES["dnn_classifier_adagrad_sum_dropout"], 12, 64),
    ("SGD: stride E, no slot", dict(FC.CASES["deepfm_sgd"], dropout=0.1), 4, 33),
])
def test_trajectory_at_the_edges(name, case, emb, batch):
    m, _ = FC.run_trajectory(name, case, "cuda", emb=emb, batch=batch)
    nsl = sum(s is not None for s in m.opt.slot_init)
    assert m.ts == (1 + nsl) * emb and (m.t_s1 is None) == (nsl < 2) and (m.t_s0 is None) == (nsl < 1)


# ---- untouched rows ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["wide_deep_two_optimizers", "deepfm_ftrl", "deepfm_rmsprop", "deepfm_sgd", "linear_classifier_ftrl_sum"])
def test_without_an_adam_part_untouched_rows_keep_their_bits(name):
    m = _started(name)
    assert m.last_step is None
    rng = np.random.default_rng(5)
    for s in range(2):                                        # (the second step: from slots that have moved)
        ids, y = FC.draw_batch(rng, FC.VOCAB, 16)
        before = _state(m)
        m.fused_train_step(dev(ids), dev(y))
        u = ~_touched(m, ids)
        assert 0 < int(u.sum()) < m.R
        for n in ("t_rec", "lin_state"):                      # whole records: weights, slots and the unused fourth word
            if n in before:
                assert torch.equal(before[n][u].view(torch.int32), getattr(m, n)[u].view(torch.int32)), (n, s)
                assert not torch.equal(before[n][~u], getattr(m, n)[~u]), (n, s)


@pytest.mark.parametrize("case,adam_part", [(ADAM_TABLE, "t_rec"), (ADAM_WIDE, "lin_state")], ids=["adam table", "adam wide"])
def test_with_adam_on_one_part_its_untouched_rows_get_the_layered_sweep_and_the_others_keep_their_bits(case, adam_part):
    """as test_hip_fused_step's test for Adam on everything: engine a takes layered steps (exact catch-up, fp32 GEMMs), b is
    a copy that takes the last one as a fused step"""
    B = 32
    from mi355x_rec.engine import DeepFM, OptimizerSpec
    mk = lambda: DeepFM(FC.VOCAB, embedding_size=FC.E, hidden_units=FC.HIDDEN, optimizer=OptimizerSpec(*case["hp"]),
                        linear_optimizer=OptimizerSpec(*case["lin_hp"]), catchup="exact", gemm="fp32", seed=3)
    a, b = mk(), mk()
    a.load_oracle_params(FC.make_params(case, seed=41))
    rng = np.random.default_rng(41)
    for _ in range(4):
        ids, y = FC.draw_batch(rng, FC.VOCAB, B)
        a.train_step(dev(ids), dev(y))
    b.load_state_dict(a.state_dict())
    assert _same(a, b) is None
    ids, y = FC.draw_batch(rng, FC.VOCAB, B)
    start = _state(b)
    a.train_step(dev(ids), dev(y))
    a.finalize_rows()
    b.fused_train_step(dev(ids), dev(y))
    u = ~_touched(a, ids)
    assert 0 < int(u.sum()) < a.R
    if adam_part == "t_rec":
        assert torch.equal(a.t_rec[u], b.t_rec[u])                                       # w, m, v: the exact one-step catch-up
        assert int((b.t_rec[u] != start["t_rec"][u]).any(1).sum()) > 0                   # (the sweep did move something)
        assert torch.equal(b.lin_state[u][:, :3].view(torch.int32), start["lin_state"][u][:, :3].view(torch.int32))
    else:
        assert torch.equal(a.lin_state[u][:, :3], b.lin_state[u][:, :3])
        assert int((b.lin_state[u][:, :3] != start["lin_state"][u][:, :3]).any(1).sum()) > 0
        assert torch.equal(b.t_rec[u].view(torch.int32), start["t_rec"][u].view(torch.int32))
    assert bool((b.last_step == 5).all()) and torch.equal(a.last_step, b.last_step)      # stamps: the step, on every row


# ---- zeros stay zero ---------------------------------------------------------------------------------------------------------
def test_padded_columns_their_kernel_rows_and_unused_wide_records_keep_their_bits():
    name = "wide_and_deep_parts_on_different_columns_with_per_column_dimensions"
    m, _ = FC.run_trajectory(name, name, "cuda")
    start = FC.make_engine(name, "cuda")                       # (slots at their initial values)
    bits = lambda t: t.contiguous().view(torch.int32)
    off, E = m.field_off_host, m.E
    k0, k0_s = m.kernel(0), m.kernel(0, m.d_s0)
    for f, d in enumerate(FC.DIMS):
        r = slice(int(off[f]), int(off[f + 1]))
        assert not bool(bits(m.table[r, d:]).any()), f                                      # the padding: +0.0
        assert torch.equal(bits(m.t_s0[r, d:]), bits(start.t_s0[r, d:])), f                # its accumulator: no increment
        assert not bool(bits(k0[f * E + d:(f + 1) * E]).any()), f                          # the matching rows of kernel_0
        assert torch.equal(bits(k0_s[f * E + d:(f + 1) * E]), bits(start.kernel(0, start.d_s0)[f * E + d:(f + 1) * E])), f
        if d:
            assert bool((m.t_s0[r, :d] != start.t_s0[r, :d]).any()), f                      # (the columns in use did move)
    r = slice(int(off[1]), int(off[2]))                                                      # field 1 has no wide weight
    assert torch.equal(bits(m.lin_state[r]), bits(start.lin_state[r]))
    assert bool((m.lin_state[int(off[0]):int(off[1])] != start.lin_state[int(off[0]):int(off[1])]).any())


# ---- gradients against fp64 ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", sorted(FC.GRAD_RULES))
def test_one_step_from_the_cold_state_against_fp64(kind):
    from tests.fused_rules_kernels import FusedRulesKernels
    margin = FC.grad_margin(kind)
    print("FRULES fp64 %-8s margin on the host first: %.2e" % (kind, margin))
    assert margin >= FC.RELU_MARGIN
    FC.check_gradients(kind, "cpu", FusedRulesKernels())       # (the stand-in holds the same bar: the check itself is sound)
    FC.check_gradients(kind, "cuda")


# ---- bits ---------------------------------------------------------------------------------------------------------------------
POPULATION = [dict(flags=(True, True, True), hp=("Adam", 0.001), dropout=0.1), dict(FC.CASES["deepfm_adagrad"], dropout=0.1),
              dict(WIDE_DEEP, flags=(True, False, True)), FC.CASES["deepfm_rmsprop"], FC.CASES["deepfm_sgd"]]


def _members(order):
    return [_started(POPULATION[i], gen_seed=50 + i) for i in order]


@pytest.mark.parametrize("name", ["wide_deep_two_optimizers", "two_different_adam_optimizers", "deepfm_sgd"])
def test_two_calls_from_equal_state_and_any_sweep_blocks_give_equal_bits(name):
    rng = np.random.default_rng(9)
    batches = [FC.draw_batch(rng, FC.VOCAB, 48) for _ in range(2)]
    ref = None
    for blocks in (0, 0, 1, 7):
        m = _started(name)
        m.FUSED_STEP_SWEEP_BLOCKS = blocks
        outs = []
        for ids, y in batches:
            loss, logits = m.fused_train_step(dev(ids), dev(y))
            outs += [loss.clone(), logits.clone()]
        got = (_state(m), outs)
        if ref is None:
            ref = got
        assert _same(ref[0], got[0]) is None, (name, blocks)
        assert all(torch.equal(x, z) for x, z in zip(ref[1], got[1])), (name, blocks)


@pytest.mark.parametrize("order", [[0, 1, 2, 3, 4], [4, 2, 0, 3, 1]], ids=["in order", "shuffled"])
def test_a_mixed_population_steps_and_evaluates_each_member_as_its_solo_run(order):
    from mi355x_rec.population import FusedPopulation
    solo, group = _members(order), _members(order)
    pop = FusedPopulation(group)
    rng = np.random.default_rng(13)
    B = 32
    for s in range(3):
        ids, y = FC.draw_batch(rng, FC.VOCAB, B)
        loss, logits = pop.train_step(dev(ids), dev(y))
        for i, m in enumerate(solo):
            lo, lg = m.fused_train_step(dev(ids), dev(y))
            assert torch.equal(lo[0], loss[i]) and torch.equal(lg, logits[i]), (order[i], s)
            assert _same(m, group[i]) is None, (order[i], s, _same(m, group[i]))
    assert "mi_train_group_plan_models" in pop.k.__dict__
    # evaluate: every member's logits are its own forward's (no dropout), bit for bit; nothing of any member moves
    before = [_state(m) for m in group]
    ids, y = FC.draw_batch(rng, FC.VOCAB, 2 * B + 5)
    _, z = pop.evaluate(dev(ids), dev(y), batch_size=B, return_logits=True)
    for i, m in enumerate(solo):
        assert _same(before[i], group[i]) is None
        keep, m.dropout = m.dropout, 0.0
        st = _state(m)
        for lo_ in range(0, len(y), B):                         # a solo step without dropout reports the tile's logits
            _, lg = m.fused_train_step(dev(ids[lo_:lo_ + B]), dev(y[lo_:lo_ + B]))
            assert torch.equal(lg, z[i, lo_:lo_ + B]), (order[i], lo_)
            for n, t in st.items():                             # (back to the evaluated state)
                getattr(m, n).copy_(t)
            m.step = m._final_step = 3
        m.dropout = keep


# ---- refusals on the device --------------------------------------------------------------------------------------------------
def test_refusals_through_the_entries_launch_nothing():
    from mi355x_rec.engine import OptimizerSpec
    from mi355x_rec.population import FusedPopulation
    B = 16
    m = _started(ADAM_TABLE)
    rng = np.random.default_rng(3)
    ids, y = (dev(a) for a in FC.draw_batch(rng, FC.VOCAB, B))
    logits, loss = torch.full((B,), float("nan"), device="cuda"), torch.full((1,), float("nan"), device="cuda")
    ws = torch.empty(int(m.k.query("mi_train_step_fused_workspace_bytes", B, m.F, m.E, m.P)), dtype=torch.uint8, device="cuda")
    before = _state(m)

    def corrupt(**at):
        model, held = m.fused_model(B, ws, 0.001, 0.0)
        for k, v in at.items():
            setattr(model, k, v)
        return model, held
    cases = [
        (dict(l_v=None), "lin_w / l_m / l_v"), (dict(t_m=None), "table / t_m / t_v"), (dict(dw_m=None), "dw_m / dw_v"),
        (dict(d_v=None), "dense / d_m / d_v"), (dict(last_step=None), "last_step"),
        (dict(use_linear=0), "two_rules without the wide part"), (dict(wide_fields=1 << m.F), "wide_fields names a field at or above F=4"),
        (dict(hp_wide=OptimizerSpec("Ftrl", 0.1, lr_power=-0.4).hparams()), "learning_rate_power"),
        (dict(hp=OptimizerSpec("Adam").hparams().__class__(7, *[0.0] * 10)), "optimizer kind 7"),
    ]
    for at, text in cases:
        model, held = corrupt(**at)
        with pytest.raises(_lib.MiError, match=text):
            m.k.mi_train_step_model(model, m.field_off, ids, y, B, m.F, 1, 1, logits, loss, 0)
        table = torch.full((int(m.k.query("mi_train_group_plan_bytes", 1)),), 0xA5, dtype=torch.uint8, device="cuda")
        plan = _lib.FusedGroupPlan()
        model.lr_table, model.lr_table_len = m.sched.table.data_ptr(), m.sched.table.numel()
        with pytest.raises(_lib.MiError, match="member 0: .*" + text):
            m.k.mi_train_group_plan_models((_lib.FusedModel * 1)(model), 1, B, m.F, m.field_off, table, table.numel(), plan)
        assert plan.magic == 0 and bool((table == 0xA5).all())
    # a schedule table is required exactly for a rule under Adam
    model, held = corrupt()
    plan = _lib.FusedGroupPlan()
    table = torch.full((int(m.k.query("mi_train_group_plan_bytes", 1)),), 0xA5, dtype=torch.uint8, device="cuda")
    with pytest.raises(_lib.MiError, match="member 0: .*lr_table of 0 entries"):
        m.k.mi_train_group_plan_models((_lib.FusedModel * 1)(model), 1, B, m.F, m.field_off, table, table.numel(), plan)
    # the host side: numeric columns stay outside, on the device as on the stand-ins
    from mi355x_rec.engine import DeepFM
    n = DeepFM(FC.VOCAB, n_numeric=2, embedding_size=8, hidden_units=[8], optimizer=OptimizerSpec("Adagrad", 0.05))
    assert not n.fused_step_ok(B) and "numeric columns" in n._fused_step_limit(B)
    with pytest.raises(ValueError, match="numeric columns"):
        FusedPopulation([n])
    torch.cuda.synchronize()
    assert _same(before, m) is None
    assert bool(torch.isnan(logits).all()) and bool(torch.isnan(loss).all()) and bool((table == 0xA5).all())
