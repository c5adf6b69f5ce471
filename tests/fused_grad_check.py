"""The one-launch train step's gradients and Adam slots against fp64 (shared by test_hip_fused_gradients.py, on the
device, and test_fused_gradients_cpu.py, on the numpy stand-in).  Not a test file.

mi_train_step_fused keeps its activations and gradients in LDS and exposes none of them; the slots it writes are the
witness.  After ONE step from a known state m is linear in the gradient and v quadratic, while the weights — the only
thing the trajectory tests look at — move by lr * m / (sqrt(v) + eps), where the gradient's magnitude cancels.

check_step:
  1. reads the engine's whole state back (variables, every slot, stamps, step) and builds the oracle's Params and
     TrainState from it, once widened to fp64 and once in fp32, beta powers at the engine's step;
  2. runs one oracle.deepfm.train_step in each precision, with the host replica of the step's dropout masks and the
     kernel's constants (beta1, beta2, epsilon, lr, keep_prob: the fp32 values, widened), so that the measure sees
     arithmetic and not constants; a relu model's fp64 hidden pre-activations must lie at least 1e-6 from 0 (the fused
     step leaves no activation in memory to read its decisions from: cases are chosen with a margin);
  3. runs one fused_train_step;
  4. compares EVERY element of every variable's m and v with the fp64 run: tests.util.max_err_scaled per variable, bar
     max(1e-5, 4 x E32), E32 the same measure for the fp32 oracle run against the fp64 one (computed here, never taken
     from the engine; the factor 4 is the headroom test_hip_gradients.py gives over a plain fp32 evaluation).  From a
     cold state the rows the batch does not touch keep m == 0, v == 0 and their weight's bits; from a warm state they
     are part of the table-wide measure, the reference doing TF's whole-table sweep.  Every stamp equals the new step;
     loss, logits and variables stay at test_hip_fused_step.py's bars against that file's reference, the fp32 oracle
     run (the weights cannot be held to the fp64 run at 2e-6: where |g| is near eps / 0.03 = 3e-7 the first Adam
     update lr g / (|g| + 3e-7) turns a rounding of g into up to 1e-5 of weight, in the fp32 oracle as anywhere).

Every figure is printed (pytest -s): FGRAD <case> <variable> <slot> device ... fp32-oracle ... bar ..."""
from collections import namedtuple

import numpy as np

from oracle import deepfm as O
from oracle import optimizers as OO
from tests.cases import FLAGS, ML100K_VOCAB, TRAJECTORIES
from tests.util import _fresh_ids as fresh_ids
from tests.util import dev, dropout_mask, make_problem, max_err_scaled

RELU_MARGIN = 1e-6
WARM_STEPS = 4

State = namedtuple("State", "params emb_slots lin_slots dense_slots step")
Report = namedtuple("Report", "case figures failures margin loss_err logits_err")


def bar(e32):
    return max(1e-5, 4.0 * e32)


def _np(t):
    return t.detach().cpu().numpy().copy()


def read_state(m):
    """The engine's variables and slots as the oracle lays them out (fp32 numpy copies).  A model without a table or
    without a wide part gets zero arrays there, which the oracle then neither reads nor writes."""
    g = m.export_numpy()
    off, F = m.field_off_host, m.F
    assert m._final_step == m.step and bool((m.last_step == m.step).all()), "every row must be current"

    def per_field(t, shape):
        if t is None:
            return [np.zeros((int(off[f + 1] - off[f]),) + shape, np.float32) for f in range(F)]
        return [_np(t[int(off[f]):int(off[f + 1])]) for f in range(F)]
    emb = g["emb"] if g["emb"] is not None else per_field(None, (m.E,))
    lin_w = g["lin_w"] if g["lin_w"] is not None else per_field(None, ())
    p = O.Params([a.copy() for a in emb], [a.copy() for a in lin_w], g["lin_bias"].copy(),
                 [(k.copy(), b.copy()) for k, b in g["mlp"]])
    emb_slots = list(zip(per_field(m.t_s0, (m.E,)), per_field(m.t_s1, (m.E,))))
    lin_slots = list(zip(per_field(m.l_s0, ()), per_field(m.l_s1, ())))
    dense_slots = []
    lb = slice(m.lin_bias_off, m.lin_bias_off + 1)
    for i in range(len(m.layers)):                           # Params.dense_list() order: kernels and biases, the wide bias
        dense_slots += [(_np(m.kernel(i, m.d_s0)), _np(m.kernel(i, m.d_s1))), (_np(m.bias(i, m.d_s0)), _np(m.bias(i, m.d_s1)))]
    dense_slots.append((_np(m.d_s0[lb]), _np(m.d_s1[lb])))
    assert len(dense_slots) == len(p.dense_list())
    return State(p, emb_slots, lin_slots, dense_slots, int(m.step))


def _oracle_state(s, dt, hp):
    p = s.params.astype(dt)
    st = O.TrainState(p, hp)
    c = lambda pair: (pair[0].astype(dt), pair[1].astype(dt))
    st.emb, st.lin, st.dense = [c(x) for x in s.emb_slots], [c(x) for x in s.lin_slots], [c(x) for x in s.dense_slots]
    st.step = s.step
    for _ in range(s.step):                                  # beta powers as step s.step + 1 sees them
        st.powers.finish()
    return p, st


def _variables(m, p, emb_slots, lin_slots, dense_slots):
    """name -> (w, m, v): each layer's kernel and bias, the wide bias, the table (all rows), the wide weights (all rows)"""
    out = []
    names = [n % i for i in range(len(p.mlp)) for n in ("kernel_%d", "bias_%d")] + ["lin_bias"]
    for name, w, (s0, s1) in zip(names, p.dense_list(), dense_slots):
        out.append((name, w, s0, s1))
    cat = lambda parts: np.concatenate(parts, 0)
    if m.table is not None:
        out.append(("table", cat(p.emb), cat([a for a, _ in emb_slots]), cat([b for _, b in emb_slots])))
    if m.lin_w is not None:
        out.append(("lin_w", cat(p.lin_w), cat([a for a, _ in lin_slots]), cat([b for _, b in lin_slots])))
    return out


def check_step(case, m, ids, y, use_linear=True, use_mf=True, use_dnn=True, activation="relu", dropout=0.0,
               reduction="mean", hold=True):
    """One fused_train_step of engine m (any device) on the batch (ids, y) from the state it is in, against the oracle
    from that state.  The model's options are stated by the caller, not read from the engine.  Returns a Report; with
    hold, a non-empty Report.failures is an AssertionError."""
    B = ids.shape[0]
    hidden = list(m.hidden)
    f32w = lambda v: float(np.float32(v))
    hp = OO.Hyper("Adam", f32w(m.opt.lr), beta1=f32w(m.opt.beta1), beta2=f32w(m.opt.beta2), epsilon=f32w(m.opt.epsilon))
    keep = f32w(1.0 - dropout) if dropout else 1.0
    start = read_state(m)
    cold = start.step == 0
    if cold:
        assert all(not a.any() and not b.any() for a, b in start.emb_slots + start.lin_slots + start.dense_slots)
    masks = [dropout_mask(m._layer_seed(i), B, h, keep) for i, h in enumerate(hidden)] if dropout else None
    kw = dict(use_linear=use_linear, use_mf=use_mf, use_dnn=use_dnn, dropout_masks=masks, keep_prob=keep, activation=activation)
    runs = {}
    for dt in (np.float64, np.float32):
        p, st = _oracle_state(start, dt, hp)
        if dt is np.float64:
            pre = O.forward(p, ids, None, **kw).get("pre", [])
            margin = min([float(np.abs(q).min()) for q in pre] or [np.inf])
        loss, logits = O.train_step(p, st, ids, y, reduction=reduction, **kw)
        assert st.step == start.step + 1
        runs[dt] = (p, st, float(loss), logits)
    if activation == "relu" and use_dnn and hidden:
        assert margin >= RELU_MARGIN, (case, margin)
    p64, st64, _, _ = runs[np.float64]
    p32, st32, loss32, logits32 = runs[np.float32]

    loss_g, logits_g = m.fused_train_step(dev(ids, m.device), dev(y, m.device))
    after = read_state(m)

    failures = []
    step = start.step + 1
    if not (after.step == step and bool((m.last_step == step).all())):
        failures.append(("stamps", step, after.step))
    loss_err = abs(float(loss_g.item()) - loss32) / abs(loss32)
    logits_err = max_err_scaled(_np(logits_g), logits32)
    logits_bar = 5e-6 if cold else 5e-5
    print("FGRAD %-40s loss err %.2e (bar 2e-05)  logits err %.2e (bar %.0e)  smallest |pre-activation| %.2e" % (
        case, loss_err, logits_err, logits_bar, margin))
    if not loss_err < 2e-5:
        failures.append(("loss", loss_err))
    if not logits_err < logits_bar:
        failures.append(("logits", logits_err))
    atol = 2e-6 if activation == "relu" else 3e-6
    figures = {}
    got_vars = _variables(m, after.params, after.emb_slots, after.lin_slots, after.dense_slots)
    ref64 = _variables(m, p64, st64.emb, st64.lin, st64.dense)
    ref32 = _variables(m, p32, st32.emb, st32.lin, st32.dense)
    assert [v[0] for v in got_vars] == [v[0] for v in ref64] == [v[0] for v in ref32]
    for got, r64, r32 in zip(got_vars, ref64, ref32):
        name = got[0]
        assert got[1].shape == r64[1].shape and got[2].shape == r64[2].shape and got[3].shape == r64[3].shape, name
        werr = float(np.max(np.abs(got[1] - r32[1])))
        if not werr < atol:
            failures.append((name, "w", werr, atol))
        for slot, j in (("m", 2), ("v", 3)):
            assert np.isfinite(got[j]).all(), (name, slot)
            err, e32 = max_err_scaled(got[j], r64[j]), max_err_scaled(r32[j], r64[j])
            figures[(name, slot)] = (err, e32, bar(e32))
            print("FGRAD %-40s %-9s %s  device %.2e  fp32-oracle %.2e  bar %.2e%s" % (
                case, name, slot, err, e32, bar(e32), "  (second term)" if bar(e32) > 1e-5 else ""))
            if not err < bar(e32):
                failures.append((name, slot, err, e32, bar(e32)))
    if cold:
        # rows the batch did not touch: m == 0, v == 0, the weight's bits unchanged
        touched = np.zeros(m.R, bool)
        touched[(ids.astype(np.int64) + m.field_off_host[:-1][None, :]).reshape(-1)] = True
        u = ~touched
        before = {v[0]: v for v in _variables(m, start.params, start.emb_slots, start.lin_slots, start.dense_slots)}
        for got in got_vars:
            if got[0] not in ("table", "lin_w"):
                continue
            w0 = before[got[0]][1]
            if got[2][u].any() or got[3][u].any() or not np.array_equal(got[1][u].view(np.uint32), w0[u].view(np.uint32)):
                failures.append((got[0], "untouched rows"))
    rep = Report(case, figures, failures, margin, loss_err, logits_err)
    if hold:
        assert not failures, (case, failures)
    return rep


# ---- the cases: the smallest that reach each path of batch_block -------------------------------------------------------------
# Case.batch: "fresh" = test_hip_fused_step._fresh_ids' batches; "same" / "pair" / "triple" = hand-placed duplicates in field 0
Case = namedtuple("Case", "name vocab E hidden B seed kw batch")
SMALL, HAND = [9, 13, 5, 6], [40, 37, 41]


def _case(name, vocab, E, hidden, B, problem_seed, batch="fresh", **kw):
    return Case(name, vocab, E, hidden, B, problem_seed, kw, batch)            # (kw["seed"] is the engine's dropout seed)


# Relu cases: the smallest |hidden pre-activation| of the fp64 oracle at the checked step on the numpy stand-in's state
# (test_fused_gradients_cpu.py prints it), cold / warm, is in the comment.  At least 1e-5 each, so that the device's own
# four-step drift (variables within 2e-6) cannot bring it under the asserted 1e-6.
# TRAJECTORIES' own seeds give, in its order: 1.0e-3 / 5.0e-4, 1.7e-2 / 2.0e-2, 3.5e-5 / 6.4e-5, 4.9e-5 / 1.4e-4, 7.2e-5 / 6.8e-4,
# 2.5e-5 / 2.5e-5 (B = 32 default; B = 1: one example, one wave; B = 128: two waves, duplicate runs of about 64 in the
# vocabulary-2 fields; E = 16 with [64, 64, 32]; [9, 13, 5, 6]; six fields at E = 16, B = 96).
CASES = [_case("trajectory%d" % i, *t) for i, t in enumerate(TRAJECTORIES)]
CASES += [
    _case("partial second wave B=65", SMALL, 8, [16, 8], 65, 401),                            # 6.3e-4 / 3.9e-5
    _case("the largest concat", [3] * 32, 16, [64, 64, 64], 32, 727),                         # 1.0e-4 / 6.0e-5 (runs of about 10)
    _case("d_concat in the workspace", [3] * 32, 4, [64, 64, 64], 128, 755),                  # 7.5e-5 / 4.1e-5 (dcat_ws non-NULL; runs of about 43)
    _case("one id for every example", HAND, 8, [16, 8], 36, 403, batch="same"),               # 7.0e-4 / 2.2e-4
    _case("a row hit twice", HAND, 8, [16, 8], 36, 404, batch="pair"),                        # 1.4e-4 / 1.4e-3
    _case("a row hit three times", HAND, 8, [16, 8], 36, 405, batch="triple"),                # 8.7e-5 / 1.1e-4
]
# FLAGS (linear, mf, dnn): 111 1.6e-4 / 1.3e-4; 100, 010: no DNN; 001 3.8e-4 / 1.5e-4; 101 2.5e-4 / 2.5e-4; 011 2.7e-4 / 4.1e-4
_FLAG_SEEDS = [410, 411, 412, 463, 414, 415]
CASES += [_case("flags %d%d%d" % tuple(map(int, fl)), SMALL, 8, [16, 8], 64, s, use_linear=fl[0], use_mf=fl[1], use_dnn=fl[2])
          for s, fl in zip(_FLAG_SEEDS, FLAGS)]
CASES += [
    _case("sigmoid", SMALL, 8, [16, 8], 48, 420, activation="sigmoid", seed=3),
    _case("tanh dropout 0.2", SMALL, 8, [16, 8], 48, 421, activation="tanh", dropout=0.2, seed=3),
    _case("identity", SMALL, 8, [16, 8], 48, 422, activation=None, seed=3),
    _case("sigmoid dropout 0.2", SMALL, 8, [16, 8], 48, 423, activation="sigmoid", dropout=0.2, seed=3),
    _case("relu dropout 0.25 B=128", SMALL, 8, [32, 16], 128, 499, dropout=0.25, seed=7),     # 4.0e-5 / 6.9e-5
    _case("three hidden layers dropout 0.1", SMALL, 8, [16, 12, 8], 48, 425, dropout=0.1, seed=5),   # 5.1e-4 / 8.2e-5 (/ keep twice)
    _case("reduction sum", [9, 13, 5], 4, [8], 40, 426, reduction="sum"),                     # 1.3e-3 / 9.2e-4
    _case("no hidden layer", SMALL, 8, [], 48, 427),                                          # (the logits layer reads the concat: L = 1)
]
assert ML100K_VOCAB == TRAJECTORIES[0][0]


def hand_placed_ids(rng, vocab, B, batch):
    """Fields 1.. carry B distinct ids each, so that a row gradient's error is not averaged away; field 0: one id for every
    example, or distinct ids but for one row hit by exactly two / three non-adjacent examples."""
    assert min(vocab) >= B
    ids = np.stack([rng.permutation(v)[:B] for v in vocab], 1).astype(np.int32)
    hit = {"same": range(B), "pair": (3, B - 5), "triple": (2, B // 2 + 1, B - 3)}[batch]
    ids[list(hit), 0] = ids[hit[0], 0]
    assert int((ids[:, 0] == ids[hit[0], 0]).sum()) == len(hit)
    return ids


def run_case(case, make_engine, warm, hold=True):
    """make_engine(vocab, E, hidden, **kw) -> an engine with Adam(0.001).  Cold: the step from the loaded parameters
    (step 1, slots zero).  Warm: after WARM_STEPS fused steps on fresh batches the next step is checked."""
    kw = dict(case.kw)
    p, _, _, y = make_problem(case.seed, case.vocab, case.E, case.hidden, case.B, use_dnn=kw.get("use_dnn", True))
    m = make_engine(case.vocab, case.E, case.hidden, **kw)
    assert m.fused_step_ok(case.B), m._fused_step_limit(case.B)
    m.load_oracle_params(p)
    rng = np.random.default_rng(case.seed)
    if warm:
        for _ in range(WARM_STEPS):
            m.fused_train_step(dev(fresh_ids(rng, case.vocab, case.B), m.device), dev(y, m.device))
    ids = fresh_ids(rng, case.vocab, case.B) if case.batch == "fresh" else hand_placed_ids(rng, case.vocab, case.B, case.batch)
    kw.pop("seed", None)
    return check_step("%s %s" % (case.name, "warm" if warm else "cold"), m, ids, y, hold=hold, **kw)
