"""The one-launch train step under every optimizer, two rules and the canned estimators' columns: the cases, the trajectory
against the oracle and the fp64 witness check that test_fused_rules_cpu.py (numpy stand-in) and test_hip_fused_rules.py
(device) share.  Not a test file.

Trajectory bar (tests/test_canned_parity._run's): loss <= 2e-5 |loss| + 1e-6, logits <= 5e-5 max(1, max |logit|) at every
step, every variable within 2e-5 after the steps, against oracle.deepfm.train_step with TrainState(p, hp, lin_hp) and the
host replica of the dropout masks.
Fp64 bar (tests/fused_grad_check.bar): max(1e-5, 4 x the fp32 oracle's own error against the fp64 oracle), per variable
in tests.util.max_err_scaled, on a witness that is linear or quadratic in the gradient:
  Adagrad  accumulator - its initial value (sum of g^2)      Ftrl     the `linear` slot (g - sigma w)
  RMSProp  ms (1 + (g^2 - 1)(1 - decay))                     SGD      (w before - w after) / lr  (= g)
Every figure is printed before it is asserted (pytest -s): FRULES ..."""
import math

import numpy as np

from oracle import deepfm as O
from oracle import optimizers as OO
from tests.fused_grad_check import bar
from tests.util import dev, dropout_mask, max_err_scaled

VOCAB, E, HIDDEN, B = [9, 13, 5, 6], 8, [16, 8], 64
DIMS, WIDE = [8, 3, 0, 4], [True, False, True, True]
ADAGRAD = ("Adagrad", 0.05)
FTRL4 = ("Ftrl", min(0.2, 1.0 / math.sqrt(len(VOCAB))))          # trainers/linear.py:30: min(0.2, 1 / sqrt(columns))

# name -> the model and its optimizers: flags (linear, mf, dnn), (optimizer, lr), (linear_optimizer, lr) or None, the rest of
# engine.DeepFM's arguments.  The first five are tests/test_canned_parity's cases of these names at the common shape.
CASES = {
    "linear_classifier_ftrl_sum": dict(flags=(True, False, False), hidden=[], hp=FTRL4, reduction="sum"),
    "dnn_classifier_adagrad_sum_dropout": dict(flags=(False, False, True), hp=ADAGRAD, dropout=0.1, reduction="sum"),
    "wide_deep_two_optimizers": dict(flags=(True, False, True), hp=ADAGRAD, lin_hp=FTRL4, dropout=0.1, reduction="sum"),
    "wide_and_deep_parts_on_different_columns_with_per_column_dimensions": dict(
        flags=(True, False, True), hp=ADAGRAD, lin_hp=("Ftrl", min(0.2, 1.0 / math.sqrt(3))), dropout=0.1, reduction="sum",
        field_dims=DIMS, wide_fields=WIDE),
    "two_different_adam_optimizers": dict(flags=(True, True, True), hp=("Adam", 0.001), lin_hp=("Adam", 0.02), seed=33),
    "deepfm_adagrad": dict(flags=(True, True, True), hp=ADAGRAD),
    "deepfm_ftrl": dict(flags=(True, True, True), hp=("Ftrl", 0.05)),
    "deepfm_rmsprop": dict(flags=(True, True, True), hp=("RMSProp", 0.001)),
    "deepfm_sgd": dict(flags=(True, True, True), hp=("SGD", 0.05)),
}
TRAJECTORY_NAMES = list(CASES)


def hyper(spec):
    return None if spec is None else OO.Hyper(spec[0], spec[1])


def make_engine(case, device, kernels=None, vocab=VOCAB, emb=E, engine_seed=3):
    """engine.DeepFM of a case (kernels: a stand-in instance for the CPU, None for the library)"""
    from mi355x_rec.engine import DeepFM, OptimizerSpec
    c = CASES[case] if isinstance(case, str) else case
    ul, um, ud = c["flags"]
    kw = dict(embedding_size=emb, hidden_units=c.get("hidden", HIDDEN), use_linear=ul, use_mf=um, use_dnn=ud,
              dropout=c.get("dropout", 0.0), reduction=c.get("reduction", "mean"), optimizer=OptimizerSpec(*c["hp"]),
              seed=engine_seed, numeric="embed" if um else "raw", field_dims=c.get("field_dims"), wide_fields=c.get("wide_fields"),
              device=device)
    if c.get("lin_hp") is not None:
        kw["linear_optimizer"] = OptimizerSpec(*c["lin_hp"])
    if kernels is not None:
        kw["_kernels"] = kernels
    return DeepFM(vocab, **kw)


def make_params(case, vocab=VOCAB, emb=E, seed=21):
    c = CASES[case] if isinstance(case, str) else case
    rng0 = np.random.default_rng(c.get("seed", seed))
    p = O.init_params(rng0, vocab, emb, c.get("hidden", HIDDEN), dtype=np.float32, lin_scale=0.05, use_dnn=c["flags"][2],
                      numeric="embed" if c["flags"][1] else "raw", field_dims=c.get("field_dims"), wide_fields=c.get("wide_fields"))
    p.lin_bias[:] = 0.1
    for _, b in p.mlp:
        b[:] = (rng0.standard_normal(b.shape) * 0.05).astype(np.float32)
    return p


def draw_batch(rng, vocab, batch):
    ids = np.stack([rng.integers(0, v, batch) for v in vocab], 1).astype(np.int32)
    if batch > 1:
        ids[batch // 2] = ids[0]                    # duplicates inside a batch
    return ids, (rng.random(batch) < 0.3).astype(np.uint8)


def compare(m, p, atol):
    """every variable of engine m against the oracle's p; returns the largest difference"""
    g = m.export_numpy()
    worst = 0.0

    def hold(a, b, what):
        nonlocal worst
        err = float(np.max(np.abs(a - b), initial=0.0))
        worst = max(worst, err)
        assert err < atol, (what, err, atol)
    for f in range(len(p.emb)):
        if g.get("emb") is not None:
            assert g["emb"][f].shape == p.emb[f].shape
            hold(g["emb"][f], p.emb[f], ("emb", f))
        if g.get("lin_w") is not None and g["lin_w"][f] is not None:       # (None: the column has no linear weight)
            hold(g["lin_w"][f], p.lin_w[f], ("lin_w", f))
    for i, (k, b) in enumerate(g["mlp"]):
        assert k.shape == p.mlp[i][0].shape
        hold(k, p.mlp[i][0], ("kernel", i))
        hold(b, p.mlp[i][1], ("bias", i))
    if m.use_linear:
        hold(g["lin_bias"][:1], p.lin_bias[:1], "lin_bias")
    return worst


def run_trajectory(name, case, device, kernels=None, vocab=VOCAB, emb=E, batch=B, steps=3, atol=2e-5):
    """`steps` fused steps of the case against the oracle at the trajectory bar; returns (engine, oracle params)"""
    c = CASES[case] if isinstance(case, str) else case
    ul, um, ud = c["flags"]
    hidden, dropout, reduction = c.get("hidden", HIDDEN), c.get("dropout", 0.0), c.get("reduction", "mean")
    p = make_params(c, vocab, emb)
    m = make_engine(c, device, kernels, vocab, emb)
    assert m.fused_step_ok(batch), m._fused_step_limit(batch)
    m.load_oracle_params(p)
    st = O.TrainState(p, hyper(c["hp"]), hyper(c.get("lin_hp")))
    rng = np.random.default_rng(c.get("seed", 21) + 1)
    keep = 1.0 - dropout
    for s in range(steps):
        ids, y = draw_batch(rng, vocab, batch)
        masks = [dropout_mask(m._layer_seed(i), batch, h, keep) for i, h in enumerate(hidden)] if (dropout and ud) else None
        lo, logit_o = O.train_step(p, st, ids, y, None, ul, um, ud, reduction, masks, numeric="embed" if um else "raw",
                                   keep_prob=keep, wide_fields=c.get("wide_fields"))
        lg, logit_g = m.fused_train_step(dev(ids, device), dev(y, device))
        loss_err = abs(lg.item() - float(lo))
        logit_err = float(np.max(np.abs(logit_g.cpu().numpy() - logit_o)))
        print("FRULES %-40s step %d  loss %.6f err %.2e (bar %.2e)  logits err %.2e (bar %.2e)" % (
            name, s + 1, float(lo), loss_err, 2e-5 * abs(float(lo)) + 1e-6, logit_err, 5e-5 * max(1.0, float(np.max(np.abs(logit_o))))))
        assert loss_err <= 2e-5 * abs(float(lo)) + 1e-6, (name, s)
        assert logit_err <= 5e-5 * max(1.0, float(np.max(np.abs(logit_o)))), (name, s)
    worst = compare(m, p, atol)
    print("FRULES %-40s variables after %d steps: largest difference %.2e (bar %.0e)" % (name, steps, worst, atol))
    assert m.step == steps and m._final_step == steps
    return m, p


# ---- one step from the cold state against fp64 --------------------------------------------------------------------------------
RELU_MARGIN = 1e-5
# rule -> (its case, the seed of parameters and batch).  From the cold state the forward does not depend on the rule: seed 24
# keeps every fp64 hidden pre-activation 9.1e-4 from 0 (seed 21, the trajectories', only 4.5e-6); printed and asserted.
GRAD_RULES = {"Adagrad": ("deepfm_adagrad", 24), "Ftrl": ("deepfm_ftrl", 24), "RMSProp": ("deepfm_rmsprop", 24),
              "SGD": ("deepfm_sgd", 24)}


def _oracle_step(c, p32, dt, ids, y):
    p = p32.astype(dt)
    hp = OO.Hyper(c["hp"][0], float(np.float32(c["hp"][1])))
    st = O.TrainState(p, hp)
    pre = O.forward(p, ids, None, *c["flags"]).get("pre", [])
    margin = min([float(np.abs(q).min()) for q in pre] or [np.inf])
    O.train_step(p, st, ids, y, None, *c["flags"], "mean")
    return p, st, margin


def _witness(kind, lr, w0, w1, s0, s1):
    if kind == "Adagrad":
        return s0 - 0.1
    if kind == "Ftrl":
        return s1
    if kind == "RMSProp":
        return s0
    return (w0.astype(np.float64) - w1.astype(np.float64)) / float(np.float32(lr))


def grad_margin(kind):
    """the smallest fp64 |hidden pre-activation| of the rule's case at the checked step"""
    case, seed = GRAD_RULES[kind]
    c = CASES[case]
    p = make_params(c, seed=seed)
    ids, y = draw_batch(np.random.default_rng(seed + 1), VOCAB, B)
    return _oracle_step(c, p, np.float64, ids, y)[2]


def check_gradients(kind, device, kernels=None):
    """one fused step of the rule's DeepFM from the cold state: the witness of every variable against the fp64 oracle"""
    case, seed = GRAD_RULES[kind]
    c = CASES[case]
    lr = c["hp"][1]
    p0 = make_params(c, seed=seed)
    ids, y = draw_batch(np.random.default_rng(seed + 1), VOCAB, B)
    p64, st64, margin = _oracle_step(c, p0, np.float64, ids, y)
    p32, st32, _ = _oracle_step(c, p0, np.float32, ids, y)
    print("FRULES fp64 %-8s smallest |pre-activation| %.2e (at least %.0e)" % (kind, margin, RELU_MARGIN))
    assert margin >= RELU_MARGIN, (kind, margin)
    m = make_engine(c, device, kernels)
    m.load_oracle_params(p0)
    m.fused_train_step(dev(ids, device), dev(y, device))
    cpu = lambda t: None if t is None else t.detach().cpu().numpy().astype(np.float32)
    cat = lambda parts: np.concatenate(parts, 0)
    zeros = lambda a: np.zeros_like(a)
    got = {"table": (cpu(m.table), cpu(m.t_s0), cpu(m.t_s1)), "lin_w": (cpu(m.lin_w), cpu(m.l_s0), cpu(m.l_s1)),
           "lin_bias": tuple(cpu(None if t is None else t[m.lin_bias_off:m.lin_bias_off + 1]) for t in (m.dense, m.d_s0, m.d_s1))}
    for i in range(len(m.layers)):
        got["kernel_%d" % i] = tuple(cpu(None if t is None else m.kernel(i, t)) for t in (m.dense, m.d_s0, m.d_s1))
        got["bias_%d" % i] = tuple(cpu(None if t is None else m.bias(i, t)) for t in (m.dense, m.d_s0, m.d_s1))

    def ref(p, st):
        names = [n % i for i in range(len(p.mlp)) for n in ("kernel_%d", "bias_%d")] + ["lin_bias"]
        out = {n: (w, s[0], s[1]) for n, w, s in zip(names, p.dense_list(), st.dense)}
        out["table"] = (cat(p.emb), cat([a for a, _ in st.emb]), cat([b for _, b in st.emb]))
        out["lin_w"] = (cat(p.lin_w), cat([a for a, _ in st.lin]), cat([b for _, b in st.lin]))
        return out
    r64, r32 = ref(p64, st64), ref(p32, st32)
    start = ref(p0, O.TrainState(p0, OO.Hyper(c["hp"][0], lr)))
    failures = []
    for name in sorted(got):
        w0 = start[name][0]
        fill = lambda t: [zeros(w0) if a is None else a for a in t]
        wit = lambda t: _witness(kind, lr, w0, *fill(t))
        dev_w, w64, w32 = wit(got[name]), wit(r64[name]), wit(r32[name])
        assert dev_w.shape == w64.shape, name
        err, e32 = max_err_scaled(dev_w, w64), max_err_scaled(w32, w64)
        print("FRULES fp64 %-8s %-9s step err %.2e  fp32-oracle %.2e  bar %.2e" % (kind, name, err, e32, bar(e32)))
        if not err < bar(e32):
            failures.append((name, err, e32, bar(e32)))
    assert not failures, (kind, failures)
