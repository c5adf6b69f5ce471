"""Numeric embedding columns in the one-launch step: the case table and the checks that test_fused_numeric_cpu.py (the numpy
stand-in, tests/fused_numeric_kernels.py) and test_hip_fused_numeric.py (the device) share, so that both sides state the
same thing.  Not a test file.

Shapes are the smallest at which the kernel can go wrong: one column of each kind; a few; 26 + 13 columns at E = 4, B = 32
(the canonical DeepFM dataset's columns, three hidden layers of 64); the concat at its budget exactly (26 + 6 columns at
E = 4, B = 128: LDS has no room for d_concat, it lies in the workspace); no hidden layer; each part switched off; B = 1
(one example), 32, 33 (odd, past a half wave); E = 16 once per shape.

x_num is drawn from a normal; its LAST column is scaled by 100 and one value of column 0 is exactly 0.

Bars.  Trajectory: tests/test_hip_fused_step.py's — loss 2e-5 relative, logits 5e-6 on identical weights and 5e-5 after
the first update (tests.util.max_err_scaled), every variable 2e-6 absolute, num_emb and lin_num included.  Other rules:
tests/fused_rules_cases.run_trajectory's — loss 2e-5 |loss| + 1e-6, logits 5e-5 max(1, max |logit|), variables 2e-5.
Gradients' window: tests/fused_grad_check.bar — max(1e-5, 4 x the fp32 oracle's own error against the fp64 oracle) on EVERY
element of the Adam m slot of num_emb and lin_num after one step from zero slots (m = (1 - beta1) g there: linear in the
gradient).  Every figure is printed before it is asserted (pytest -s): FNUM ..."""
import numpy as np

from oracle import deepfm as O
from oracle import optimizers as OO
from tests.fused_grad_check import bar
from tests.util import dev, max_err_scaled

VOCAB26 = [2, 2, 7, 2, 2, 2, 2, 2, 2, 2, 2, 3, 2, 200, 2, 2, 50, 8, 2, 2, 2, 2, 100, 2, 2, 100]

# name -> vocab, nd, hidden, flags (linear, mf, dnn)
SHAPES = {
    "one_of_each": ([11], 1, [16, 16], (True, True, True)),
    "three_and_two": ([9, 13, 5], 2, [16, 16], (True, True, True)),
    "no_hidden_layer": ([9, 13, 5], 2, [], (True, True, True)),
    "no_dnn": ([9, 13, 5], 2, [], (True, True, False)),
    "no_fm": ([9, 13, 5], 2, [16, 16], (True, False, True)),
    "no_linear": ([9, 13, 5], 2, [16, 16], (False, True, True)),
}
# (shape, E, B, seed): every shape at B = 1, 32, 33 with E = 4 and once with E = 16; then the concat near its budget
CASES = [(s, 4, b, 700 + 10 * i + j) for i, s in enumerate(SHAPES) for j, b in enumerate((1, 32, 33))]
CASES += [(s, 16, 32, 800 + i) for i, s in enumerate(SHAPES)]
SHAPES["budget_26_13"] = (VOCAB26, 13, [64, 64, 64], (True, True, True))
CASES.append(("budget_26_13", 4, 32, 900))
# B (F + nd) E = 16384 exactly, with three hidden layers of 64: LDS has no room for d_concat, it lies in the workspace
SHAPES["budget_exact"] = ([3] * 26, 6, [64, 64, 64], (True, True, True))
CASES.append(("budget_exact", 4, 128, 910))
CASE_IDS = ["%s-E%d-B%d" % c[:3] for c in CASES]

RELU_MARGIN = 1e-6

# the other rules: (optimizer, lr), (linear_optimizer, lr) or None — one case each at the shape three_and_two, E = 4, B = 32
RULES = {
    "adagrad": (("Adagrad", 0.05), None),
    "sgd": (("SGD", 0.05), None),
    "ftrl_wide_adagrad_deep": (("Adagrad", 0.05), ("Ftrl", 0.1)),
}


def draw_x(rng, B, nd, zero=True):
    x = rng.standard_normal((B, nd)).astype(np.float32)
    x[:, nd - 1] *= np.float32(100.0)
    if zero:
        x[B // 2, 0] = 0.0
    return x


def draw_ids(rng, vocab, B):
    ids = np.stack([rng.integers(0, v, B) for v in vocab], 1).astype(np.int32)
    if B > 1:
        ids[B // 2] = ids[0]
    return ids


def make_params(seed, vocab, E, hidden, nd, use_dnn=True):
    rng = np.random.default_rng(seed)
    p = O.init_params(rng, vocab, E, hidden, n_numeric=nd, dtype=np.float32, lin_scale=0.05, use_dnn=use_dnn)
    p.lin_bias[:] = 0.1
    for _, b in p.mlp:
        b[:] = (rng.standard_normal(b.shape) * 0.05).astype(np.float32)
    return p


def make_engine(vocab, E, hidden, nd, flags, device, kernels=None, hp=("Adam", 0.001), lin_hp=None, **kw):
    from mi355x_rec.engine import DeepFM, OptimizerSpec
    ul, um, ud = flags
    kw = dict(kw, n_numeric=nd, embedding_size=E, hidden_units=hidden, use_linear=ul, use_mf=um, use_dnn=ud,
              optimizer=OptimizerSpec(*hp), device=device, catchup="exact", fused_numeric=True)
    if lin_hp is not None:
        kw["linear_optimizer"] = OptimizerSpec(*lin_hp)
    if kernels is not None:
        kw["_kernels"] = kernels
    return DeepFM(vocab, **kw)


def compare(m, p, atol):
    """every variable of engine m against the oracle's p, num_emb and lin_num included; returns {name: largest difference}"""
    g = m.export_numpy()
    out = {}

    def hold(a, b, what):
        err = float(np.max(np.abs(np.asarray(a) - np.asarray(b)), initial=0.0))
        out[what] = max(out.get(what, 0.0), err)
    for f in range(len(p.emb)):
        if g.get("emb") is not None:
            hold(g["emb"][f], p.emb[f], "emb")
        if g.get("lin_w") is not None:
            hold(g["lin_w"][f], p.lin_w[f], "lin_w")
    for i, (k, b) in enumerate(g["mlp"]):
        hold(k, p.mlp[i][0], "kernel_%d" % i)
        hold(b, p.mlp[i][1], "bias_%d" % i)
    if m.use_linear:
        hold(g["lin_bias"][:1], p.lin_bias[:1], "lin_bias")
        assert "lin_num" in g, "the engine exports lin_num"
        hold(g["lin_num"], p.lin_num, "lin_num")
    assert "num_emb" in g, "the engine exports num_emb"
    hold(g["num_emb"], p.num_emb, "num_emb")
    bad = {k: v for k, v in out.items() if not v < atol}
    assert not bad, (bad, atol)
    return out


def run_trajectory(case, device, kernels=None, steps=5):
    """`steps` fused steps against the fp32 oracle at test_hip_fused_step's bars; returns (engine, oracle params)"""
    shape, E, B, seed = case
    vocab, nd, hidden, flags = SHAPES[shape]
    ul, um, ud = flags
    p = make_params(seed, vocab, E, hidden, nd, ud)
    m = make_engine(vocab, E, hidden, nd, flags, device, kernels)
    assert m.fused_step_ok(B), m._fused_step_limit(B)
    m.load_oracle_params(p)
    st = O.TrainState(p, OO.Hyper("Adam", 0.001))
    rng = np.random.default_rng(seed)
    margin = np.inf
    for s in range(steps):
        ids, x = draw_ids(rng, vocab, B), draw_x(rng, B, nd, zero=s % 2 == 0)
        y = (rng.random(B) < 0.3).astype(np.uint8)
        pre = O.forward(p, ids, x, ul, um, ud).get("pre", [])
        margin = min([margin] + [float(np.abs(q).min()) for q in pre])
        lo, logit_o = O.train_step(p, st, ids, y, x, ul, um, ud)
        lg, logit_g = m.fused_train_step(dev(ids, device), dev(y, device), dev(x, device))
        diff = abs(lg.item() - float(lo))                    # (a saturated batch of one example: the loss may be exactly 0)
        le = diff / abs(float(lo)) if float(lo) != 0.0 else (0.0 if diff == 0.0 else np.inf)
        ge = max_err_scaled(logit_g.cpu().numpy(), logit_o)
        print("FNUM %-28s step %d  loss %.6f err %.2e (bar 2e-05)  logits err %.2e (bar %.0e)  margin %.2e" % (
            "%s-E%d-B%d" % case[:3], s, float(lo), le, ge, 5e-6 if s == 0 else 5e-5, margin))
        assert le < 2e-5, (case, s, le)
        assert ge < (5e-6 if s == 0 else 5e-5), (case, s, ge)
        assert m._final_step == m.step == s + 1 and bool((m.last_step == m.step).all())
    if ud and hidden:
        assert margin >= RELU_MARGIN, (case, margin)
    worst = compare(m, p, 2e-6)
    print("FNUM %-28s variables after %d steps: %s (bar 2e-06)" % ("%s-E%d-B%d" % case[:3], steps,
                                                                    ", ".join("%s %.1e" % kv for kv in sorted(worst.items()))))
    return m, p


def run_rule(name, device, kernels=None, steps=3):
    """one of RULES at the shape three_and_two against the oracle at the rules' bars; under two rules lin_num must have moved
    by the WIDE rule (the oracle applies linear_optimizer to it, and the comparison holds it to that)"""
    hp, lin_hp = RULES[name]
    vocab, nd, hidden, flags = SHAPES["three_and_two"]
    E, B, seed = 4, 32, 950
    p = make_params(seed, vocab, E, hidden, nd)
    m = make_engine(vocab, E, hidden, nd, flags, device, kernels, hp=hp, lin_hp=lin_hp)
    assert m.fused_step_ok(B), m._fused_step_limit(B)
    m.load_oracle_params(p)
    lin_num0 = p.lin_num.copy()
    st = O.TrainState(p, OO.Hyper(*hp), None if lin_hp is None else OO.Hyper(*lin_hp))
    rng = np.random.default_rng(seed)
    for s in range(steps):
        ids, x = draw_ids(rng, vocab, B), draw_x(rng, B, nd)
        y = (rng.random(B) < 0.3).astype(np.uint8)
        lo, logit_o = O.train_step(p, st, ids, y, x)
        lg, logit_g = m.fused_train_step(dev(ids, device), dev(y, device), dev(x, device))
        loss_err = abs(lg.item() - float(lo))
        logit_err = float(np.max(np.abs(logit_g.cpu().numpy() - logit_o)))
        print("FNUM rule %-24s step %d  loss %.6f err %.2e (bar %.2e)  logits err %.2e (bar %.2e)" % (
            name, s + 1, float(lo), loss_err, 2e-5 * abs(float(lo)) + 1e-6, logit_err, 5e-5 * max(1.0, float(np.max(np.abs(logit_o))))))
        assert loss_err <= 2e-5 * abs(float(lo)) + 1e-6, (name, s)
        assert logit_err <= 5e-5 * max(1.0, float(np.max(np.abs(logit_o)))), (name, s)
    worst = compare(m, p, 2e-5)
    print("FNUM rule %-24s variables after %d steps: %s (bar 2e-05)" % (name, steps, ", ".join("%s %.1e" % kv for kv in sorted(worst.items()))))
    assert float(np.max(np.abs(p.lin_num - lin_num0))) > 1e-4, "lin_num did not move"
    return m, p


# ---- the gradients' window: the Adam m slot of num_emb and lin_num after one step from zero slots, against fp64 ------------------
GRAD_CASES = [c for c in CASES if c[2] != 1]
GRAD_IDS = ["%s-E%d-B%d" % c[:3] for c in GRAD_CASES]


def check_gradient_window(case, device, kernels=None):
    shape, E, B, seed = case
    vocab, nd, hidden, flags = SHAPES[shape]
    ul, um, ud = flags
    p0 = make_params(seed + 1, vocab, E, hidden, nd, ud)
    rng = np.random.default_rng(seed + 1)
    ids, x = draw_ids(rng, vocab, B), draw_x(rng, B, nd)
    y = (rng.random(B) < 0.3).astype(np.uint8)
    f32w = lambda v: float(np.float32(v))
    hp = OO.Hyper("Adam", f32w(0.001), beta1=f32w(0.9), beta2=f32w(0.999), epsilon=f32w(1e-8))
    ref = {}
    for dt in (np.float64, np.float32):
        p = p0.astype(dt)
        st = O.TrainState(p, hp)
        if dt is np.float64:
            pre = O.forward(p, ids, x.astype(dt), ul, um, ud).get("pre", [])
            margin = min([float(np.abs(q).min()) for q in pre] or [np.inf])
        O.train_step(p, st, ids, y, x.astype(dt), ul, um, ud)
        names = [n % i for i in range(len(p.mlp)) for n in ("kernel_%d", "bias_%d")] + ["lin_bias", "num_emb", "lin_num"]
        assert len(names) == len(st.dense), "Params.dense_list(): the MLP, the wide bias, num_emb, lin_num"
        ref[dt] = {n: s[0] for n, s in zip(names, st.dense)}
    if ud and hidden:
        assert margin >= RELU_MARGIN, (case, margin)
    m = make_engine(vocab, E, hidden, nd, flags, device, kernels)
    m.load_oracle_params(p0)
    assert not bool(m.d_s0.any()) and not bool(m.d_s1.any()), "zero slots"
    m.fused_train_step(dev(ids, device), dev(y, device), dev(x, device))
    got = {"num_emb": m.d_s0[m.num_emb_off:m.num_emb_off + nd * E].cpu().numpy().reshape(nd, E)}
    if ul:                                                           # (without a wide part lin_num is no variable of the model)
        got["lin_num"] = m.d_s0[m.lin_num_off:m.lin_num_off + nd].cpu().numpy()
    failures = []
    for name in sorted(got):
        assert got[name].shape == ref[np.float64][name].shape and np.isfinite(got[name]).all(), name
        err = max_err_scaled(got[name], ref[np.float64][name])
        e32 = max_err_scaled(ref[np.float32][name], ref[np.float64][name])
        print("FNUM fp64 %-28s %-8s m  step err %.2e  fp32-oracle %.2e  bar %.2e  margin %.2e" % (
            "%s-E%d-B%d" % case[:3], name, err, e32, bar(e32), margin))
        if not err < bar(e32):
            failures.append((name, err, e32, bar(e32)))
    assert not failures, (case, failures)
