"""-m gpu: the optimizer kernels away from TF's default hyperparameters.  mi_opt_hparams and mi_sparse_catchup take their
betas, epsilon, l1, l2, decay and momentum at run time, and three pieces of device code are correct only for part of that
space: the exact replay's unscaled sqrt / divide (gated by catchup_params_in_range), the bounded replay (its error bound
is a statement about the betas: mi_catchup_bounded_runs) and the apply rules' terms that vanish at the defaults.

A  the exact replay, bit for bit against the literal fp32 sweep, one hyperparameter at a time across every limit of the
   gate, and every lower limit at once;
B  the bounded replay against the header's own bound, |w - w_sweep| <= 3 ulp(w) + 2e-6 sum_j |t_j| for every variable,
   wherever the entry accepts the flag (outside the region it ignores the flag: error 0);
D  the apply rules, bit for bit against oracle/optimizers.py, parameter and both slots;
E  a DeepFM trained with Adam(beta1 = 0.5, beta2 = 0.9, epsilon = 1e-3) in both catch-up modes against the oracle.

References are numpy fp32 sweeps (tests/util.py: catchup_sweep), made once per hyperparameter set and shared by the
embedding widths (E = 8 reads the first 8 columns: the sweep is elementwise)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from oracle import deepfm as O
from oracle import optimizers as OO
from tests.cases import OPTIMIZER_HPARAM_IDS, OPTIMIZER_HPARAM_SETS, _hip_engine, ftrl_gradients
from tests.util import (_chk, _compare_vars, _p, _st, adam_lr_table, bounded_catchup_error, catchup_sweep, dev, make_problem,
                        max_err_scaled)

pytestmark = pytest.mark.gpu

f32, u32 = np.float32, np.uint32
R = 1024                                  # 256 waves' worth of rows at E = 64 (16 lanes per row), 32 at E = 8 (2 lanes)
WIDTHS = (64, 8)
B1, B2, EPS = 0.9, 0.999, 1e-8


def below(x):
    return float(np.nextafter(f32(x), f32(0)))


def above(x):
    return float(np.nextafter(f32(x), f32(np.inf)))


def _frozen(*arrays):
    for a in arrays:
        a.flags.writeable = False
    return arrays


def _bits_equal(got, exp, what):
    g, e = got.cpu().numpy().view(u32), np.ascontiguousarray(exp).view(u32)
    assert np.array_equal(g, e), (what, int((g != e).sum()), "of", g.size)


# ---- A: the exact replay ------------------------------------------------------------------------------------------------------
STEP = 300
EDGE_GROUPS = [(-50, -49, -93, -92, None), (59, 60, 19, 20, None), (-50, -49, 19, 20, None), (59, 60, -93, -92, None),   # at the limits
               (-51, -50, -94, -93, None), (-45, -44, -88, -87, None),                                              # just outside, inside
               (-50, -49, -93, -92, 200), (-50, -49, -93, -92, 201)]                                                 # the step limit, and past it


@functools.lru_cache(maxsize=None)
def _edge_state():
    """The state recipe of test_hip_kernels.py::test_catchup_exact_at_range_edges at 1,024 rows: (m, v) from denormal to
    huge, 60 % of the rows well inside the fast loop's range (so waves mix both kinds), zeros, gaps 1 .. 299 (both sides of
    the 200-step limit), rows never applied, and groups of 64 rows — whole waves at either width — AT catchup_in_range's
    limits (|m| in [2^-50, 2^60], v in [2^-93, 2^20]), just outside them, and at gaps of exactly 200 and 201.  The wide
    part's (m, v) are column 1 of the rows': the same groups are whole waves of catchup_lin_k (one thread per row)."""
    rng = np.random.default_rng(12)
    E = 64
    w = rng.standard_normal((R, E)).astype(f32)
    m = (rng.choice([-1.0, 1.0], (R, E)) * 10.0 ** rng.uniform(-30, 1, (R, E))).astype(f32)
    v = (10.0 ** rng.uniform(-42, 2, (R, E))).astype(f32)
    calm = rng.random(R) < 0.6
    m[calm] = (rng.standard_normal((int(calm.sum()), E)) * 1e-6).astype(f32)
    v[calm] = (10.0 ** rng.uniform(-14, -8, (int(calm.sum()), E))).astype(f32)
    m[rng.random((R, E)) < 0.05] = 0.0
    v[rng.random((R, E)) < 0.05] = 0.0
    last = rng.integers(1, STEP, R).astype(np.int32)
    last[rng.random(R) < 0.1] = 0
    for gi, (mlo, mhi, vlo, vhi, gap) in enumerate(EDGE_GROUPS):
        g = slice(64 * gi, 64 * gi + 64)
        m[g] = (rng.choice([-1.0, 1.0], (64, E)) * 2.0 ** rng.uniform(mlo, mhi, (64, E))).astype(f32)
        v[g] = (2.0 ** rng.uniform(vlo, vhi, (64, E))).astype(f32)
        last[g] = STEP - (rng.integers(150, 201, 64) if gap is None else gap)
    lw = rng.standard_normal(R).astype(f32)
    return _frozen(w, m, v, lw, m[:, 1].copy(), v[:, 1].copy(), last)


def _lr_table(mode, b1, b2, n, at):
    """TF's schedule of (beta1, beta2), scaled so that lr_table[at] — the entry the gate reads — is exactly `mode`"""
    if mode == "lr 1e-3":
        return adam_lr_table(1e-3, b1, b2, n)
    target = {"2^-17": 2.0 ** -17, "below 2^-17": below(2.0 ** -17), "1.0": 1.0}[mode]
    shape = adam_lr_table(1.0, b1, b2, n).astype(np.float64)
    tab = (shape * (target / shape[at])).astype(f32)
    tab[at] = f32(target)
    return tab


@functools.lru_cache(maxsize=None)
def _edge_reference(b1, b2, eps, mode):
    w, m, v, lw, lm, lv, last = _edge_state()
    lr = _lr_table(mode, b1, b2, STEP + 1, STEP)
    return _frozen(lr) + (_frozen(*catchup_sweep(w, m, v, last, STEP, lr, b1, b2, eps)[:3]),
                          _frozen(*catchup_sweep(lw, lm, lv, last, STEP, lr, b1, b2, eps)[:3]))


def _run_catchup(catchup, state, last, lr, E, step_to, b1, b2, eps, flags, uniq=None):
    """catchup = the library's mi_sparse_catchup, on fresh device copies of (w, m, v, lw, lm, lv), rows cut to their first E
    columns; returns the device tensors [w, m, v, lw, lm, lv, stamps]"""
    w, m, v, lw, lm, lv = state
    d = [dev(np.array(a)) for a in (w[:, :E], m[:, :E], v[:, :E], lw, lm, lv, last)]      # (copies: the shared state is read-only)
    dlr = dev(np.array(lr))
    duq = dnu = None
    n_max = len(last)
    if uniq is not None:                                     # (slots past *num_uniq hold row 0: never read)
        n_max = len(uniq) + 36
        duq, dnu = dev(np.concatenate([uniq, np.zeros(36, np.int32)])), dev(np.array([len(uniq)], np.int32))
    _chk(catchup(*[_p(t) for t in d], _p(duq), _p(dnu), n_max, E, step_to, _p(dlr), b1, b2, eps, flags, 1, 0, _st()))
    torch.cuda.synchronize()
    return d


EXACT_SETS = ([(B1, B2, EPS, "lr 1e-3")] +
              [(b, B2, EPS, "lr 1e-3") for b in (below(0.9), 0.5, 0.0, 0.99)] +
              [(B1, b, EPS, "lr 1e-3") for b in (float(f32(0.99)), below(0.99), 0.9, 0.9999)] +
              [(B1, B2, e, "lr 1e-3") for e in (2.0 ** -40, below(2.0 ** -40), 1e-30, 1.0, above(1.0), 1e-3)] +
              [(B1, B2, EPS, mode) for mode in ("2^-17", "below 2^-17", "1.0")] +
              [(float(f32(0.9)), float(f32(0.99)), 2.0 ** -40, "2^-17"),        # every limit of the gate's hyperparameters at once
               (below(0.9), float(f32(0.99)), 2.0 ** -40, "2^-17"),            # ... and one of them missed
               (0.99, 0.9999, 1.0, "1.0"),                                      # every upper end
               (0.5, 0.9, 1e-3, "lr 1e-3")])                                    # the set of the end-to-end test


@pytest.mark.parametrize("b1,b2,eps,mode", EXACT_SETS, ids=["b1=%.9g b2=%.9g eps=%.9g %s" % s for s in EXACT_SETS])
def test_exact_catchup_is_the_sweep_bit_for_bit(lib, b1, b2, eps, mode):
    """Flags 0, all rows, slots and stamps written: w, m, v of the rows and of the wide part and the stamps as bit patterns,
    on both sides of every limit of catchup_params_in_range (steps <= 200, lr_last >= 2^-17, eps in [2^-40, 1], beta1 in
    [0.9, 1], beta2 in [0.99, 1]) — inside, the unscaled sqrt / divide run wherever a wave's (m, v) allow; outside, sqrtf
    and '/'.  Either way the result is the sweep's bits."""
    w, m, v, lw, lm, lv, last = _edge_state()
    lr, rows, wide = _edge_reference(b1, b2, eps, mode)
    assert mode == "lr 1e-3" or float(lr[STEP]) == {"2^-17": 2.0 ** -17, "below 2^-17": below(2.0 ** -17), "1.0": 1.0}[mode]
    for E in WIDTHS:
        d = _run_catchup(lib.mi_sparse_catchup, (w, m, v, lw, lm, lv), last, lr, E, STEP, b1, b2, eps, 0)
        for got, exp, what in zip(d[:3], rows, "wmv"):
            _bits_equal(got, exp[:, :E], ("rows", what, E))
        for got, exp, what in zip(d[3:6], wide, "wmv"):
            _bits_equal(got, exp, ("wide part", what, E))
        assert np.array_equal(d[6].cpu().numpy(), np.where(last < STEP, STEP, last)), E
    assert not np.array_equal(rows[0] if b1 else rows[1], w if b1 else m)     # (it had work; beta1 = 0: on m and v only)


@pytest.mark.parametrize("v_exp", [-93, 19])
def test_exact_catchup_with_every_lower_limit_of_the_fast_path_at_once(lib, v_exp):
    """The point the derivation above catchup_in_range ends at: constant lr_t = 2^-17, beta1 = 0.9f, beta2 = 0.99f,
    eps = 2^-40, whole waves with |m| in [2^-50, 2^-49] and v in [2^-93, 2^-92] (or [2^19, 2^20]), a gap of exactly 200 —
    numerators lr_t m down to 2^-98, their residuals 2^-24 below that, v beta2^k down to 2^-96.  The weights are sized
    to 64 first updates, so that the quotients' last bits reach them."""
    rng = np.random.default_rng(40 + abs(v_exp))
    E, gap = 64, 200
    b1, b2, eps = float(f32(0.9)), float(f32(0.99)), 2.0 ** -40
    lr = np.full(STEP + 2, 2.0 ** -17, f32)
    m = (rng.choice([-1.0, 1.0], (R, E)) * 2.0 ** rng.uniform(-50, -49, (R, E))).astype(f32)
    v = (2.0 ** rng.uniform(v_exp, v_exp + 1, (R, E))).astype(f32)
    assert np.abs(m).min() >= 2.0 ** -50 and np.abs(m).max() <= 2.0 ** -49 and v.min() >= 2.0 ** v_exp and v.max() <= 2.0 ** (v_exp + 1)
    first = 2.0 ** -17 * np.abs(m.astype(np.float64)) / (np.sqrt(v.astype(np.float64)) + eps)
    w = (rng.standard_normal((R, E)) * 64 * first).astype(f32)
    last = np.full(R, STEP - gap, np.int32)
    state = (w, m, v, w[:, 1].copy(), m[:, 1].copy(), v[:, 1].copy())
    ew, em, ev, moved = catchup_sweep(w, m, v, last, STEP, lr, b1, b2, eps)
    elw, elm, elv, _ = catchup_sweep(state[3], state[4], state[5], last, STEP, lr, b1, b2, eps)
    # the corner is reached, and from inside: the last numerators are far below 2^-96 but not below 2^-101, v stays above 2^-96
    num = np.abs(em).astype(np.float64) * 2.0 ** -17
    assert 2.0 ** -101 <= num.min() < 2.0 ** -96 and ev.min() >= 2.0 ** -96, (float(num.min()), float(ev.min()))
    assert (ew != w).mean() > 0.99                             # (the updates do reach the weights)
    for width in WIDTHS:
        d = _run_catchup(lib.mi_sparse_catchup, state, last, lr, width, STEP, b1, b2, eps, 0)
        for got, exp, what in zip(d[:6], (ew[:, :width], em[:, :width], ev[:, :width], elw, elm, elv), ("w", "m", "v", "lin w", "lin m", "lin v")):
            _bits_equal(got, exp, (what, width))
        assert (d[6].cpu().numpy() == STEP).all()


# ---- B: the bounded replay ----------------------------------------------------------------------------------------------------
BOUNDED_SETS = ([(B1, b, EPS) for b in (0.999, 0.99, 0.98, 0.95, 0.9, 0.5)] + [(b, B2, EPS) for b in (0.5, 0.99)] +
                [(B1, B2, e) for e in (1e-3, 1.0)] +
                [(0.5, 0.9, EPS),
                 (0.5, 0.98, EPS)])           # inside the region near its beta2 end: the carried reciprocal's e^3 is half the bound
GAPS = [(300, 150, 200), (1300, 1030, 1100)]  # (step_to, gaps from, to): the second runs the loop before the 1,024-step LDS window of lr_t


@functools.lru_cache(maxsize=None)
def _bounded_state(step_to, lo, hi):
    """The recipe of test_hip_kernels.py::test_bounded_catchup_stays_within_its_bound_of_the_sweep at 1,024 rows: (m, v) pairs
    spanning everything Adam can produce — gradient scales 2^-46 .. 2^10, whole waves at either end —, elements whose
    gradient has always been 0, an overflowed v, rows never applied and rows up to date."""
    rng = np.random.default_rng(31)
    E = 64
    sig = 2.0 ** rng.uniform(-46, 10, (R, 1))
    sig[:128] = 2.0 ** rng.uniform(-46, -45, (128, 1))
    sig[128:256] = 2.0 ** rng.uniform(9, 10, (128, 1))
    v = (sig ** 2 * rng.uniform(0.2, 1.0, (R, E))).astype(f32)
    m = (sig * rng.standard_normal((R, E)) * 0.5).astype(f32)
    zero = rng.random((R, E)) < 0.03
    m[zero] = 0.0; v[zero] = 0.0
    v[600:604, ::7] = np.inf
    w = (rng.standard_normal((R, E)) * 0.3).astype(f32)
    lw = (rng.standard_normal(R) * 0.3).astype(f32)
    lsig = 2.0 ** rng.uniform(-46, 10, R)
    lv = (lsig ** 2 * rng.uniform(0.2, 1.0, R)).astype(f32)
    lm = (lsig * rng.standard_normal(R) * 0.5).astype(f32)
    last = (step_to - rng.integers(lo, hi + 1, R)).astype(np.int32)
    last[rng.random(R) < 0.05] = 0
    last[rng.random(R) < 0.05] = step_to
    uniq = np.sort(rng.permutation(R)[:700]).astype(np.int32)
    return _frozen(w, m, v, lw, lm, lv, last, uniq)


@functools.lru_cache(maxsize=None)
def _bounded_reference(b1, b2, eps, step_to, lo, hi):
    w, m, v, lw, lm, lv, last, _ = _bounded_state(step_to, lo, hi)
    lr = adam_lr_table(1e-3, b1, b2, step_to + 1)
    return _frozen(lr) + (_frozen(*catchup_sweep(w, m, v, last, step_to, lr, b1, b2, eps)),
                          _frozen(*catchup_sweep(lw, lm, lv, last, step_to, lr, b1, b2, eps)))


def bounded_catchup_case(catchup, b1, b2, eps, step_to, lo, hi, check=True):
    """Both forms of a bounded call — flags 2: all rows, slots and stamps written; flags 3: the rows of a batch, deferred,
    only w moves — at both widths, through catchup(*arguments of mi_sparse_catchup) -> status.  Asserts (check) the
    header's bound for every variable of the rows and of the wide part and that m, v and the stamps are the exact chains;
    returns {(what, E, flags): (worst |err| / bound, share bit-identical, share within 1e-7 relative)}."""

    w, m, v, lw, lm, lv, last, uniq = _bounded_state(step_to, lo, hi)
    lr, (ew, em, ev, moved), (elw, elm, elv, lmoved) = _bounded_reference(b1, b2, eps, step_to, lo, hi)
    sel = np.zeros(R, bool); sel[uniq] = True
    out = {}
    for E in WIDTHS:
        d = _run_catchup(catchup, (w, m, v, lw, lm, lv), last, lr, E, step_to, b1, b2, eps, 2)
        tag = "b1=%g b2=%g eps=%g gaps %d-%d E=%d" % (b1, b2, eps, lo, hi, E)
        out["rows", E, 2] = bounded_catchup_error(d[0].cpu().numpy(), ew[:, :E], moved[:, :E], "rows, " + tag, check)
        out["wide", E, 2] = bounded_catchup_error(d[3].cpu().numpy(), elw, lmoved, "wide part, " + tag, check)
        for got, exp, what in zip((d[1], d[2], d[4], d[5]), (em[:, :E], ev[:, :E], elm, elv), ("m", "v", "lin m", "lin v")):
            _bits_equal(got, exp, (what, tag))
        assert np.array_equal(d[6].cpu().numpy(), np.where(last < step_to, step_to, last)), tag
        d = _run_catchup(catchup, (w, m, v, lw, lm, lv), last, lr, E, step_to, b1, b2, eps, 3, uniq)
        gw, gl = d[0].cpu().numpy(), d[3].cpu().numpy()
        out["rows", E, 3] = bounded_catchup_error(gw[sel], ew[sel, :E], moved[sel, :E], "rows (deferred slots), " + tag, check)
        out["wide", E, 3] = bounded_catchup_error(gl[sel], elw[sel], lmoved[sel], "wide part (deferred slots), " + tag, check)
        assert np.array_equal(gw[~sel], w[~sel, :E]) and np.array_equal(gl[~sel], lw[~sel]), tag
        for got, exp, what in zip(d[1:3] + d[4:6], (m[:, :E], v[:, :E], lm, lv), ("m", "v", "lin m", "lin v")):
            _bits_equal(got, exp, (what, "deferred", tag))
        assert np.array_equal(d[6].cpu().numpy(), last), tag
    return out


@pytest.mark.parametrize("step_to,lo,hi", GAPS, ids=["gaps %d-%d" % g[1:] for g in GAPS])
@pytest.mark.parametrize("b1,b2,eps", BOUNDED_SETS, ids=["b1=%g b2=%g eps=%g" % s for s in BOUNDED_SETS])
def test_bounded_catchup_meets_the_headers_bound_at_any_hyperparameters(lib, b1, b2, eps, step_to, lo, hi):
    """MI_CATCHUP_BOUNDED's published contract, wherever mi_sparse_catchup accepts the flag: for EVERY variable
    |w - w_sweep| <= 3 ulp(w) + 2e-6 sum_j |t_j|, with m, v and the stamps exact.  Where the library does not run the
    bounded form (mi_catchup_bounded_runs == 0) it ignores the flag and the result is the sweep's bits; at TF's defaults
    it does run it (not every variable is bit-identical), and after 150-200 replayed steps — what the header states them
    for — the distribution conditions hold too (>= 95 % bit-identical, >= 98 % within 1e-7 relative).  After 1,030-1,100
    steps they are printed: more steps, more roundings of w that can fall the other way (measured on an MI355X at the
    defaults: rows 96.0 % / 98.6 %, the 700 wide scalars of the deferred call 95.4 % / 97.9 %).
    Worst |err| / bound measured with and without the region: profiles/catchup_hparams_region.md."""
    res = bounded_catchup_case(lib.mi_sparse_catchup, b1, b2, eps, step_to, lo, hi)
    runs = int(lib.mi_catchup_bounded_runs(b1, b2, eps))
    defaults = (b1, b2, eps) == (B1, B2, EPS)
    assert runs == 1 or not defaults
    for key, (worst, same, within) in res.items():
        if not runs:
            assert same == 1.0 and worst == 0.0, (key, worst, same)
        if defaults and hi <= 200:
            assert same >= 0.95 and within >= 0.98, (key, same, within)
        if defaults:
            assert same < 1.0, (key, "the bounded form did not run")


# ---- D: the apply rules -------------------------------------------------------------------------------------------------------
def _both_ftrl_branches(hp, w, linear, what):
    if hp.name == "Ftrl" and hp.l1 > 0:
        inside = np.abs(linear) <= np.float32(hp.l1)
        assert inside.any() and (~inside).any(), (what, int(inside.sum()), inside.size)
        assert (w[inside] == 0).all() and (w[~inside] != 0).all(), what


@pytest.mark.parametrize("name,lr,kw", OPTIMIZER_HPARAM_SETS, ids=OPTIMIZER_HPARAM_IDS)
def test_dense_apply_bit_exact_at_other_hyperparameters(lib, name, lr, kw):
    """mi_dense_apply against oracle/optimizers.py, three steps: the parameter and BOTH slots, with the terms that vanish at
    TF's defaults switched on.  Ftrl with l1 > 0: both sides of |linear| <= l1 occur in every step."""
    from mi355x_rec.engine import OptimizerSpec
    rng = np.random.default_rng(21)
    n = 1000
    hp, spec = OO.Hyper(name, lr=lr, **kw), OptimizerSpec(name, lr, **kw)
    w = rng.standard_normal(n).astype(f32)
    s0, s1 = [a.copy() for a in OO.slot_init(hp, w)]
    assert tuple(float(a[0]) for a in (s0, s1)) == tuple(f32(x or 0.0) for x in spec.slot_init)
    dw, d0, d1 = dev(w), dev(s0), dev(s1)
    powers = OO.AdamPowers(hp, f32) if name == "Adam" else None
    for step in range(3):
        g = ftrl_gradients(rng, n)
        lr_t = powers.lr_t(hp.lr) if powers else 0.0
        OO.dense_apply(hp, w, s0, s1, g, lr_t)
        if powers:
            powers.finish()
        _both_ftrl_branches(hp, w, s1, step)
        h, dg = spec.hparams(float(lr_t)), dev(g)
        _chk(lib.mi_dense_apply(_p(dw), _p(d0), _p(d1) if name != "Adagrad" else None, _p(dg), n, C.byref(h), _st()))
        torch.cuda.synchronize()
    _bits_equal(dw, w, "param"); _bits_equal(d0, s0, "slot0")
    if name != "Adagrad":
        _bits_equal(d1, s1, "slot1")
        assert s1.any()


@pytest.mark.parametrize("name,lr,kw", OPTIMIZER_HPARAM_SETS, ids=OPTIMIZER_HPARAM_IDS)
def test_sparse_apply_and_catchup_bit_exact_at_other_hyperparameters(lib, name, lr, kw):
    """mi_sparse_apply (+ for Adam the exact lazy catch-up with the set's betas and epsilon) against the oracle's TF rule
    at E = 4 in the engine's record layout ([w | slot0 | slot1] per row, table_stride 3 E): rows that sit out steps,
    duplicates inside a batch; the table, the wide part and both slots of each."""
    from mi355x_rec.engine import AdamSchedule, OptimizerSpec
    rng = np.random.default_rng(4)
    Rr, E, steps, n = 50, 4, 7, 40
    hp, spec = OO.Hyper(name, lr=lr, **kw), OptimizerSpec(name, lr, **kw)
    W = rng.standard_normal((Rr, E)).astype(f32)
    L = rng.standard_normal((Rr, 1)).astype(f32)
    ws0, ws1 = [a.copy() for a in OO.slot_init(hp, W)]
    ls0, ls1 = [a.copy() for a in OO.slot_init(hp, L)]
    rec = torch.full((Rr, 3 * E), float("nan"), device="cuda")
    rec[:, :E] = dev(W); rec[:, E:2 * E] = dev(ws0); rec[:, 2 * E:] = dev(ws1)
    dW, d_ws0, d_ws1, tst = rec[:, :E], rec[:, E:2 * E], rec[:, 2 * E:], 3 * E
    dL, d_ls0, d_ls1 = dev(L[:, 0].copy()), dev(ls0[:, 0].copy()), dev(ls1[:, 0].copy())
    last = torch.zeros(Rr, dtype=torch.int32, device="cuda")
    adam, need1 = name == "Adam", name != "Adagrad"
    powers = OO.AdamPowers(hp, f32) if adam else None
    sched = AdamSchedule(spec, "cuda", 64) if adam else None
    for step in range(1, steps + 1):
        rows = rng.integers(0, Rr // 2 if step % 2 else Rr, n).astype(np.int32)
        rows[5] = rows[0]; rows[6] = rows[0]
        g, gl = ftrl_gradients(rng, (n, E), rows), ftrl_gradients(rng, (n, 1), rows)
        lr_t = powers.lr_t(hp.lr) if powers else 0.0
        touched = OO.sparse_apply(hp, W, ws0, ws1, rows, g, lr_t)
        OO.sparse_apply(hp, L, ls0, ls1, rows, gl, lr_t)
        if powers:
            powers.finish()
        _both_ftrl_branches(hp, W[touched], ws1[touched], ("table", step))
        _both_ftrl_branches(hp, L[touched], ls1[touched], ("wide part", step))
        r = dev(rows)
        se = torch.empty(n, dtype=torch.int32, device="cuda"); uq = torch.empty(n, dtype=torch.int32, device="cuda")
        sg = torch.empty(n + 1, dtype=torch.int32, device="cuda"); nu = torch.empty(1, dtype=torch.int32, device="cuda")
        wsb = torch.empty(lib.mi_sort_unique_workspace_bytes(n) + 256, dtype=torch.uint8, device="cuda")
        _chk(lib.mi_sort_unique_rows(_p(r), n, Rr, _p(se), _p(uq), _p(sg), _p(nu), _p(wsb), wsb.numel(), _st()))
        if adam and step > 1:
            assert sched.lr_t(step) == float(lr_t)
            _chk(lib.mi_sparse_catchup(_p(dW), _p(d_ws0), _p(d_ws1), _p(dL), _p(d_ls0), _p(d_ls1), _p(last), _p(uq), _p(nu), n, E,
                                       step - 1, _p(sched.table), hp.beta1, hp.beta2, hp.epsilon, 0, 1, tst, _st()))
        h = spec.hparams(float(lr_t))
        dg, dgl = dev(g), dev(gl[:, 0].copy())
        _chk(lib.mi_sparse_apply(_p(dW), _p(d_ws0), _p(d_ws1) if need1 else None, _p(dL), _p(d_ls0), _p(d_ls1) if need1 else None,
                                 _p(last) if adam else None, _p(uq), _p(sg), _p(se), _p(nu), n, _p(dg), _p(dgl), E, step,
                                 C.byref(h), 1, tst, 0, _st()))
        torch.cuda.synchronize()
    if adam:
        _chk(lib.mi_sparse_catchup(_p(dW), _p(d_ws0), _p(d_ws1), _p(dL), _p(d_ls0), _p(d_ls1), _p(last), None, None, Rr, E, steps,
                                   _p(sched.table), hp.beta1, hp.beta2, hp.epsilon, 0, 1, tst, _st()))
        torch.cuda.synchronize()
        assert (last.cpu().numpy() == steps).all()
    _bits_equal(dW.contiguous(), W, "table"); _bits_equal(dL, L[:, 0], "wide part")
    _bits_equal(d_ws0.contiguous(), ws0, "table slot0"); _bits_equal(d_ls0, ls0[:, 0], "wide slot0")
    if need1:
        _bits_equal(d_ws1.contiguous(), ws1, "table slot1"); _bits_equal(d_ls1, ls1[:, 0], "wide slot1")
        assert ws1.any() and ls1.any()


def test_ftrl_learning_rate_power_other_than_minus_a_half_is_refused(lib):
    """lr_power != -0.5 is not restated (csrc/optim.hip, check_hp): a non-zero status before any launch, the reason through
    mi_last_error, every buffer as it was — for the dense and the sparse apply."""
    from mi355x_rec.engine import OptimizerSpec
    rng = np.random.default_rng(8)
    h = OptimizerSpec("Ftrl", 0.05, lr_power=-0.4).hparams()
    n, E = 64, 4
    bufs = [dev(np.abs(rng.standard_normal((n, E))).astype(f32) + i) for i in (0, 1, 0, 0)] + \
           [dev(np.abs(rng.standard_normal(n)).astype(f32) + i) for i in (0, 1, 0, 0)]                  # (the accumulators: >= 1)
    before = [b.clone() for b in bufs]
    W, s0, s1, g, Lw, l0, l1, gl = bufs
    rc = lib.mi_dense_apply(_p(W), _p(s0), _p(s1), _p(g), n * E, C.byref(h), _st())
    assert rc != 0 and b"learning_rate_power" in lib.mi_last_error() and b"dense_apply" in lib.mi_last_error(), (rc, lib.mi_last_error())
    uq, sg, se = dev(np.arange(n, dtype=np.int32)), dev(np.arange(n + 1, dtype=np.int32)), dev(np.arange(n, dtype=np.int32))
    nu = dev(np.array([n], np.int32))
    rc = lib.mi_sparse_apply(_p(W), _p(s0), _p(s1), _p(Lw), _p(l0), _p(l1), None, _p(uq), _p(sg), _p(se), _p(nu), n, _p(g), _p(gl), E, 1,
                             C.byref(h), 1, 0, 0, _st())
    assert rc != 0 and b"learning_rate_power" in lib.mi_last_error() and b"sparse_apply" in lib.mi_last_error(), (rc, lib.mi_last_error())
    torch.cuda.synchronize()
    for a, b in zip(bufs, before):
        assert torch.equal(a, b)
    ok = OptimizerSpec("Ftrl", 0.05).hparams()                  # (and the same call with the default power is taken)
    _chk(lib.mi_dense_apply(_p(W), _p(s0), _p(s1), _p(g), n * E, C.byref(ok), _st()))
    torch.cuda.synchronize()
    assert not torch.equal(W, before[0])


# ---- E: end to end ------------------------------------------------------------------------------------------------------------
E2E_HP = dict(beta1=0.5, beta2=0.9, epsilon=1e-3)


@pytest.mark.parametrize("catchup", ["bounded", "exact"])
def test_deepfm_trains_with_non_default_adam_in_both_catchup_modes(catchup):
    """A small DeepFM with Adam(lr = 0.01, beta1 = 0.5, beta2 = 0.9, epsilon = 1e-3), 12 steps on random batches of 16 (most
    rows sit out most steps), against oracle.train_step with the same Hyper: the logits of every step within 1e-5, every
    variable within the project's 2e-6 after finalize_rows().  These betas are outside the bounded replay's region:
    catchup="bounded" is not refused, the library runs the exact form, and the one-launch local-order catch-up (bounded
    only) is not chosen.  No hidden pre-activation of the oracle comes within 1e-6 of 0 (asserted): no relu decision
    depends on summation order."""
    from mi355x_rec.engine import OptimizerSpec
    vocab, E, hidden, B = [50 + 3 * i for i in range(26)], 8, [16, 16], 16
    p, _, _, _ = make_problem(61, vocab, E, hidden, B)
    m = _hip_engine(vocab, E, hidden, optimizer=OptimizerSpec("Adam", 0.01, **E2E_HP), catchup=catchup)
    assert m.catchup == catchup and not m._bounded_runs() and not m._local_catchup(True, 4096 * len(vocab))
    m.load_oracle_params(p)
    st = O.TrainState(p, OO.Hyper("Adam", 0.01, **E2E_HP))
    rng = np.random.default_rng(62)
    margin, seen = np.inf, np.zeros(sum(vocab), bool)
    off = np.concatenate([[0], np.cumsum(vocab)])[:-1]
    for step in range(12):
        ids = np.stack([rng.integers(0, v, B) for v in vocab], 1).astype(np.int32)
        y = (rng.random(B) < 0.3).astype(np.uint8)
        seen[(ids + off[None, :]).ravel()] = True
        margin = min(margin, min(float(np.abs(q).min()) for q in O.forward(p, ids)["pre"]))
        loss_o, logit_o = O.train_step(p, st, ids, y)
        loss_g, logit_g = m.train_step(dev(ids), dev(y))
        err = max_err_scaled(logit_g.cpu().numpy(), logit_o)
        print("Adam(0.5, 0.9, 1e-3), catchup=%s, step %d: logits err %.3g" % (catchup, step, err))
        assert err < 1e-5, (step, err)
        assert abs(loss_g.item() - float(loss_o)) / abs(float(loss_o)) < 2e-5, step
    assert margin >= 1e-6, margin
    assert 0.5 < seen.mean() < 0.97                             # rows did sit out steps, and some were never touched
    m.finalize_rows()
    _compare_vars(m, p, 2e-6)
    assert m.step == 12
