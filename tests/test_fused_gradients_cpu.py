"""CPU: tests/fused_grad_check.py's checker on the numpy restatement of mi_train_step_fused (NumpyKernels of
tests/cpu_kernels.py).  Every case of test_hip_fused_gradients.py passes here first — this is where the relu margins
and the E32 values are first seen (pytest -s) — and the checker FAILS when the step's backward is subtly wrong:

  * a gradient wrong by 1 % everywhere (the stand-in called with scale x 1.01, its loss put back);
  * one slot class at a time (t_s0, l_s0, d_s0, then the v's) multiplied by 1 + 1e-4 N(0, 1) after the step.

Why the file exists — test_todays_assertions_pass_both_perturbations: the same two perturbations, five steps on the
[9, 13, 5, 6], E = 8, [16, 8], B = 64 model, PASS what the suite asserted before: every variable within 2e-6 of the
oracle's (_compare_vars / _check_vars) and every step's loss within 2e-5.  Adam's update is m / (sqrt(v) + eps): the
gradient's magnitude cancels."""
import numpy as np
import pytest

from mi355x_rec.engine import DeepFM, OptimizerSpec
from oracle import deepfm as O
from oracle import optimizers as OO
from tests import fused_grad_check as C
from tests.cpu_kernels import NumpyKernels
from tests.util import _check_vars, _t, make_problem

_SCALE, _LOSS = 30, 34                                       # positions in mi_train_step_fused's argument list
_SLOT_ARG = {"t_s0": 1, "t_s1": 2, "l_s0": 5, "l_s1": 6, "d_s0": 17, "d_s1": 18}
_SLOT_OF = {"t_s0": ("table", "m"), "t_s1": ("table", "v"), "l_s0": ("lin_w", "m"), "l_s1": ("lin_w", "v")}


class GradientOffByOnePercent(NumpyKernels):
    """every gradient of the step x 1.01 (dlogit carries `scale`); the reported loss is the unperturbed one"""

    def mi_train_step_fused(self, *a):
        a = list(a)
        a[_SCALE] = np.float32(a[_SCALE]) * np.float32(1.01)
        super().mi_train_step_fused(*a)
        a[_LOSS].numpy()[0] /= np.float32(1.01)


class NoisySlots(NumpyKernels):
    """after the step, one slot class x (1 + 1e-4 N(0, 1)) element by element"""

    def __init__(self, which):
        super().__init__()
        self.which = which
        self.rng = np.random.default_rng(1)

    def mi_train_step_fused(self, *a):
        super().mi_train_step_fused(*a)
        s = a[_SLOT_ARG[self.which]].numpy()
        s *= (1 + 1e-4 * self.rng.standard_normal(s.shape)).astype(np.float32)


def _maker(kernels=NumpyKernels):
    def make(vocab, E, hidden, **kw):
        return DeepFM(vocab, embedding_size=E, hidden_units=hidden, optimizer=OptimizerSpec("Adam", 0.001), device="cpu",
                      _kernels=kernels(), **kw)
    return make


@pytest.mark.parametrize("warm", [False, True], ids=["cold", "warm"])
@pytest.mark.parametrize("case", C.CASES, ids=[c.name for c in C.CASES])
def test_checker_passes_on_the_numpy_restatement(case, warm):
    rep = C.run_case(case, _maker(), warm)
    relu = case.kw.get("activation", "relu") == "relu" and case.kw.get("use_dnn", True) and case.hidden
    if relu:
        assert rep.margin >= 1e-5, rep.margin                # (the seed's margin on this state: fused_grad_check.CASES)
    assert len(rep.figures) >= 2 and all(np.isfinite(v).all() for v in rep.figures.values())


MUTATION_CASES = [C.CASES[0], C.CASES[4]]                    # the default model and the [9, 13, 5, 6] model
assert MUTATION_CASES[1].vocab == [9, 13, 5, 6] and MUTATION_CASES[1].B == 64


@pytest.mark.parametrize("warm", [False, True], ids=["cold", "warm"])
@pytest.mark.parametrize("case", MUTATION_CASES, ids=[c.name for c in MUTATION_CASES])
def test_checker_fails_a_gradient_wrong_by_one_percent(case, warm):
    rep = C.run_case(case, _maker(GradientOffByOnePercent), warm, hold=False)
    failed = {(f[0], f[1]) for f in rep.failures}
    # every variable's m and v; beyond them only weights (one step from the reference's own state shows some of them:
    # elements with |g| near eps / 0.03, and rows whose m and v had decayed) — never the loss, the logits or the stamps
    assert failed >= set(rep.figures), (failed, rep.failures)
    assert all(slot == "w" for _, slot in failed - set(rep.figures)), rep.failures
    assert min(err for err, _, _ in rep.figures.values()) > 5e-4
    with pytest.raises(AssertionError):
        C.run_case(case, _maker(GradientOffByOnePercent), warm)


@pytest.mark.parametrize("which", list(_SLOT_ARG))
@pytest.mark.parametrize("warm", [False, True], ids=["cold", "warm"])
@pytest.mark.parametrize("case", MUTATION_CASES, ids=[c.name for c in MUTATION_CASES])
def test_checker_fails_relative_noise_of_1e_4_in_one_slot_class(case, warm, which):
    rep = C.run_case(case, _maker(lambda: NoisySlots(which)), warm, hold=False)
    failed = {(f[0], f[1]) for f in rep.failures}
    slot = "m" if which.endswith("0") else "v"
    if which in _SLOT_OF:
        assert failed == {_SLOT_OF[which]}, rep.failures
    else:                                                    # the dense variables: each of them large enough to show 1e-4 N(0, 1)
        assert failed and all(s == slot and name not in ("table", "lin_w") for name, s in failed), rep.failures
        assert {name for name, _ in failed} >= {"kernel_0", "kernel_1"}
    with pytest.raises(AssertionError):
        C.run_case(case, _maker(lambda: NoisySlots(which)), warm)


@pytest.mark.parametrize("kernels", [GradientOffByOnePercent] + [pytest.param(w, id=w) for w in _SLOT_ARG])
def test_todays_assertions_pass_both_perturbations(kernels):
    """The reason this file exists: test_fused_step_cpu.test_fused_train_step_matches_oracle's assertions (the loss of
    every step within 2e-5, every variable within 2e-6 after five steps: what test_hip_fused_step.py asks of the
    kernel) on the [9, 13, 5, 6], E = 8, [16, 8], B = 64 trajectory, with a gradient wrong by 1 % everywhere and with
    1e-4 relative noise in each slot class after every step: all of them pass."""
    vocab, E, hidden, B, seed = C.TRAJECTORIES[4]
    assert vocab == [9, 13, 5, 6]
    p, _, _, y = make_problem(seed, vocab, E, hidden, B)
    make = _maker(kernels if isinstance(kernels, type) else (lambda: NoisySlots(kernels)))
    m = make(vocab, E, hidden)
    m.load_oracle_params(p)
    st = O.TrainState(p, OO.Hyper("Adam", 0.001))
    rng = np.random.default_rng(seed)
    for step in range(5):
        ids = C.fresh_ids(rng, vocab, B)
        lo, _ = O.train_step(p, st, ids, y)
        lg, _ = m.fused_train_step(_t(ids), _t(y))
        assert abs(lg.item() - float(lo)) < 2e-5 * abs(float(lo)), step
    _check_vars(m, p, 2e-6)


def test_which_cases_keep_d_concat_in_the_workspace():
    """The kernel's LDS plan restated (plan_model in csrc/train_fused.hip: rows, sumv, tq, lin, dl, the layers' outputs and
    d_concat must fit 160 KB - 1 KB, or d_concat goes to the workspace): of the envelope's two corners [3] * 32,
    [64, 64, 64] only E = 4, B = 128 leaves no room (186 KB); E = 16, B = 32 takes 99 KB and keeps d_concat in LDS, as
    every other case does."""
    def lds_bytes(case):
        B, F, E = case.B, len(case.vocab), case.E
        a4 = lambda n: (n + 3) // 4 * 4
        dnn = case.kw.get("use_dnn", True)
        layers = sum(a4(B * h) for h in list(case.hidden) + [1]) if dnn else 0
        return 4 * (a4(B * F) + 2 * a4(B * E) + 2 * a4(B) + layers + (a4(B * F * E) if dnn else 0))
    limit = 160 * 1024 - 1024
    in_ws = [c.name for c in C.CASES if lds_bytes(c) > limit]
    assert in_ws == ["d_concat in the workspace"], in_ws
    by_name = {c.name: c for c in C.CASES}
    assert lds_bytes(by_name["the largest concat"]) == 98688
