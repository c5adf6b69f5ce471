"""-m gpu: the gradients of the one-launch train step (mi_train_step_fused, csrc/train_fused.hip: forward_block,
batch_block, sweep_block) against the oracle's backward in fp64, read from the only window the kernel has: the Adam slots
it writes.  The population step, the population evaluation and the ensemble paths are proved bit-identical to this step,
so what it gets wrong every member of every sweep gets wrong with the same bits.

Why slots and why one step: Adam's update is m / (sqrt(v) + eps), so the gradient's magnitude cancels in every trajectory
of weights — test_fused_gradients_cpu.py shows a gradient wrong by 1 % everywhere, and 1e-4 relative noise in any slot
class, passing test_hip_fused_step.py's assertions.  After one step from a known state m is linear in g and v quadratic.

The checker, its measure (tests.util.max_err_scaled per variable, every element of every row; bar max(1e-5, 4 x E32), E32
the fp32 oracle's own error, never taken from the device), the cases and their relu margins are in tests/fused_grad_check.py.
Each case runs from a cold state (step 1, slots zero) and from a warm one (the step after four fused steps on fresh
batches: m and v of many rows non-zero, untouched rows swept).  Every figure is printed (pytest -s) as
FGRAD <case> <variable> <slot> device ... fp32-oracle ... bar ...; the worst per case are in DESIGN.md section 11."""
import pytest

from tests import fused_grad_check as C
from tests.cases import _hip_engine

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("warm", [False, True], ids=["cold", "warm"])
@pytest.mark.parametrize("case", C.CASES, ids=[c.name for c in C.CASES])
def test_slots_after_one_step_match_the_fp64_oracle(case, warm):
    m_kw = dict(case.kw)
    rep = C.run_case(case, _hip_engine, warm)
    assert not rep.failures
    if m_kw.get("use_dnn", True):
        assert ("kernel_0", "m") in rep.figures and ("kernel_%d" % len(case.hidden), "v") in rep.figures
    assert (("table", "m") in rep.figures) == (m_kw.get("use_mf", True) or m_kw.get("use_dnn", True))
    assert (("lin_w", "v") in rep.figures) == m_kw.get("use_linear", True)
