"""-m gpu: MI_CATCHUP_LOCAL_ORDER — the train step's catch-up as ONE launch that orders its rows by staleness itself and
replays the wide part from the records it reads the stamps from — against the sequence it replaces
(mi_catchup_rows_by_gap, mi_sparse_catchup with the wide part alone, mi_sparse_catchup with the rows alone), bit for bit:
the per-row code of the two forms is the same, and results do not depend on the order of rows."""
import functools

import numpy as np
import pytest
import torch

from tests.util import _chk, _p, _st, dev, make_problem

pytestmark = pytest.mark.gpu

BOUNDED_DEFER, LOCAL = 3, 8
INVALID = -1                                         # MI_ERR_INVALID


def _chunk(lib):
    return int(lib.mi_catchup_local_chunk_rows())


def _plan(lib, n_max, U):
    """(workgroups, chunks per workgroup, rows per chunk) of a launch: the launcher's own arithmetic"""
    plan = np.zeros(3, np.int64)
    _chk(lib.mi_catchup_local_plan(n_max, U, plan.ctypes.data))
    return int(plan[0]), int(plan[1]), int(plan[2])


@functools.lru_cache(maxsize=None)
def _state(seed, R, E, st, step_to):             # (made once per shape, shared, never written)
    """table / m / v, the wide part's {w, m, v, stamp} (records of `st` = 4 words, or four arrays) and the stamps: mostly
    geometric gaps of mean 15, plus never-applied rows (stamp 0, m = v = 0), current rows (stamp = step_to), gaps above
    the ordering's clamp (63) and two above the LDS window of lr_t (1,024 steps); v = 0 and v = inf elements."""
    rng = np.random.default_rng(seed)
    f = np.float32
    w = (rng.standard_normal((R, E)) * 0.3).astype(f)
    m = (rng.standard_normal((R, E)) * 1e-3).astype(f)
    v = (rng.uniform(0.2, 1.0, (R, E)) * 1e-6).astype(f)
    lin = np.zeros((R, 4), f)
    lin[:, 0] = rng.standard_normal(R) * 0.3
    lin[:, 1] = rng.standard_normal(R) * 1e-3
    lin[:, 2] = rng.uniform(0.2, 1.0, R) * 1e-6
    zero = rng.random((R, E)) < 0.03
    m[zero] = 0.0; v[zero] = 0.0
    v[rng.random((R, E)) < 0.002] = np.inf
    lin[rng.random(R) < 0.03, 1:3] = 0.0
    lin[rng.random(R) < 0.002, 2] = np.inf
    gaps = np.minimum(rng.geometric(1.0 / 15.0, R), step_to - 1)
    far = rng.random(R) < 0.01
    gaps[far] = rng.integers(64, 200, int(far.sum()))
    stamps = (step_to - gaps).astype(np.int32)
    never = rng.random(R) < 0.05
    stamps[never] = 0; m[never] = 0.0; v[never] = 0.0; lin[never, 1:3] = 0.0
    stamps[rng.random(R) < 0.05] = step_to
    old = rng.choice(R, 2, replace=False)
    stamps[old] = step_to - np.array([1030, 1090], np.int32)
    return w, m, v, lin, stamps, old


def _device_state(w, m, v, lin, stamps, st):
    d = {"w": dev(w), "m": dev(m), "v": dev(v)}
    if st == 4:
        rec = lin.copy()
        rec.view(np.int32)[:, 3] = stamps
        d["rec"] = dev(rec)
        d["lw"], d["lm"], d["lv"] = d["rec"][:, 0], d["rec"][:, 1], d["rec"][:, 2]
        d["last"] = d["rec"].view(torch.int32)[:, 3]
    else:
        d["lw"], d["lm"], d["lv"] = dev(lin[:, 0].copy()), dev(lin[:, 1].copy()), dev(lin[:, 2].copy())
        d["last"] = dev(stamps)
    return d


def _catchup(lib, d, rows, nu, n_max, E, step_to, lr, flags, st, table=True, wide=True, beta1=0.9, beta2=0.999, eps=1e-8):
    return lib.mi_sparse_catchup(_p(d["w"]) if table else None, _p(d["m"]) if table else None, _p(d["v"]) if table else None,
                                 _p(d["lw"]) if wide else None, _p(d["lm"]) if wide else None, _p(d["lv"]) if wide else None,
                                 _p(d["last"]), _p(rows), _p(nu), n_max, E, step_to, _p(lr), beta1, beta2, eps, flags, st, 0, _st())


def _todays_sequence(lib, d, rows, nu, n_max, E, step_to, lr, st, wide, **hp):
    by_gap = torch.empty(n_max, dtype=torch.int32, device="cuda")
    ws = torch.empty(lib.mi_sort_unique_workspace_bytes(n_max) + 256, dtype=torch.uint8, device="cuda")
    _chk(lib.mi_catchup_rows_by_gap(_p(rows), _p(nu), _p(d["last"]), n_max, step_to, st, _p(by_gap), _p(ws), ws.numel(), _st()))
    if wide:
        _chk(_catchup(lib, d, by_gap, nu, n_max, E, step_to, lr, BOUNDED_DEFER, st, table=False, **hp))
    _chk(_catchup(lib, d, by_gap, nu, n_max, E, step_to, lr, BOUNDED_DEFER, st, wide=False, **hp))


def _same(a, b):
    for k in a:
        x, y = a[k].contiguous().view(torch.int32), b[k].contiguous().view(torch.int32)
        assert torch.equal(x, y), (k, int((x != y).sum()))


_LR = {}


def _lr(step_to):
    if step_to not in _LR:
        s = np.arange(step_to + 2)
        _LR[step_to] = dev((1e-3 * np.sqrt(1 - 0.999 ** s) / np.maximum(1 - 0.9 ** s, 1e-30)).astype(np.float32))
    return _LR[step_to]


def _u_values(ch):
    return {"one": 1, "chunk-1": ch - 1, "chunk": ch, "3chunks+37": 3 * ch + 37}


@pytest.mark.parametrize("wide", [True, False])
@pytest.mark.parametrize("st", [4, 1])
@pytest.mark.parametrize("E", [64, 8])
@pytest.mark.parametrize("u_name", ["one", "chunk-1", "chunk", "3chunks+37"])
def test_local_order_equals_todays_sequence_bitwise(lib, u_name, E, st, wide):
    _local_order_against_todays_sequence(lib, u_name, E, st, wide)


HPARAMS = [dict(beta1=0.5, beta2=0.999, eps=1e-3),          # not TF's defaults, and the library still runs the bounded form
           dict(beta1=0.9, beta2=0.9, eps=1e-8)]            # outside the bounded form's region (mi_catchup_bounded_runs)


@pytest.mark.parametrize("hp", HPARAMS, ids=["bounded runs", "bounded does not run"])
def test_local_order_at_other_hyperparameters(lib, hp):
    """Where the library runs the bounded form, the one launch equals the three-call sequence bit for bit at those
    hyperparameters too.  Where it does not, the sequence's calls ignore MI_CATCHUP_BOUNDED (the exact form runs) and the
    one launch, which has no exact form, is REFUSED before anything is written: the caller — engine._local_catchup asks
    mi_catchup_bounded_runs — runs the sequence."""
    runs = bool(lib.mi_catchup_bounded_runs(hp["beta1"], hp["beta2"], hp["eps"]))
    assert runs == (hp["beta2"] == 0.999)
    if runs:
        _local_order_against_todays_sequence(lib, "chunk", 64, 4, True, **hp)
        return
    R, E, st, step_to = 20_000, 64, 4, 1200
    U = _chunk(lib)
    w, m, v, lin, stamps, _ = _state(1000 + E + st, R, E, st, step_to)
    rows_np = np.sort(np.random.default_rng(U + E).choice(R, U, replace=False)).astype(np.int32)
    rows, nu, lr = dev(rows_np), dev(np.array([U], np.int32)), _lr(step_to)
    a, b = _device_state(w, m, v, lin, stamps, st), _device_state(w, m, v, lin, stamps, st)
    before = {k: t.clone() for k, t in b.items()}
    rc = _catchup(lib, b, rows, nu, U, E, step_to, lr, BOUNDED_DEFER | LOCAL, st, **hp)
    torch.cuda.synchronize()
    assert rc == INVALID and b"mi_catchup_bounded_runs" in lib.mi_last_error(), (rc, lib.mi_last_error())
    _same(before, b)
    _todays_sequence(lib, a, rows, nu, U, E, step_to, lr, st, True, **hp)      # (taken, and it has work)
    torch.cuda.synchronize()
    assert not torch.equal(a["w"], before["w"]) and not torch.equal(a["lw"], before["lw"])


def _local_order_against_todays_sequence(lib, u_name, E, st, wide, **hp):
    R, step_to = 20_000, 1200
    U = _u_values(_chunk(lib))[u_name]
    if u_name == "3chunks+37":
        # the grid cap: a workgroup walks >= 3 chunks, and the last chunk of the list is partial
        G, per_wg, rows = _plan(lib, U + 19, U)
        assert per_wg >= 3 and 0 < U - (G * per_wg - 1) * rows < rows <= _chunk(lib)
    w, m, v, lin, stamps, old = _state(1000 + E + st, R, E, st, step_to)
    rng = np.random.default_rng(U + E)
    if U > 4:                                                         # the two rows older than the lr_t window are in the batch
        rows_np = np.concatenate([old, rng.choice(np.setdiff1d(np.arange(R), old), U - 2, replace=False)])
    else:
        rows_np = rng.choice(R, U, replace=False)
    rows_np = np.sort(rows_np).astype(np.int32)
    assert len(np.unique(rows_np)) == U
    n_max = U + 19                                                    # (slots past *num_uniq hold a row that is not in the batch)
    spare = np.setdiff1d(np.arange(R), rows_np)
    spare = int(spare[(stamps[spare] > 0) & (stamps[spare] < step_to)][0])      # (it would be replayed if it were read)
    rows = dev(np.concatenate([rows_np, np.full(n_max - U, spare, np.int32)]))
    nu = dev(np.array([U], np.int32))
    lr = _lr(step_to)
    a, b = _device_state(w, m, v, lin, stamps, st), _device_state(w, m, v, lin, stamps, st)
    _todays_sequence(lib, a, rows, nu, n_max, E, step_to, lr, st, wide, **hp)
    _chk(_catchup(lib, b, rows, nu, n_max, E, step_to, lr, BOUNDED_DEFER | LOCAL, st, wide=wide, **hp))
    torch.cuda.synchronize()
    _same(a, b)
    # it had work, and only on the rows of the batch; m, v, stamps as they were
    sel = np.zeros(R, bool); sel[rows_np] = True
    gw = b["w"].cpu().numpy()
    assert np.array_equal(gw[~sel].view(np.uint32), w[~sel].view(np.uint32))
    if U > 4:
        assert (gw[sel] != w[sel]).any()
    assert np.array_equal(b["m"].cpu().numpy().view(np.uint32), m.view(np.uint32))
    assert np.array_equal(b["v"].cpu().numpy().view(np.uint32), v.view(np.uint32))
    assert np.array_equal(b["last"].cpu().numpy(), stamps)
    glw = b["lw"].cpu().numpy()
    assert np.array_equal(glw[~sel].view(np.uint32), lin[~sel, 0].view(np.uint32))
    if not wide:
        assert np.array_equal(glw.view(np.uint32), lin[:, 0].view(np.uint32))


def test_local_order_with_chunks_of_nearly_the_full_length(lib):
    """Chunks longer than 3/4 of the largest window (every thread of the prologue holds four rows) need the full grid and
    2.4 M rows: the state is made on the device, E = 8."""
    R, E, st, step_to = 2_500_000, 8, 4, 300
    U = 3 * 1024 * 800 + 37
    G, per_wg, rows = _plan(lib, U, U)
    assert G == 1024 and per_wg == 3 and 768 < rows <= _chunk(lib)
    g = torch.Generator(device="cuda"); g.manual_seed(3)
    w = torch.randn(R, E, device="cuda", generator=g) * 0.3
    m = torch.randn(R, E, device="cuda", generator=g) * 1e-3
    v = torch.rand(R, E, device="cuda", generator=g) * 1e-6 + 1e-9
    rec = torch.randn(R, 4, device="cuda", generator=g) * 1e-3
    rec[:, 2] = rec[:, 2].abs() * 1e-3 + 1e-9
    gaps = torch.empty(R, device="cuda").geometric_(1.0 / 15.0, generator=g).clamp_(0, step_to - 1).to(torch.int32)
    rec.view(torch.int32)[:, 3] = step_to - gaps
    rows_t = torch.randperm(R, device="cuda", generator=g)[:U].to(torch.int32).sort().values.contiguous()
    nu, lr = dev(np.array([U], np.int32)), _lr(step_to)

    def state():
        r = rec.clone()
        return {"w": w.clone(), "m": m, "v": v, "rec": r, "lw": r[:, 0], "lm": r[:, 1], "lv": r[:, 2], "last": r.view(torch.int32)[:, 3]}

    a, b = state(), state()
    _todays_sequence(lib, a, rows_t, nu, U, E, step_to, lr, st, True)
    _chk(_catchup(lib, b, rows_t, nu, U, E, step_to, lr, BOUNDED_DEFER | LOCAL, st))
    torch.cuda.synchronize()
    assert torch.equal(a["w"].view(torch.int32), b["w"].view(torch.int32))
    assert torch.equal(a["rec"].view(torch.int32), b["rec"].view(torch.int32))
    assert not torch.equal(b["w"], w) and not torch.equal(b["rec"][:, 0], rec[:, 0])
    assert torch.equal(b["rec"][:, 1:].view(torch.int32), rec[:, 1:].view(torch.int32))


def test_local_order_under_a_registered_step_state(lib):
    """a captured step: step_to <- state->step - 1, whatever the argument says"""
    R, E, st, step_to = 20_000, 64, 4, 1200
    U = 3 * _chunk(lib) + 37
    w, m, v, lin, stamps, _ = _state(77, R, E, st, step_to)
    rows_np = np.sort(np.random.default_rng(5).choice(R, U, replace=False)).astype(np.int32)
    rows, nu, lr = dev(rows_np), dev(np.array([U], np.int32)), _lr(step_to)
    a, b = _device_state(w, m, v, lin, stamps, st), _device_state(w, m, v, lin, stamps, st)
    state = torch.zeros(16, dtype=torch.uint8, device="cuda")
    state.view(torch.int32)[0] = step_to + 1
    _chk(lib.mi_set_step_state(_p(state)))
    try:
        _todays_sequence(lib, a, rows, nu, U, E, 3, lr, st, True)
        _chk(_catchup(lib, b, rows, nu, U, E, 3, lr, BOUNDED_DEFER | LOCAL, st))
        torch.cuda.synchronize()
    finally:
        _chk(lib.mi_set_step_state(None))
    _same(a, b)
    c = _device_state(w, m, v, lin, stamps, st)                      # and that is the eager call with step_to itself
    _chk(_catchup(lib, c, rows, nu, U, E, step_to, lr, BOUNDED_DEFER | LOCAL, st))
    torch.cuda.synchronize()
    _same(b, c)
    assert not torch.equal(c["w"], dev(w))


@pytest.mark.parametrize("case", ["no bounded", "no defer", "no uniq_rows", "no table", "keep stamps"])
def test_local_order_refuses_every_other_combination(lib, case):
    R, E, st, step_to = 3000, 16, 4, 300
    w, m, v, lin, stamps, _ = _state(3, R, E, st, 1200)
    stamps = np.minimum(stamps, step_to)
    d = _device_state(w, m, v, lin, stamps, st)
    before = {k: t.clone() for k, t in d.items()}
    rows, nu, lr = dev(np.arange(0, 2000, 2, dtype=np.int32)), dev(np.array([1000], np.int32)), _lr(step_to)
    flags = {"no bounded": LOCAL | 1, "no defer": LOCAL | 2, "keep stamps": LOCAL | 3 | 4}.get(case, LOCAL | 3)
    rc = _catchup(lib, d, None if case == "no uniq_rows" else rows, None if case == "no uniq_rows" else nu,
                  R if case == "no uniq_rows" else 1000, E, step_to, lr, flags, st, table=case != "no table")
    torch.cuda.synchronize()
    assert rc == INVALID, (case, rc)
    _same(before, d)


def _two_engines(local_values):
    from mi355x_rec.engine import DeepFM, OptimizerSpec
    vocab, E, hidden, B = [3000] * 4, 16, [32, 16], 4096
    p, _, _, _ = make_problem(17, vocab, E, hidden, B)
    ms = []
    for val in local_values:
        m = DeepFM(vocab, embedding_size=E, hidden_units=hidden, optimizer=OptimizerSpec("Adam", 0.001), dropout=0.1, seed=5,
                   catchup="bounded")
        m.LOCAL_CATCHUP = val
        m.load_oracle_params(p)
        ms.append(m)
    rng = np.random.default_rng(9)
    # ids from a window of 500 per field: a row of a batch sat out 1 .. 5 steps
    batches = [dev(np.stack([(rng.integers(0, 6) * 500 + rng.integers(0, 500, B)) for _ in vocab], 1).astype(np.int32))
               for _ in range(7)]
    ys = [dev((rng.random(B) < 0.3).astype(np.uint8)) for _ in range(7)]
    return ms, batches, ys


def _same_variables(a, b):
    a.finalize_rows(); b.finalize_rows()
    for k in ("table", "t_s0", "t_s1", "lin_state", "dense"):
        assert torch.equal(getattr(a, k), getattr(b, k)), k


def test_engine_with_and_without_local_catchup_is_bitwise_the_same_training():
    (new, old), batches, ys = _two_engines([True, False])
    launches = {"new": 0, "old": 0}
    for name, m in (("new", new), ("old", old)):
        f = m._rows_by_gap
        m._rows_by_gap = lambda *a, _f=f, _n=name, **kw: (launches.__setitem__(_n, launches[_n] + 1), _f(*a, **kw))[1]
    for i in range(6):
        assert new._local_catchup(True, batches[i].numel()) and not old._local_catchup(True, batches[i].numel())
        ln, gn = new.train_step(batches[i], ys[i], next_ids=batches[i + 1])
        lo, go = old.train_step(batches[i], ys[i], next_ids=batches[i + 1])
        assert torch.equal(ln, lo) and torch.equal(gn, go), i
        assert new._presorted["by_gap_step"] == new.step and new._presorted["by_gap"] is None
    assert launches["new"] == 0 and launches["old"] >= 5              # no staleness pass in local-order mode
    _same_variables(new, old)


def test_engine_graph_steps_with_and_without_local_catchup_are_bitwise_the_same():
    (new, old), batches, ys = _two_engines([True, False])
    for i in range(4):
        ln, gn = new.graph_train_step(batches[i], ys[i])
        lo, go = old.graph_train_step(batches[i], ys[i])
        assert torch.equal(ln, lo) and torch.equal(gn, go), i
    assert new._graph is not None and old._graph is not None
    _same_variables(new, old)


def test_engine_outside_the_bounded_region_trains_with_the_exact_form():
    """catchup="bounded" with Adam(beta2 = 0.9) — betas the bounded replay's error bound does not cover — at a batch size
    where the default engine takes the one-launch catch-up: not refused, not the one launch (the library would refuse
    it), and bit for bit the training of catchup="exact"."""
    from mi355x_rec.engine import DeepFM, OptimizerSpec
    vocab, E, hidden, B = [3000] * 4, 16, [32, 16], 4096
    p, _, _, _ = make_problem(17, vocab, E, hidden, B)
    ms = []
    for mode in ("bounded", "exact"):
        m = DeepFM(vocab, embedding_size=E, hidden_units=hidden, optimizer=OptimizerSpec("Adam", 0.001, beta2=0.9), dropout=0.1, seed=5,
                   catchup=mode)
        m.load_oracle_params(p)
        ms.append(m)
    bounded, exact = ms
    rng = np.random.default_rng(9)
    batches = [dev(np.stack([(rng.integers(0, 6) * 500 + rng.integers(0, 500, B)) for _ in vocab], 1).astype(np.int32)) for _ in range(5)]
    ys = [dev((rng.random(B) < 0.3).astype(np.uint8)) for _ in range(5)]
    assert not bounded._bounded_runs() and not bounded._local_catchup(True, batches[0].numel())
    for i in range(4):
        lb, gb = bounded.train_step(batches[i], ys[i], next_ids=batches[i + 1])
        le, ge = exact.train_step(batches[i], ys[i], next_ids=batches[i + 1])
        assert torch.equal(lb, le) and torch.equal(gb, ge), i
    _same_variables(bounded, exact)
    assert bounded.step == 4 and torch.isfinite(bounded.table).all()
