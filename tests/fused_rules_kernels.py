"""numpy stand-ins for mi_train_step_model and mi_train_group_plan_models (include/mi355x_rec.h) — TEST INFRASTRUCTURE ONLY,
not a test file.

FusedRulesKernels is tests/cpu_kernels.NumpyKernels plus the one-launch step under any of the five optimizers, two rules and
a subset of wide columns, so that the host code that reaches those entries (engine.fused_train_step, population, the canned
estimators' CLIs, trainers.sweep --optimizer) runs without a GPU.  Like the other fused stand-ins it is restated from the
header and the kernel's order of operations on its own: it calls no numpy of a layered entry and takes no update rule from
the oracle (the rules below are csrc/optim_rules.h, expression by expression).

  phases   rows; forward (the wide sum over the wide fields only); head; backward; apply
  apply    per DISTINCT touched row, entries summed in ascending entry order: the table record under hp, the wide record —
           only where the row's field is a wide one — under the wide rule; dense: the MLP under hp, the wide bias under the
           wide rule with its own dense slots
  sweep    records under Adam only: every untouched row one replay step with that rule's lr_t; stamps where there are any
  slots    one the rule does not keep is neither read nor written
A plan of mi_train_group_plan_models is kept in `plans` beside NumpyKernels' own, marked; mi_train_group_step and
mi_eval_group run such a plan here and hand any other to NumpyKernels."""
import numpy as np
import pytest
import torch

from mi355x_rec import _lib, engine
from tests.cpu_kernels import _ACT, NumpyKernels, _at, counters
from tests.util import MASK64, dropout_mask

F32 = np.float32
SLOTS = {0: 2, 1: 1, 2: 2, 3: 2, 4: 0}          # Adam, Adagrad, Ftrl, RMSProp, SGD


def rule(hp, lr_t, w, s0, s1, g, sparse):
    """dense_rule / sparse_rule of csrc/optim_rules.h on fp32 arrays, one rounding per operation; returns (w, s0, s1) — a slot
    the rule does not keep comes back as it came"""
    one, lr, k = F32(1), F32(hp.lr), hp.kind
    if k == 0:
        b1, b2, eps, lr_t = F32(hp.beta1), F32(hp.beta2), F32(hp.epsilon), F32(lr_t)
        if sparse:
            s0 = s0 * b1 + g * (one - b1)
            s1 = s1 * b2 + (g * g) * (one - b2)
            w = w - (lr_t * s0) / (np.sqrt(s1) + eps)
        else:
            s0 = s0 + (g - s0) * (one - b1)
            s1 = s1 + (g * g - s1) * (one - b2)
            w = w - (s0 * lr_t) / (np.sqrt(s1) + eps)
    elif k == 1:
        s0 = s0 + g * g
        w = w - (g * lr) * (one / np.sqrt(s0))
    elif k == 2:
        na = s0 + g * g
        s1 = s1 + (g - ((np.sqrt(na) - np.sqrt(s0)) / lr) * w)
        adj = np.minimum(np.maximum(s1, -F32(hp.l1)), F32(hp.l1))
        w = (adj - s1) / (np.sqrt(na) / lr + F32(2) * F32(hp.l2))
        s0 = na
    elif k == 3:
        s0 = s0 + (g * g - s0) * (one - F32(hp.decay))
        s1 = s1 * F32(hp.momentum) + (g * lr) / np.sqrt(s0 + F32(hp.epsilon))
        w = w - s1
    else:
        w = w - g * lr
    return w, s0, s1


def _copy_hp(hp):
    return _lib.OptHparams.from_buffer_copy(hp)


def decode(m):
    """a mi_fused_model_t on host memory as numpy views and scalars (slots the rules do not keep: None)"""
    E, R, ts, ls, nl, nd = m.E, m.R, m.table_stride or m.E, m.lin_stride, m.n_layers, m.n_dense
    emb, lin, two = bool(m.use_fm or m.use_dnn), bool(m.use_linear), bool(m.two_rules)
    hp = _copy_hp(m.hp)
    hpw = _copy_hp(m.hp_wide) if two else hp
    nt, nw = SLOTS[hp.kind], SLOTS[hpw.kind]
    assert not two or lin, "two_rules needs the wide part"
    assert not lin or m.wide_fields >> 32 == 0
    np_ = lambda t: None if t is None else t.numpy()
    at = lambda on, ptr, *a: np_(_at(ptr, *a)) if on else None
    d = dict(
        table=at(emb, m.table, R, F32, ts, E), t_m=at(emb and nt >= 1, m.t_m, R, F32, ts, E),
        t_v=at(emb and nt >= 2, m.t_v, R, F32, ts, E), lin_w=at(lin, m.lin_w, R, F32, ls),
        l_m=at(lin and nw >= 1, m.l_m, R, F32, ls), l_v=at(lin and nw >= 2, m.l_v, R, F32, ls),
        dense=at(True, m.dense, nd, F32), d_m=at(nt >= 1, m.d_m, nd, F32), d_v=at(nt >= 2, m.d_v, nd, F32),
        layer_off=at(True, m.layer_off, max(2 * nl, 1), np.int64), widths=at(True, m.widths, nl + 1, np.int32),
        hp=hp, hpw=hpw, E=E, R=R, nl=nl, act=m.activation, use_linear=lin, use_fm=bool(m.use_fm), use_dnn=bool(m.use_dnn),
        lin_bias_off=m.lin_bias_off, keep=F32(m.keep_prob), scale=F32(m.scale), seed_base=m.seed_base, wide=m.wide_fields,
        lr_table=at(hp.kind == 0 and bool(m.lr_table), m.lr_table, max(m.lr_table_len, 1), F32),
        lr_table_w=at(two and hpw.kind == 0 and bool(m.lr_table_wide), m.lr_table_wide, max(m.lr_table_wide_len, 1), F32))
    d["dw_m"] = at(nw >= 1, m.dw_m, nd, F32) if two else (d["d_m"] if nw >= 1 else None)
    d["dw_v"] = at(nw >= 2, m.dw_v, nd, F32) if two else (d["d_v"] if nw >= 2 else None)
    adam = (emb and hp.kind == 0) or (lin and hpw.kind == 0)
    assert m.last_step or not adam, "a part under Adam stamps every row"
    d["last_step"] = at(adam, m.last_step, R, np.int32, ls)
    for name, need in (("t_m", emb and nt >= 1), ("t_v", emb and nt >= 2), ("l_m", lin and nw >= 1), ("l_v", lin and nw >= 2),
                       ("d_m", nt >= 1), ("d_v", nt >= 2), ("dw_m", nw >= 1), ("dw_v", nw >= 2)):
        assert not need or d[name] is not None, "the rule keeps slot %s" % name
    return d


def forward(d, rows, labels, B, F, seed, keep, scale, train):
    """phases 0-2: (logits z, loss, and for the backward: dl, V, s, acts, Ws)"""
    E, nl, act, dn = d["E"], d["nl"], d["act"], d["dense"]
    emb = d["use_fm"] or d["use_dnn"]
    V = d["table"][rows] if emb else None                                 # [B, F, E]
    z = np.zeros(B, F32)
    if d["use_linear"]:
        acc = np.zeros(B, F32)
        for f in range(F):
            if (d["wide"] >> f) & 1:
                acc = acc + d["lin_w"][rows[:, f]]
        z = acc + dn[d["lin_bias_off"]]
    s = None
    if d["use_fm"]:
        s = V.sum(1, dtype=F32)
        z = z + F32(0.5) * (s * s - (V * V).sum(1, dtype=F32)).sum(1, dtype=F32)
    acts, Ws = [], []
    lo, wd = d["layer_off"], d["widths"]
    if d["use_dnn"]:
        h = V.reshape(B, F * E)
        for i in range(nl):
            W = dn[lo[2 * i]:lo[2 * i] + wd[i] * wd[i + 1]].reshape(wd[i], wd[i + 1])
            acts.append(h)
            Ws.append(W.copy())
            h = (h @ W + dn[lo[2 * i + 1]:lo[2 * i + 1] + wd[i + 1]]).astype(F32)
            if i + 1 < nl:
                h = _ACT[act](h).astype(F32)
                if train and keep < 1:
                    h = (h / keep) * dropout_mask((seed + 7919 * i) & MASK64, B, int(wd[i + 1]), keep)
        z = z + h[:, 0]
    y = labels.astype(F32)
    e = np.exp(-np.abs(z))
    loss = ((np.maximum(z, 0) - z * y + np.log1p(e)) * scale).sum(dtype=F32)
    dl = ((np.where(z >= 0, 1 / (1 + e), e / (1 + e)).astype(F32) - y) * scale).astype(F32)
    return z.astype(F32), loss, dl, V, s, acts, Ws


def step(d, field_off, ids, labels, B, F, seed, step_no, lr_t, lr_tw, logits, loss):
    """one step of the model d: what train_fused_k does to its buffers"""
    assert 1 <= B <= 128 and 1 <= F <= 32 and d["R"] <= 1 << 18 and d["nl"] <= 4 and step_no >= 1
    E, nl, act, dn, keep = d["E"], d["nl"], d["act"], d["dense"], d["keep"]
    hp, hpw, R = d["hp"], d["hpw"], d["R"]
    emb = d["use_fm"] or d["use_dnn"]
    if d["last_step"] is not None:
        assert step_no == 1 or bool((d["last_step"] == step_no - 1).all()), "every row must be current"
    rows = ids.astype(np.int64) + field_off[None, :]
    z, ls, dl, V, s, acts, Ws = forward(d, rows, labels, B, F, seed, keep, d["scale"], True)
    logits[:] = z
    loss[0] = ls
    lo, wd = d["layer_off"], d["widths"]
    gd = np.zeros(len(dn), F32)
    d_concat = None
    if d["use_dnn"]:
        dy = dl[:, None]
        for i in reversed(range(nl)):
            gd[lo[2 * i]:lo[2 * i] + wd[i] * wd[i + 1]] = (acts[i].T @ dy).reshape(-1)
            gd[lo[2 * i + 1]:lo[2 * i + 1] + wd[i + 1]] = dy.sum(0, dtype=F32)
            g = (dy @ Ws[i].T).astype(F32)
            if i:
                x = acts[i]                                            # the layer's stored output: act(pre) / keep, or 0
                if act == 1:
                    g = np.where(x > 0, g / keep, 0).astype(F32)
                else:
                    o = x * keep
                    der = {0: np.ones_like(o), 2: o * (1 - o), 3: 1 - o * o}[act]
                    g = np.where((keep < 1) & (x == 0), 0, (g / keep) * der).astype(F32)
                dy = g
            else:
                d_concat = g.reshape(B, F, E)
    # 4. apply, sparse: per field the distinct rows, entries in ascending order
    G = None
    if emb:
        G = np.zeros((B, F, E), F32)
        if d_concat is not None:
            G = G + d_concat
        if d["use_fm"]:
            G = G + dl[:, None, None] * (s[:, None, :] - V)
    touched = np.zeros(R, bool)
    touched[rows.reshape(-1)] = True
    zero = lambda like: np.zeros_like(like)
    for f in range(F):
        for r in np.unique(rows[:, f]):
            bs = np.flatnonzero(rows[:, f] == r)
            if emb:
                g = np.zeros(E, F32)
                for b in bs:
                    g = g + G[b, f]
                w = d["table"][r].copy()
                m = d["t_m"][r].copy() if d["t_m"] is not None else zero(w)
                v = d["t_v"][r].copy() if d["t_v"] is not None else zero(w)
                w, m, v = rule(hp, lr_t, w, m, v, g, True)
                d["table"][r] = w
                if d["t_m"] is not None:
                    d["t_m"][r] = m
                if d["t_v"] is not None:
                    d["t_v"][r] = v
            if d["use_linear"] and (d["wide"] >> f) & 1:
                gl = F32(0)
                for b in bs:
                    gl = F32(gl + dl[b])
                w = F32(d["lin_w"][r])
                m = F32(d["l_m"][r]) if d["l_m"] is not None else F32(0)
                v = F32(d["l_v"][r]) if d["l_v"] is not None else F32(0)
                w, m, v = rule(hpw, lr_tw, w, m, v, gl, True)
                d["lin_w"][r] = w
                if d["l_m"] is not None:
                    d["l_m"][r] = m
                if d["l_v"] is not None:
                    d["l_v"][r] = v
    # the sweep: records under Adam, untouched rows
    u = ~touched
    for on, h, lrt, W, M, Vv in ((emb and hp.kind == 0, hp, lr_t, d["table"], d["t_m"], d["t_v"]),
                                 (d["use_linear"] and hpw.kind == 0, hpw, lr_tw, d["lin_w"], d["l_m"], d["l_v"])):
        if on:
            M[u] = M[u] * F32(h.beta1)
            Vv[u] = Vv[u] * F32(h.beta2)
            W[u] = W[u] - (F32(lrt) * M[u]) / (np.sqrt(Vv[u]) + F32(h.epsilon))
    if d["last_step"] is not None:
        d["last_step"][:] = step_no
    # dense: the MLP's variables under hp, the wide bias under the wide rule
    idx = []
    for i in range(nl):
        idx += list(range(lo[2 * i], lo[2 * i] + wd[i] * wd[i + 1])) + list(range(lo[2 * i + 1], lo[2 * i + 1] + wd[i + 1]))
    if d["use_linear"]:
        gd[d["lin_bias_off"]] = dl.sum(dtype=F32)
    for sel, h, lrt, M, Vv in ((np.asarray(idx, np.int64), hp, lr_t, d["d_m"], d["d_v"]),
                               (np.asarray([d["lin_bias_off"]] if d["use_linear"] else [], np.int64), hpw, lr_tw, d["dw_m"],
                                d["dw_v"])):
        if not len(sel):
            continue
        w = dn[sel]
        m = M[sel] if M is not None else zero(w)
        v = Vv[sel] if Vv is not None else zero(w)
        w, m, v = rule(h, lrt, w, m, v, gd[sel], False)
        dn[sel] = w
        if M is not None:
            M[sel] = m
        if Vv is not None:
            Vv[sel] = v


class FusedRulesKernels(NumpyKernels):
    supports_fused_rules = True

    def mi_train_step_model(self, model, field_off, ids, labels, B, F, seed, step_no, logits, loss, sweep_blocks):
        assert 0 <= sweep_blocks <= 1024
        step(decode(model), field_off.numpy(), ids.numpy(), labels.numpy(), B, F, seed, step_no, model.hp.lr_t,
             model.hp_wide.lr_t if model.two_rules else model.hp.lr_t, logits.numpy(), loss.numpy())

    def mi_train_group_plan_models(self, members, M, B, F, field_off, table, nbytes, plan):
        if M < 1:
            raise _lib.MiError("mi_train_group_plan_models failed (-1): train_group_plan: %d members (at least 1)" % M)
        if M > _lib.FUSED_GROUP_MAX_MEMBERS:
            raise _lib.MiError("mi_train_group_plan_models failed (-2): train_group_plan: %d members (at most %d in one launch)"
                               % (M, _lib.FUSED_GROUP_MAX_MEMBERS))
        assert nbytes >= 64 * M and len(members) == M
        decoded, owned, max_step = [], {}, 2 ** 31 - 1
        for i in range(M):
            m = members[i]
            assert m.workspace and 0 < m.keep_prob <= 1
            d = decode(m)
            for name in ("lr_table", "lr_table_w"):
                if d["hp" if name == "lr_table" else "hpw"].kind == 0 and (name == "lr_table" or m.two_rules):
                    assert d[name] is not None and len(d[name]) >= 2, "a rule under Adam needs its schedule table"
                    max_step = min(max_step, len(d[name]) - 1)
            for p in (m.table, m.t_m, m.t_v, m.lin_w, m.l_m, m.l_v, m.last_step, m.dense, m.d_m, m.d_v, m.workspace) + (
                    (m.dw_m, m.dw_v) if m.two_rules else ()):
                if p and p in owned:
                    raise _lib.MiError("mi_train_group_plan_models failed (-1): train_group_plan: member %d and member %d share "
                                       "a state or workspace pointer" % (owned[p], i))
                if p:
                    owned[p] = i
            decoded.append(d)
        key = len(self.plans) + 1
        self.plans[key] = ("models", decoded, field_off, B, F)
        plan.device_table, plan.magic, plan.n_members, plan.B, plan.F = key, self.MAGIC, M, B, F
        plan.max_step = max_step

    def _models(self, plan):
        got = self.plans.get(plan.device_table)
        return got if (got is not None and got[0] == "models") else None

    @staticmethod
    def _lr(d, step_no):
        lr_t = float(d["lr_table"][step_no]) if d["lr_table"] is not None else 0.0
        lr_tw = float(d["lr_table_w"][step_no]) if d["lr_table_w"] is not None else (lr_t if d["hpw"] is d["hp"] else 0.0)
        return lr_t, lr_tw

    def mi_train_group_step(self, plan, M, ids, ids_stride, labels, labels_stride, B, step_no, logits, loss, sweep_blocks):
        got = self._models(plan)
        if got is None:
            return super().mi_train_group_step(plan, M, ids, ids_stride, labels, labels_stride, B, step_no, logits, loss,
                                               sweep_blocks)
        assert plan.magic == self.MAGIC and M == plan.n_members and B == plan.B and 1 <= step_no <= plan.max_step
        _, decoded, field_off, _, F = got
        assert ids_stride in (0, B * F) and labels_stride in (0, B) and tuple(logits.shape) == (M, B) and tuple(loss.shape) == (M,)
        for i, d in enumerate(decoded):
            lr_t, lr_tw = self._lr(d, step_no)
            step(d, field_off.numpy(), (ids[i] if ids_stride else ids).numpy(), (labels[i] if labels_stride else labels).numpy(),
                 B, F, (d["seed_base"] + step_no * 1000003) & MASK64, step_no, lr_t, lr_tw, logits[i].numpy(),
                 loss[i:i + 1].numpy())

    def mi_eval_group(self, plan, M, ids, labels, N, tail_scale, logits, batch_loss, hist, counts, partials, blocks):
        got = self._models(plan)
        if got is None:
            return super().mi_eval_group(plan, M, ids, labels, N, tail_scale, logits, batch_loss, hist, counts, partials, blocks)
        assert plan.magic == self.MAGIC and M == plan.n_members and N >= 1 and 0 <= blocks <= 1024
        _, decoded, field_off, B, F = got
        T = -(-N // B)
        assert tuple(ids.shape) == (N, F) and tuple(labels.shape) == (N,) and tuple(batch_loss.shape) == (M, T)
        assert not bool(hist.any()) and not bool(counts.any()), "the caller zeroes hist and counts"
        for i, d in enumerate(decoded):
            for t in range(T):
                lo, hi = t * B, min(N, (t + 1) * B)
                n = hi - lo
                rows = ids[lo:hi].numpy().astype(np.int64) + field_off.numpy()[None, :]
                y = labels[lo:hi].numpy()
                z, lb = forward(d, rows, y, n, F, 0, F32(1), F32(float(tail_scale[i])) if n < B else d["scale"], False)[:2]
                batch_loss[i, t] = float(lb)
                if logits is not None:
                    logits[i, lo:hi] = torch.from_numpy(z)
                h, cn, sm = counters(z, y)
                hist[i] += torch.from_numpy(h)
                counts[i] += torch.from_numpy(cn)
                partials[i, t] = torch.from_numpy(sm)


@pytest.fixture
def fused_rules_kernels(monkeypatch):
    """every engine the code under test builds gets the numpy stand-ins with the general one-launch step"""
    monkeypatch.setattr(engine, "HipKernels", FusedRulesKernels)
