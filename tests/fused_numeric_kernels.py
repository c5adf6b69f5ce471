"""numpy stand-ins for the one-launch step's numeric entries — mi_train_step_model_numeric, mi_train_group_plan_models_numeric,
mi_train_group_step_numeric, mi_eval_group_numeric, mi_train_step_fused_workspace_bytes_numeric (include/mi355x_rec.h) —
TEST INFRASTRUCTURE ONLY, not a test file.

FusedNumericKernels is tests/fused_rules_kernels.FusedRulesKernels plus those entries, so that the host code that reaches
them (engine.fused_train_step with x_num, FusedPopulation, model_fn with numeric_columns and fused_step="on", trainers.sweep)
runs without a GPU.  Restated from the header section "numeric columns in the one-launch step":

  forward   the concat is the F gathered rows, then the nd rows x[b, j] V[j, :]; sumv and the FM term over all F + nd rows;
            layer 1 over (F + nd) E inputs; lin[b] = the categorical wide sum, then + x[b, j] w_num[j], j ascending
  backward  g[b, j, :] = d_concat[b, F + j, :] + dlogit[b] (sumv[b, :] - x[b, j] V[j, :]);  dV[j, e] = sum_b x[b, j] g[b, j, e];
            dw_num[j] = sum_b dlogit[b] x[b, j];  b ascending, one rounding per operation
  apply     V under hp with d_m / d_v, w_num under the wide rule with dw_m / dw_v (d_m / d_v with one rule); everything
            else as fused_rules_kernels.step
  refused   nd outside [0, 16]; B (F + nd) E > 16384; nd > 0 without the FM term and the DNN; NULL x_num with nd > 0; a plan
            with numeric columns handed to mi_train_group_step / mi_eval_group
The update rules, the decoding of a mi_fused_model_t and the sweep are fused_rules_kernels' (rule, decode)."""
import numpy as np
import pytest
import torch

from mi355x_rec import _lib, engine
from tests.cpu_kernels import _ACT, counters
from tests.fused_rules_kernels import F32, FusedRulesKernels, decode, rule
from tests.util import MASK64, dropout_mask

MAX_NUMERIC, MAX_CONCAT = 16, 16384


def _refuse(entry, status, text):
    raise _lib.MiError("%s failed (%d): %s" % (entry, status, text))


def check_limits(entry, d, num, B, F, have_x):
    """the numeric limits of the header, in plan_model's order; num: (nd, num_emb_off, lin_num_off)"""
    nd = num[0]
    emb = d["use_fm"] or d["use_dnn"]
    E = d["E"] if emb else 4
    if not 0 <= nd <= MAX_NUMERIC:
        _refuse(entry, -2, "train_step_fused: %d numeric columns (0 to %d)" % (nd, MAX_NUMERIC))
    if B * (F + nd) * E > MAX_CONCAT:
        _refuse(entry, -2, "train_step_fused: B (F + n_numeric) E = %d (at most %d)" % (B * (F + nd) * E, MAX_CONCAT))
    if nd and not emb:
        _refuse(entry, -1, "train_step_fused: %d numeric columns without the FM term and the DNN" % nd)
    if nd and not (0 <= num[1] and num[1] + nd * E <= len(d["dense"])):
        _refuse(entry, -1, "train_step_fused: num_emb_off=%d" % num[1])
    if nd and d["use_linear"] and not (0 <= num[2] and num[2] + nd <= len(d["dense"])):
        _refuse(entry, -1, "train_step_fused: lin_num_off=%d" % num[2])
    if nd and not have_x:
        _refuse(entry, -1, "train_step_fused: x_num (the model has %d numeric columns)" % nd)


def forward(d, num, rows, x, labels, B, F, seed, keep, scale, train):
    """phases 0-2 with numeric columns: (logits z, loss, dl, the concat [B, F + nd, E], sumv, acts, Ws)"""
    E, nl, act, dn = d["E"], d["nl"], d["act"], d["dense"]
    nd, veo, lno = num
    emb = d["use_fm"] or d["use_dnn"]
    cat = None
    if emb:
        cat = d["table"][rows]                                              # [B, F, E]
        if nd:
            Vn = dn[veo:veo + nd * E].reshape(nd, E)
            cat = np.concatenate([cat, (x[:, :, None] * Vn[None, :, :]).astype(F32)], 1)
    z = np.zeros(B, F32)
    if d["use_linear"]:
        acc = np.zeros(B, F32)
        for f in range(F):
            if (d["wide"] >> f) & 1:
                acc = acc + d["lin_w"][rows[:, f]]
        for j in range(nd):
            acc = acc + x[:, j] * dn[lno + j]
        z = acc + dn[d["lin_bias_off"]]
    s = None
    if d["use_fm"]:
        s = np.zeros((B, E), F32)
        q = np.zeros((B, E), F32)
        for r in range(F + nd):                                             # rows in order, one rounding per operation
            s = s + cat[:, r]
            q = q + cat[:, r] * cat[:, r]
        t = s * s - q
        tot = np.zeros(B, F32)
        for c in range(E):
            tot = tot + t[:, c]
        z = z + F32(0.5) * tot
    acts, Ws = [], []
    lo, wd = d["layer_off"], d["widths"]
    if d["use_dnn"]:
        assert wd[0] == (F + nd) * E, "widths[0] is the concat's width"
        h = cat.reshape(B, (F + nd) * E)
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
    return z.astype(F32), loss, dl, cat, s, acts, Ws


def step(d, num, field_off, ids, x, labels, B, F, seed, step_no, lr_t, lr_tw, logits, loss):
    """one step of the model d with the numeric columns num: what train_fused_k does to its buffers"""
    assert 1 <= B <= 128 and 1 <= F <= 32 and d["R"] <= 1 << 18 and d["nl"] <= 4 and step_no >= 1
    E, nl, act, dn, keep = d["E"], d["nl"], d["act"], d["dense"], d["keep"]
    hp, hpw, R = d["hp"], d["hpw"], d["R"]
    nd, veo, lno = num
    emb = d["use_fm"] or d["use_dnn"]
    if d["last_step"] is not None:
        assert step_no == 1 or bool((d["last_step"] == step_no - 1).all()), "every row must be current"
    rows = ids.astype(np.int64) + field_off[None, :]
    z, ls, dl, cat, s, acts, Ws = forward(d, num, rows, x, labels, B, F, seed, keep, d["scale"], True)
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
                a = acts[i]                                            # the layer's stored output: act(pre) / keep, or 0
                if act == 1:
                    g = np.where(a > 0, g / keep, 0).astype(F32)
                else:
                    o = a * keep
                    der = {0: np.ones_like(o), 2: o * (1 - o), 3: 1 - o * o}[act]
                    g = np.where((keep < 1) & (a == 0), 0, (g / keep) * der).astype(F32)
                dy = g
            else:
                d_concat = g.reshape(B, F + nd, E)
    G = None
    if emb:
        G = np.zeros((B, F + nd, E), F32)
        if d_concat is not None:
            G = G + d_concat
        if d["use_fm"]:
            G = G + dl[:, None, None] * (s[:, None, :] - cat)
    # the numeric columns' gradients: b ascending
    if nd:
        gv = np.zeros((nd, E), F32)
        for b in range(B):
            gv = gv + x[b][:, None] * G[b, F:]
        gd[veo:veo + nd * E] = gv.reshape(-1)
        if d["use_linear"]:
            gw = np.zeros(nd, F32)
            for b in range(B):
                gw = gw + dl[b] * x[b]
            gd[lno:lno + nd] = gw
    # 4. apply, sparse: per field the distinct rows, entries in ascending order
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
    # the sweep: records under Adam, untouched rows (a numeric column owns no row)
    u = ~touched
    for on, h, lrt, W, M, Vv in ((emb and hp.kind == 0, hp, lr_t, d["table"], d["t_m"], d["t_v"]),
                                 (d["use_linear"] and hpw.kind == 0, hpw, lr_tw, d["lin_w"], d["l_m"], d["l_v"])):
        if on:
            M[u] = M[u] * F32(h.beta1)
            Vv[u] = Vv[u] * F32(h.beta2)
            W[u] = W[u] - (F32(lrt) * M[u]) / (np.sqrt(Vv[u]) + F32(h.epsilon))
    if d["last_step"] is not None:
        d["last_step"][:] = step_no
    # dense: the MLP and numeric_embeddings under hp; the wide bias and the numeric linear weights under the wide rule
    idx = []
    for i in range(nl):
        idx += list(range(lo[2 * i], lo[2 * i] + wd[i] * wd[i + 1])) + list(range(lo[2 * i + 1], lo[2 * i + 1] + wd[i + 1]))
    idx += list(range(veo, veo + nd * E)) if nd else []
    widx = []
    if d["use_linear"]:
        gd[d["lin_bias_off"]] = dl.sum(dtype=F32)
        widx = [d["lin_bias_off"]] + (list(range(lno, lno + nd)) if nd else [])
    for sel, h, lrt, M, Vv in ((np.asarray(idx, np.int64), hp, lr_t, d["d_m"], d["d_v"]),
                               (np.asarray(widx, np.int64), hpw, lr_tw, d["dw_m"], d["dw_v"])):
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


def _num(numeric):
    """a mi_fused_numeric_t (or None) as (nd, num_emb_off, lin_num_off)"""
    return (0, 0, 0) if numeric is None else (int(numeric.n_numeric), int(numeric.num_emb_off), int(numeric.lin_num_off))


class FusedNumericKernels(FusedRulesKernels):
    supports_fused_numeric = True
    NUMERIC_MAGIC = 0x6e75          # of a plan whose members have numeric columns

    def query(self, name, *args):
        if name == "mi_train_step_fused_workspace_bytes_numeric":
            B, F, nd, E, n_dense = args
            return 4 * (((n_dense + 3) & ~3) + ((B * (F + nd) * E + 3) & ~3))
        return super().query(name, *args)

    def mi_train_step_model_numeric(self, model, numeric, field_off, ids, x_num, labels, B, F, seed, step_no, logits, loss,
                                    sweep_blocks):
        assert 0 <= sweep_blocks <= 1024
        d, num = decode(model), _num(numeric)
        check_limits("mi_train_step_model_numeric", d, num, B, F, x_num is not None)
        step(d, num, field_off.numpy(), ids.numpy(), x_num.numpy() if num[0] else None, labels.numpy(), B, F, seed, step_no,
             model.hp.lr_t, model.hp_wide.lr_t if model.two_rules else model.hp.lr_t, logits.numpy(), loss.numpy())

    def mi_train_group_plan_models_numeric(self, members, numerics, M, B, F, field_off, table, nbytes, plan):
        nums = [_num(None if numerics is None else numerics[i]) for i in range(M)]
        for i in range(M):
            if nums[i][0] != nums[0][0]:
                _refuse("mi_train_group_plan_models_numeric", -1, "train_group_plan: member %d: train_step_fused: %d numeric "
                        "columns, member 0 has %d" % (i, nums[i][0], nums[0][0]))
            try:
                check_limits("mi_train_group_plan_models_numeric", decode(members[i]), nums[i], B, F, True)
            except _lib.MiError as e:
                raise _lib.MiError(str(e).replace("train_step_fused:", "train_group_plan: member %d: train_step_fused:" % i, 1))
        self.mi_train_group_plan_models(members, M, B, F, field_off, table, nbytes, plan)      # (the members' own checks, the plan)
        kind, decoded, field_off, B, F = self.plans[plan.device_table]
        self.plans[plan.device_table] = ("numeric" if nums[0][0] else kind, decoded, field_off, B, F, nums)
        if nums[0][0]:
            plan.magic = self.NUMERIC_MAGIC

    def _numeric(self, plan):
        got = self.plans.get(plan.device_table)
        return got if (got is not None and got[0] == "numeric") else None

    def mi_train_group_step(self, plan, M, ids, ids_stride, labels, labels_stride, B, step_no, logits, loss, sweep_blocks):
        if self._numeric(plan) is not None:
            _refuse("mi_train_group_step", -1, "train_group_step: the plan's members have %d numeric columns and this entry "
                    "brings no x_num" % self._numeric(plan)[5][0][0])
        return super().mi_train_group_step(plan, M, ids, ids_stride, labels, labels_stride, B, step_no, logits, loss, sweep_blocks)

    def mi_eval_group(self, plan, M, ids, labels, N, tail_scale, logits, batch_loss, hist, counts, partials, blocks):
        if self._numeric(plan) is not None:
            _refuse("mi_eval_group", -1, "eval_group: the plan's members have %d numeric columns and this entry brings no x_num"
                    % self._numeric(plan)[5][0][0])
        return super().mi_eval_group(plan, M, ids, labels, N, tail_scale, logits, batch_loss, hist, counts, partials, blocks)

    def mi_train_group_step_numeric(self, plan, M, ids, ids_stride, x_num, x_stride, labels, labels_stride, B, step_no, logits,
                                    loss, sweep_blocks):
        got = self._numeric(plan)
        if got is None:
            return super().mi_train_group_step(plan, M, ids, ids_stride, labels, labels_stride, B, step_no, logits, loss,
                                               sweep_blocks)
        assert plan.magic == self.NUMERIC_MAGIC and M == plan.n_members and B == plan.B and 1 <= step_no <= plan.max_step
        _, decoded, field_off, _, F, nums = got
        nd = nums[0][0]
        if x_num is None:
            _refuse("mi_train_group_step_numeric", -1, "train_group_step: x_num (the plan's members have %d numeric columns)" % nd)
        assert ids_stride in (0, B * F) and labels_stride in (0, B) and x_stride in (0, B * nd)
        assert tuple(logits.shape) == (M, B) and tuple(loss.shape) == (M,)
        for i, d in enumerate(decoded):
            lr_t, lr_tw = self._lr(d, step_no)
            step(d, nums[i], field_off.numpy(), (ids[i] if ids_stride else ids).numpy(), (x_num[i] if x_stride else x_num).numpy(),
                 (labels[i] if labels_stride else labels).numpy(), B, F, (d["seed_base"] + step_no * 1000003) & MASK64, step_no,
                 lr_t, lr_tw, logits[i].numpy(), loss[i:i + 1].numpy())

    def mi_eval_group_numeric(self, plan, M, ids, x_num, x_stride, labels, N, tail_scale, logits, batch_loss, hist, counts,
                              partials, blocks):
        got = self._numeric(plan)
        if got is None:
            return super().mi_eval_group(plan, M, ids, labels, N, tail_scale, logits, batch_loss, hist, counts, partials, blocks)
        assert plan.magic == self.NUMERIC_MAGIC and M == plan.n_members and N >= 1 and 0 <= blocks <= 1024
        _, decoded, field_off, B, F, nums = got
        nd = nums[0][0]
        if x_num is None:
            _refuse("mi_eval_group_numeric", -1, "eval_group: x_num (the plan's members have %d numeric columns)" % nd)
        T = -(-N // B)
        assert x_stride in (0, N * nd) and tuple(ids.shape) == (N, F) and tuple(labels.shape) == (N,)
        assert tuple(batch_loss.shape) == (M, T)
        assert not bool(hist.any()) and not bool(counts.any()), "the caller zeroes hist and counts"
        for i, d in enumerate(decoded):
            xs = (x_num[i] if x_stride else x_num).numpy()
            for t in range(T):
                lo, hi = t * B, min(N, (t + 1) * B)
                n = hi - lo
                rows = ids[lo:hi].numpy().astype(np.int64) + field_off.numpy()[None, :]
                y = labels[lo:hi].numpy()
                z, lb = forward(d, nums[i], rows, xs[lo:hi], y, n, F, 0, F32(1),
                                F32(float(tail_scale[i])) if n < B else d["scale"], False)[:2]
                batch_loss[i, t] = float(lb)
                if logits is not None:
                    logits[i, lo:hi] = torch.from_numpy(z)
                h, cn, sm = counters(z, y)
                hist[i] += torch.from_numpy(h)
                counts[i] += torch.from_numpy(cn)
                partials[i, t] = torch.from_numpy(sm)


@pytest.fixture
def fused_numeric_kernels(monkeypatch):
    """every engine the code under test builds gets the numpy stand-ins with the numeric entries"""
    monkeypatch.setattr(engine, "HipKernels", FusedNumericKernels)
