"""A population of small DeepFM models trained side by side: every member takes one training step in ONE launch
(mi_train_group_step, include/mi355x_rec.h), member i's result being bit for bit what its own
``engine.DeepFM.fused_train_step`` gives.  What the reference does for a grid of hyper-parameters, seeds or folds is M
runs of trainers/deep_fm.py:36-125 one after the other; a model of this size leaves the chip idle, so M of them fit at once.

The members are ordinary engines: after a population step each is exactly where its own fused step would have left it and
can be used alone (loss, predict_fused, top_k, state_dict, train_step, fused_train_step) — as long as all members are at
the same step again before the next population step."""
import numpy as np
import torch

from . import _lib
from .engine import DeepFM
from .metrics import metrics_from_counters


class FusedPopulation:
    MAX_MEMBERS = _lib.FUSED_GROUP_MAX_MEMBERS
    SWEEP_BLOCKS = 0     # workgroups of each member's all-rows sweep; 0: the library's choice (tests: results do not depend on it)
    EVAL_BLOCKS = 0      # workgroups per member of an evaluation (mi_eval_group's X); 0: the library's choice (the same holds)
    EVAL_BATCH = 32      # evaluate()'s tile size when neither the caller nor an earlier step names one

    def __init__(self, engines):
        engines = list(engines)
        if not engines:
            raise ValueError("FusedPopulation: no members")
        if len(engines) > self.MAX_MEMBERS:
            raise ValueError("FusedPopulation: %d members (at most %d in one launch)" % (len(engines), self.MAX_MEMBERS))
        seen = {}
        for i, e in enumerate(engines):
            if not isinstance(e, DeepFM):
                raise ValueError("FusedPopulation: member %d is %s, an engine.DeepFM is expected" % (i, type(e).__name__))
            if id(e) in seen:
                raise ValueError("FusedPopulation: member %d is the same engine as member %d" % (i, seen[id(e)]))
            seen[id(e)] = i
        first = engines[0]
        for i, e in enumerate(engines):
            why = e._fused_step_limit(1)
            if why is not None:
                raise ValueError("FusedPopulation: member %d: the model has %s; use train_step" % (i, why))
            if e.vocab_sizes != first.vocab_sizes:
                raise ValueError("FusedPopulation: member %d has other vocab_sizes than member 0 (%d fields against %d): the "
                                 "members share one set of feature columns" % (i, e.F, first.F))
            if e.n_numeric != first.n_numeric:
                raise ValueError("FusedPopulation: member %d has %d numeric columns, member 0 has %d: the members share one "
                                 "set of feature columns" % (i, e.n_numeric, first.n_numeric))
            if e.device != first.device:
                raise ValueError("FusedPopulation: member %d lives on %s, member 0 on %s" % (i, e.device, first.device))
        self.engines = engines
        self.M = len(engines)
        self.F = first.F
        self.nd = first.n_numeric      # numeric embedding columns: x_num float32 [.., nd] beside ids
        self.device = first.device
        self.k = first.k
        self._plans = {}           # B -> (B, struct, device table, the members' schedule generations, what the struct points to)
        self._last_b = None        # the batch size of the latest train_step
        self._eval_buf = {}        # (B, N, with logits) -> evaluate()'s output buffer and its views
        self.eval_out = None       # the latest evaluate()'s raw results on the host: hist, counts, partials, batch_loss
        self._out = {}             # B -> (loss [M], logits [M, B])
        self._table_len = 0        # the shortest schedule table of the members (steps below it need no look at the schedules)

    def __len__(self):
        return self.M

    # ------------------------------------------------------------------ the plan
    def rebuild(self):
        """Forget the plan: the next step makes a new one.  For a caller who REPLACED a member's tensors (load_state_dict
        copies into them in place and needs none)."""
        self._plans = {}

    def _describe(self, e, B, keep_alive):
        """engine e as a mi_fused_member_t for batches of B (keep_alive: the tensors the struct points to and e does not hold)"""
        layer_off, widths = e.layer_tables()
        ws = torch.empty(max(e.fused_workspace_bytes(B), 16), dtype=torch.uint8, device=e.device)
        if self.nd or not e._fused_step_plain():
            # any other optimizer, a linear_optimizer, field_dims / wide_fields, numeric columns: the general description
            m, held = e.fused_model(B, ws)
            keep_alive += list(held)
            for sched, tab, n in ((e.sched, "lr_table", "lr_table_len"),
                                  (e.lin_sched if m.two_rules else None, "lr_table_wide", "lr_table_wide_len")):
                if sched is not None:
                    keep_alive.append(sched.table)
                    _lib.set_ptrs(m, **{tab: sched.table})
                    setattr(m, n, int(sched.table.numel()))
            m.seed_base = (e.seed * 0x9E3779B97F4A7C15) & (2 ** 64 - 1)
            return m
        keep_alive += [layer_off, widths, ws, e.sched.table]
        m = _lib.FusedMember()
        _lib.set_ptrs(m, table=e.table, t_m=e.t_s0, t_v=e.t_s1, lin_w=e.lin_w, l_m=e.l_s0, l_v=e.l_s1, last_step=e.last_step,
                      dense=e.dense, d_m=e.d_s0, d_v=e.d_s1, layer_off=layer_off, widths=widths, lr_table=e.sched.table,
                      workspace=ws)
        m.table_stride, m.lin_stride, m.R, m.E, m.n_dense = e.ts, e.ls, e.R, e.E, e.P
        m.n_layers, m.activation = len(e.layers), e.act
        m.use_linear, m.use_fm, m.use_dnn = int(e.use_linear), int(e.use_mf), int(e.use_dnn)
        m.lin_bias_off = e.lin_bias_off
        m.keep_prob = float(1.0 - e.dropout if e.dropout > 0 else 1.0)
        m.scale = float(np.float32(1.0 / B)) if e.reduction == "mean" else 1.0
        m.hp = e.opt.hparams(0.0)
        m.lr_table_len = int(e.sched.table.numel())
        m.seed_base = (e.seed * 0x9E3779B97F4A7C15) & (2 ** 64 - 1)           # engine._layer_seed(0) without its step term
        m.workspace_bytes = ws.numel()
        return m

    @staticmethod
    def _scheds(e):
        """the Adam schedules member e steps by (none under the other optimizers; two with two different Adams)"""
        out = [s for s in (e.sched, e.lin_sched) if s is not None]
        return out[:1] if len(out) == 2 and out[0] is out[1] else out

    def _gens(self):
        return [[s.gen for s in self._scheds(e)] for e in self.engines]

    def _build(self, B):
        keep_alive = []
        nbytes = int(self.k.query("mi_train_group_plan_bytes", self.M))
        table = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=self.device)
        plan = _lib.FusedGroupPlan()
        if self.nd:
            members = (_lib.FusedModel * self.M)(*[self._describe(e, B, keep_alive) for e in self.engines])
            numerics = (_lib.FusedNumeric * self.M)(*[e.fused_numeric() for e in self.engines])
            self.k.mi_train_group_plan_models_numeric(members, numerics, self.M, B, self.F, self.engines[0].field_off, table,
                                                      table.numel(), plan)
        elif all(e._fused_step_plain() for e in self.engines):
            members = (_lib.FusedMember * self.M)(*[self._describe(e, B, keep_alive) for e in self.engines])
            self.k.mi_train_group_plan(members, self.M, B, self.F, self.engines[0].field_off, table, table.numel(), plan)
        else:
            # (a member of mi_train_step_fused's own scope among them: the same description with one rule and every field wide)
            descs = []
            for e in self.engines:
                d = self._describe(e, B, keep_alive)
                if isinstance(d, _lib.FusedMember):
                    g = _lib.FusedModel()
                    for name, _ in _lib.FusedMember._fields_:
                        setattr(g, name, getattr(d, name))
                    g.wide_fields = (1 << e.F) - 1
                    d = g
                descs.append(d)
            members = (_lib.FusedModel * self.M)(*descs)
            self.k.mi_train_group_plan_models(members, self.M, B, self.F, self.engines[0].field_off, table, table.numel(), plan)
        self._plans[B] = (B, plan, table, self._gens(), keep_alive)
        return self._plans[B]

    def _check_limits(self, B):
        for i, e in enumerate(self.engines):
            why = e._fused_step_limit(B)
            if why is not None:
                raise ValueError("FusedPopulation: member %d: the model has %s; use train_step" % (i, why))

    def _plan_for(self, B):
        """The plan for batches (tiles) of B examples: the one in hand while no member's schedule table has moved, else a new
        one.  Plans are kept per batch size, so training and evaluating at two sizes alternate without a rebuild."""
        plan = self._plans.get(B)
        if plan is None:
            self._check_limits(B)
        if plan is None or self._gens() != plan[3]:
            plan = self._build(B)
        return plan

    # ------------------------------------------------------------------ the step
    def _check_x(self, x_num, n, lead):
        """x_num float32 [n, nd], or [M, n, nd] where `lead` allows one set per member; None exactly without numeric columns"""
        M, nd = self.M, self.nd
        if not nd:
            if x_num is not None:
                raise ValueError("FusedPopulation: the members have no numeric columns")
            return
        shapes = ((n, nd), (M, n, nd)) if lead else ((n, nd),)
        if not isinstance(x_num, torch.Tensor) or x_num.dtype != torch.float32 or not x_num.is_contiguous() \
                or tuple(x_num.shape) not in shapes:
            raise ValueError("FusedPopulation: x_num must be a contiguous float32 %s tensor" % " or ".join(
                str(list(s)) for s in shapes))
        if x_num.device.type != self.device.type:
            raise ValueError("FusedPopulation: x_num must live on %s" % self.device)

    def _check_batch(self, ids, labels):
        M, F = self.M, self.F
        if not isinstance(ids, torch.Tensor) or ids.dtype != torch.int32 or not ids.is_contiguous() or ids.dim() not in (2, 3) \
                or ids.shape[-1] != F or (ids.dim() == 3 and ids.shape[0] != M):
            raise ValueError("FusedPopulation: ids must be a contiguous int32 [B, %d] or [%d, B, %d] tensor" % (F, M, F))
        B = int(ids.shape[-2])
        if not isinstance(labels, torch.Tensor) or labels.dtype != torch.uint8 or not labels.is_contiguous() \
                or tuple(labels.shape) not in ((B,), (M, B)):
            raise ValueError("FusedPopulation: labels must be a contiguous uint8 [B] or [%d, B] tensor (B = %d)" % (M, B))
        if ids.device.type != self.device.type or labels.device.type != self.device.type:
            raise ValueError("FusedPopulation: ids and labels must live on %s" % self.device)
        return B

    def train_step(self, ids, labels, out=None, x_num=None):
        """One optimizer.minimize(loss) of EVERY member as one launch: returns (loss [M], logits [M, B]) device tensors,
        no host sync.  ids int32 [B, F] (one batch for all members) or [M, B, F] (one per member); labels uint8 [B] or
        [M, B]; x_num float32 [B, nd] or [M, B, nd] with numeric columns (None without).  out = (loss, logits): write there
        instead of into the population's own buffers."""
        B = self._check_batch(ids, labels)
        self._check_x(x_num, B, True)
        engines = self.engines
        step = engines[0].step + 1
        for i, e in enumerate(engines):
            if e.step + 1 != step:
                raise ValueError("FusedPopulation: member %d is at step %d, member 0 at step %d: the members of a population "
                                 "step together (bring the others up with their own fused_train_step)" % (i, e.step, step - 1))
        if B not in self._plans:
            self._check_limits(B)                     # (a batch outside the kernel's scope: refused before anything is touched)
        if step >= self._table_len or any(e._final_step != e.step for e in engines):
            for e in engines:
                e.finalize_rows()                     # (a no-op after a fused step)
                for s in self._scheds(e):
                    s.lr_t(step)                      # (extends the member's table when the run outgrows it: gen changes)
            self._table_len = min([len(s.host) for e in engines for s in self._scheds(e)] or [1 << 62])
        plan = self._plan_for(B)
        self._last_b = B
        if out is None:
            out = self._out.get(B)
            if out is None:
                out = self._out[B] = (torch.empty(self.M, dtype=torch.float32, device=self.device),
                                      torch.empty(self.M, B, dtype=torch.float32, device=self.device))
        loss, logits = out
        if tuple(loss.shape) != (self.M,) or tuple(logits.shape) != (self.M, B) or loss.dtype != torch.float32 \
                or logits.dtype != torch.float32 or not loss.is_contiguous() or not logits.is_contiguous():
            raise ValueError("FusedPopulation: out = (loss float32 [%d], logits float32 [%d, %d]), contiguous" % (self.M, self.M, B))
        if self.nd:
            self.k.mi_train_group_step_numeric(plan[1], self.M, ids, B * self.F if ids.dim() == 3 else 0, x_num,
                                               B * self.nd if x_num.dim() == 3 else 0, labels, B if labels.dim() == 2 else 0, B,
                                               step, logits, loss, int(self.SWEEP_BLOCKS))
        else:
            self.k.mi_train_group_step(plan[1], self.M, ids, B * self.F if ids.dim() == 3 else 0, labels,
                                       B if labels.dim() == 2 else 0, B, step, logits, loss, int(self.SWEEP_BLOCKS))
        for e in engines:
            e.step = step
            e._final_step = step
        return loss, logits

    # ------------------------------------------------------------------ evaluation
    def evaluate(self, ids, labels, batch_size=None, return_logits=False, exact=None, x_num=None):
        """Every member's EVAL metrics over a whole evaluation set as ONE launch (mi_eval_group) and one device-to-host copy:
        a list of M dicts with the keys of metrics.metrics_from_counters plus "loss", the fp64 mean over the fp32 losses of
        the batches of batch_size examples (tf.metrics.mean over batch losses; the last batch may be short and is reduced
        with its own 1 / n) — what Estimator.evaluate reports for the member on these batches.  ids int32 [N, F], labels uint8
        [N], x_num float32 [N, nd] with numeric columns, on the population's device, one set for all members.  batch_size None: that of the latest train_step, else
        EVAL_BATCH.  No dropout; no member's variables, slots, step or schedule change.  return_logits: (metrics, logits
        [M, N] device tensor).  exact: an exact_auc.ExactAuc of these labels (and, for GAUC, the examples' groups): the
        logits of this evaluation are kept and every member's dict gains auc_exact, auc_exact_pairs and, with groups, gauc,
        gauc_groups — one more launch per layout for all members (ExactAuc.metrics).  None: none of that."""
        M, F = self.M, self.F
        if not isinstance(ids, torch.Tensor) or ids.dtype != torch.int32 or not ids.is_contiguous() or ids.dim() != 2 \
                or ids.shape[1] != F:
            raise ValueError("FusedPopulation: ids must be a contiguous int32 [N, %d] tensor" % F)
        N = int(ids.shape[0])
        if N < 1:
            raise ValueError("FusedPopulation: no examples to evaluate")
        if not isinstance(labels, torch.Tensor) or labels.dtype != torch.uint8 or not labels.is_contiguous() \
                or tuple(labels.shape) != (N,):
            raise ValueError("FusedPopulation: labels must be a contiguous uint8 [N] tensor (N = %d)" % N)
        if ids.device.type != self.device.type or labels.device.type != self.device.type:
            raise ValueError("FusedPopulation: ids and labels must live on %s" % self.device)
        self._check_x(x_num, N, False)
        if exact is not None and (exact.N != N or exact.device.type != self.device.type):
            raise ValueError("FusedPopulation: exact was built for %d examples on %s, the evaluation has %d on %s" % (
                exact.N, exact.device, N, self.device))
        B = int(batch_size) if batch_size is not None else (self._last_b or self.EVAL_BATCH)
        if B < 1:
            raise ValueError("FusedPopulation: batch_size=%d (at least 1)" % B)
        for e in self.engines:
            e.finalize_rows()                         # (a no-op after a fused step)
        plan = self._plan_for(B)
        T, n_tail = -(-N // B), N % B
        with_logits = bool(return_logits) or exact is not None
        key = (B, N, with_logits)
        buf = self._eval_buf.get(key)
        if buf is None:
            # one allocation, so that one copy brings everything home: [hist | counts] int64, partials f64, batch losses f32
            n_int, n_par, n_loss = M * (2 * 201 + 8), M * T * 3, M * T
            raw = torch.empty(8 * (n_int + n_par) + 4 * n_loss, dtype=torch.uint8, device=self.device)
            ints = raw[:8 * n_int].view(torch.int64)
            tail = torch.tensor([float(np.float32(1.0 / n_tail)) if (n_tail and e.reduction == "mean") else 1.0
                                 for e in self.engines], dtype=torch.float32).to(self.device)
            buf = self._eval_buf[key] = dict(
                raw=raw, ints=ints, hist=ints[:M * 402].view(M, 2, 201), counts=ints[M * 402:].view(M, 8),
                partials=raw[8 * n_int:8 * (n_int + n_par)].view(torch.float64).view(M, T, 3),
                loss=raw[8 * (n_int + n_par):].view(torch.float32).view(M, T), tail=tail,
                logits=torch.empty(M, N, dtype=torch.float32, device=self.device) if with_logits else None)
            if len(self._eval_buf) > 4:
                self._eval_buf.pop(next(iter(self._eval_buf)))
        buf["ints"].zero_()
        if self.nd:
            self.k.mi_eval_group_numeric(plan[1], M, ids, x_num, 0, labels, N, buf["tail"], buf["logits"], buf["loss"],
                                         buf["hist"], buf["counts"], buf["partials"], int(self.EVAL_BLOCKS))
        else:
            self.k.mi_eval_group(plan[1], M, ids, labels, N, buf["tail"], buf["logits"], buf["loss"], buf["hist"], buf["counts"],
                                 buf["partials"], int(self.EVAL_BLOCKS))
        extra = exact.metrics(buf["logits"]) if exact is not None else None     # (the pair counts of these logits, and their own copy)
        host = buf["raw"].cpu().numpy()
        n_int, n_par = M * 410, M * T * 3
        ints = host[:8 * n_int].view(np.int64)
        hist, counts = ints[:M * 402].reshape(M, 2, 201), ints[M * 402:].reshape(M, 8)
        partials = host[8 * n_int:8 * (n_int + n_par)].view(np.float64).reshape(M, T, 3)
        losses = host[8 * (n_int + n_par):].view(np.float32).reshape(M, T)
        sums = np.cumsum(partials, axis=1)[:, -1, :]          # (the tiles in ascending order, one addition after the other)
        self.eval_out = dict(hist=hist, counts=counts, partials=partials, batch_loss=losses)     # (the latest evaluation, raw)
        out = []
        for i in range(M):
            m = metrics_from_counters(hist[i], counts[i], sums[i])
            m["loss"] = float(np.cumsum(losses[i].astype(np.float64))[-1] / T)
            if extra is not None:
                m.update(extra[i])
            out.append(m)
        return (out, buf["logits"]) if return_logits else out

    # ------------------------------------------------------------------ ranking
    def rank_targets(self, plan, query_features, candidate_features, targets, exclude=None, say=None):
        """Every member's exact ranks of named target candidates (Estimator.rank_targets for all members at once): numpy
        int32 [M, U, Tmax], -1 where a target has no rank.  plan: the members' FieldPlan (they share one set of feature
        columns).  Every row is made current first (finalize_rows: a no-op after a fused step); the members inside
        mi_pair_target_ranks' scope are ranked in ONE launch, the others one by one (say(text) is told which)."""
        from .model import rank_targets_sides
        return rank_targets_sides(plan, self.engines, query_features, candidate_features, targets, exclude, say)
