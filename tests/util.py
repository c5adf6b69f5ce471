"""Shared helpers for the parity tests (oracle side = checker, HIP side = thing under test).  Case lists and the helpers
that build engines and populations are in tests/cases.py, the numpy stand-ins for the library in tests/cpu_kernels.py; no
test module imports another.  pytest does not rewrite the assertions of this module: every assert here carries its message."""
import csv
import json
import os
import re
import subprocess
import sys

import numpy as np
import torch

from oracle import deepfm as O
from oracle import optimizers as OO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "recommender-tensorflow_amd")
MASK64 = (1 << 64) - 1


def _mix32(x):
    x = x ^ (x >> np.uint32(16)); x = x * np.uint32(0x7feb352d)
    x = x ^ (x >> np.uint32(15)); x = x * np.uint32(0x846ca68b)
    return x ^ (x >> np.uint32(16))


def dropout_mask(seed, M, N, keep):
    """Host replica of the kernels' counter-based dropout mask (csrc/common.h, mi_drop_*): keep flag {0, 1} per element
    (kept values are divided by keep, as tf.nn.dropout does).  Two decisions per 32-bit hash: element (row, col) is kept
    iff its 16 bits of hash(row, col >> 1) — low half for an even column, high half for an odd one — are below keep * 2^16."""
    u = np.uint32
    row = np.arange(M, dtype=np.uint32)[:, None]
    col = np.arange(N, dtype=np.uint32)[None, :]
    with np.errstate(over="ignore"):
        s = u(seed & 0xFFFFFFFF) ^ (u((seed >> 32) & 0xFFFFFFFF) * u(0xC2B2AE35))
        rowkey = _mix32((row * u(0x9E3779B1)) ^ s)
        x = rowkey + (col >> u(1)) * u(0x85EBCA77)
        x = ~x + (x << u(15))
        x = x ^ (x >> u(12))
        x = x + (x << u(2))
        x = x ^ (x >> u(4))
        x = x + (x << u(3))
        x = x ^ (x >> u(11))
        x = x + (x << u(11))
        x = x ^ (x >> u(16))
    bits = np.where((col & u(1)) == 1, x >> u(16), x & u(0xFFFF))
    thresh = u(np.float32(keep) * np.float32(65536.0))
    return (bits < thresh).astype(np.float32)


def make_problem(seed, vocab, E, hidden, B, n_numeric=0, lin_scale=0.05, dup=True, use_dnn=True):
    rng = np.random.default_rng(seed)
    p = O.init_params(rng, vocab, E, hidden, n_numeric=n_numeric, dtype=np.float32, lin_scale=lin_scale,
                      use_dnn=use_dnn)
    p.lin_bias[:] = 0.1
    for k, b in p.mlp:
        b[:] = (rng.standard_normal(b.shape) * 0.05).astype(np.float32)
    ids = np.stack([rng.integers(0, v, B) for v in vocab], 1).astype(np.int32)
    if dup and B > 3:
        ids[B // 2] = ids[0]          # duplicate rows inside one batch
        ids[B - 1, 0] = ids[1, 0]
    x = rng.standard_normal((B, n_numeric)).astype(np.float32) if n_numeric else None
    y = (rng.random(B) < 0.3).astype(np.uint8)
    return p, ids, x, y


def dev(a, device="cuda"):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(device)


def rel_err(a, b):
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    return float(np.max(np.abs(a - b) / (np.abs(b) + 1e-30))) if a.size else 0.0


def max_err_scaled(a, b):
    """max |a-b| / max(|b|, rms(b)): a relative error that does not blow up on entries near 0."""
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    if a.size == 0:
        return 0.0
    floor = np.sqrt(np.mean(b * b)) + 1e-30
    return float(np.max(np.abs(a - b) / np.maximum(np.abs(b), floor)))


# ---- outputs and workspaces that show a write outside what a kernel entry was given (GPU tests) ------------------------------
GUARD = 64             # floats of NaN before and after every output (256 bytes: the output keeps its 16-byte alignment)
WS_FILL = 0xA5


def guarded_nan(*shape):
    """(whole buffer, view of `shape` inside it): an output pre-filled with NaN between two NaN guard bands"""
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * GUARD,), float("nan"), device="cuda")
    return buf, buf[GUARD:GUARD + n].view(*shape)


def guards_intact(buf):
    return bool(torch.isnan(buf[:GUARD]).all()) and bool(torch.isnan(buf[-GUARD:]).all())


def exact_workspace(nbytes, offset=32):
    """(whole buffer, view of EXACTLY nbytes inside it at a 32-byte-aligned — not 64- or 256-aligned — offset); the
    buffer is filled with a byte pattern that must survive before and after the view"""
    buf = torch.full((int(nbytes) + 512,), WS_FILL, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 256 == 0
    ws = buf[offset:offset + int(nbytes)]
    assert ws.data_ptr() % 256 == offset
    return buf, ws


def workspace_surroundings_intact(buf, ws):
    lo = ws.data_ptr() - buf.data_ptr()
    return bool((buf[:lo] == WS_FILL).all()) and bool((buf[lo + ws.numel():] == WS_FILL).all())


# ---- raw calls through the C ABI --------------------------------------------------------------------------------------------
def _st():
    from mi355x_rec import _lib
    return _lib.cur_stream()


def _chk(rc, what="call"):
    from mi355x_rec import _lib
    _lib.check(rc, what)


def _p(t):
    return None if t is None else t.data_ptr()


def _header_decls():
    """{entry name: number of arguments} of every mi_* declaration in include/mi355x_rec.h"""
    src = open(os.path.join(ROOT, "include", "mi355x_rec.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    decls = {}
    for m in re.finditer(r"\b(mi_\w+)\s*\(([^;{}]*?)\)\s*;", src, flags=re.S):
        args = m.group(2).strip()
        decls[m.group(1)] = 0 if args in ("", "void") else args.count(",") + 1
    return decls


# ---- inputs, and an engine's variables against the oracle's --------------------------------------------------------------------
def _t(a):
    """a host array as a CPU tensor (dev() is the same for the GPU)"""
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a))


def _fresh_ids(rng, vocab, B):
    ids = np.stack([rng.integers(0, v, B) for v in vocab], 1).astype(np.int32)
    if B > 1:
        ids[B // 2] = ids[0]
    return ids


def _check_vars(m, p, atol):
    """the numpy stand-ins' engines: every model they train has a table and a wide part"""
    g = m.export_numpy()
    for f in range(len(p.emb)):
        assert np.max(np.abs(g["emb"][f] - p.emb[f])) < atol, ("emb", f)
        assert np.max(np.abs(g["lin_w"][f] - p.lin_w[f])) < atol, ("lin_w", f)
    for i, (k, b) in enumerate(g["mlp"]):
        assert np.max(np.abs(k - p.mlp[i][0])) < atol and np.max(np.abs(b - p.mlp[i][1])) < atol, ("mlp", i)
    assert abs(g["lin_bias"][0] - p.lin_bias[0]) < atol, ("lin_bias", float(g["lin_bias"][0]), float(p.lin_bias[0]))


def _compare_vars(m, p, atol):
    """the HIP engines: a model may lack the table or the wide part, and may have numeric columns"""
    g = m.export_numpy()
    for f in range(len(p.emb)):
        if g["emb"] is not None:
            assert np.max(np.abs(g["emb"][f] - p.emb[f])) < atol, ("emb", f, float(np.max(np.abs(g["emb"][f] - p.emb[f]))))
        if g["lin_w"] is not None:
            assert np.max(np.abs(g["lin_w"][f] - p.lin_w[f])) < atol, ("lin_w", f)
    for i, (k, b) in enumerate(g["mlp"]):
        assert np.max(np.abs(k - p.mlp[i][0])) < atol, ("kernel", i, float(np.max(np.abs(k - p.mlp[i][0]))))
        assert np.max(np.abs(b - p.mlp[i][1])) < atol, ("bias", i)
    assert abs(g["lin_bias"][0] - p.lin_bias[0]) < atol, ("lin_bias", float(g["lin_bias"][0]), float(p.lin_bias[0]))
    if "num_emb" in g:
        assert np.max(np.abs(g["num_emb"] - p.num_emb)) < atol, ("num_emb", float(np.max(np.abs(g["num_emb"] - p.num_emb))))
        assert np.max(np.abs(g["lin_num"] - p.lin_num)) < atol, ("lin_num", float(np.max(np.abs(g["lin_num"] - p.lin_num))))


def _device_relu_masks(m, B):
    """Which hidden units the device's last train step let through (activation > 0), per hidden layer: read from the
    stored activations — fp32, or the planes where a layer's output exists as planes only."""
    out = []
    for i, h in enumerate(m.hidden):
        if i in m._acts_in_planes:
            a = torch.empty(B, h, device="cuda")
            m.k.mi_merge_rows(m._pl["x%dp" % (i + 1)].struct, B, h, a, h)
        else:
            a = m._ws["act%d" % i][:B * h].view(B, h)
        out.append((a > 0).cpu().numpy())
    return out


# ---- the planes GEMMs -------------------------------------------------------------------------------------------------------
def row_rel_err(got, ref):
    """max over rows of max|got - ref| / rms(ref row)  (rows that are exactly zero must match exactly)"""
    got = np.asarray(got, np.float64); ref = np.asarray(ref, np.float64)
    rms = np.sqrt(np.mean(ref * ref, 1))
    err = np.abs(got - ref).max(1)
    z = rms == 0
    assert np.all(err[z] == 0), ("rows that are zero in the reference", np.flatnonzero(z & (err != 0))[:8].tolist())
    return float((err[~z] / rms[~z]).max()) if (~z).any() else 0.0


def planned_splits(M, N, K):
    """Split-K slabs of mi_dense_bwd_weight_planes for one job, restated from the library's two launch plans — wgrad_pl.hip's
    wgrad_pl_plan (LDS-DMA kernel: N = 128 / 256 / 512; at least 32 k-steps of 16 examples per split, one round of
    workgroups) and gemm.hip's wgrad_splits (register-staged kernel, every other whole-tile shape; at least four k-tiles
    of 32 examples per split, about two rounds).  One split: the job is `direct` (the GEMM writes dW itself, no fold)."""
    cdiv = lambda a, b: -(-a // b)
    if N in (128, 256, 512) and K % 128 == 0 and M % 16 == 0:
        tiles_k = cdiv(K, 128)
        target = (512 if N == 128 else 256) // tiles_k
        target = max(1, min(target, max(M // 512, 1)))
        k_per_split = cdiv(cdiv(M, target), 16) * 16
        return cdiv(M, k_per_split)
    return max(1, min(1024 // (cdiv(K, 128) * cdiv(N, 128)), cdiv(M, 128), 256))


# ---- top-K ------------------------------------------------------------------------------------------------------------------
def host_topk(scores, k, excl_rows):
    """The header's rule (include/mi355x_rec.h): score descending, equal scores by ascending index, NaN below every number,
    excluded candidates removed, index -1 / score -inf past the eligible ones; a -0 score comes back as +0"""
    U, I = scores.shape
    out_s = np.full((U, k), -np.inf, np.float32)
    out_i = np.full((U, k), -1, np.int32)
    for u in range(U):
        ok = np.setdiff1d(np.arange(I), np.asarray(sorted(excl_rows[u]), np.int64))
        s = scores[u, ok]
        order = np.lexsort((ok, np.where(np.isnan(s), np.inf, -s)))[:k]
        out_s[u, :len(order)] = s[order] + np.float32(0.0)
        out_i[u, :len(order)] = ok[order]
    return out_s, out_i


# ---- the CLIs: data, exports, sweeps ------------------------------------------------------------------------------------------
def _write_csv(path, n, seed):
    """n MovieLens-shaped rows with a learnable rule, in trainers.ml_100k's columns"""
    from trainers import ml_100k
    rng = np.random.default_rng(seed)
    occ = ["technician", "administrator", "student", "homemaker", "none", "engineer"]
    with open(path, "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(ml_100k.COLUMNS)
        for _ in range(n):
            row = {c: (0 if d[0] == 0 else "null") for c, d in zip(ml_100k.COLUMNS, ml_100k.DEFAULTS)}
            uid, iid = int(rng.integers(1, 944)), int(rng.integers(1, 1683))
            g = rng.integers(0, 2, len(ml_100k.GENRE))
            # a learnable rule so that training visibly reduces the loss
            like = (g[1] == 1) if rng.random() < 0.9 else (g[1] == 0)
            row.update(user_id=uid, item_id=iid, rating=5 if like else int(rng.integers(1, 5)),
                       age=int(rng.integers(7, 74)), gender=str(rng.choice(["F", "M", ""])),
                       occupation=str(rng.choice(occ)), zipcode="%05d" % rng.integers(0, 99999),
                       release_year=int(rng.integers(1922, 1999)))
            row.update({k: int(v) for k, v in zip(ml_100k.GENRE, g)})
            w.writerow([row[c] for c in ml_100k.COLUMNS])


def _requests(n=30, seed=2):
    """the serving receivers' columns of n synthetic rows"""
    from trainers import ml_100k
    cols, _ = ml_100k._read_csv("synthetic:%d:%d" % (n, seed))
    recv = set(ml_100k.serving_input_fn().receiver_tensors)
    return {k: v for k, v in cols.items() if k in recv}


def _train_deep_fm_export(root, name, extra):
    """ten steps of trainers.deep_fm on the CPU in <root>/<name>: the directory of its exports"""
    from trainers import _cli, recommend
    trainer, opt = recommend.MODELS["deep_fm"]
    job = os.path.join(root, name)
    argv = ["--synthetic", "300", "--job-dir", job, "--train-steps", "10", "--batch-size", "16", "--device", "cpu"] + list(extra)
    trainer.train_and_evaluate(_cli.make_parser("deep_fm", opt).parse_args(argv))
    return os.path.join(job, "export", "exporter")


def _fake_sweep(root, exports, order=(1, 0)):
    """a sweep directory whose sweep.json lists the two exports as members `order`, best first"""
    job = os.path.join(root, "sweep")
    os.makedirs(job, exist_ok=True)
    rows = [{"member": m, "dir": os.path.dirname(os.path.dirname(exports[m])), "export": exports[m], "metrics": {"auc": 0.9 - 0.1 * r}}
            for r, m in enumerate(order)]
    with open(os.path.join(job, "sweep.json"), "w") as f:
        json.dump({"select": "auc", "members": rows}, f)
    return job


def _run_module(mod, args):
    """python -m <mod> <args> in a fresh process, from the package directory; it must succeed"""
    env = dict(os.environ)
    env["PYTHONPATH"] = os.pathsep.join([PKG, ROOT])
    r = subprocess.run([sys.executable, "-m", mod] + args, cwd=PKG, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout + r.stderr
    return r


# ---- the lazy Adam catch-up against the literal sweep ----------------------------------------------------------------------------
def adam_lr_table(lr, beta1, beta2, n):
    """lr_t of steps 0 .. n (index 0 unused) of TF's schedule lr sqrt(1 - beta2^t) / (1 - beta1^t) for the fp32 betas, as
    float32: an INPUT of mi_sparse_catchup (the tests of the replay do not depend on how it was rounded)"""
    t = np.arange(n + 1)
    b1, b2 = float(np.float32(beta1)), float(np.float32(beta2))
    return (lr * np.sqrt(1 - b2 ** t) / np.maximum(1 - b1 ** t, 1e-30)).astype(np.float32)


def catchup_sweep(w, m, v, last, step_to, lr, beta1, beta2, eps):
    """TF Adam's whole-table sweep over the steps a row sat out, in numpy fp32 (IEEE sqrt and divide, one rounding per
    operation, denormals kept): for s in (last[r], step_to]: m *= b1; v *= b2; w -= (lr[s] m) / (sqrt(v) + eps), for the
    rows with 0 < last[r] < step_to — one pass over the steps with a mask s > last[r], every row at once.  w, m, v: [R] or
    [R, E].  Returns (w, m, v, sum_j |t_j| in fp64); the inputs are not written."""
    f = np.float32
    b1, b2, eps = f(beta1), f(beta2), f(eps)
    ew, em, ev = w.copy(), m.copy(), v.copy()
    moved = np.zeros(w.shape, np.float64)
    col = last.reshape((-1,) + (1,) * (w.ndim - 1))
    live = col > 0
    if not (live & (col < step_to)).any():
        return ew, em, ev, moved
    with np.errstate(all="ignore"):
        for s in range(int(last[(last > 0) & (last < step_to)].min()) + 1, step_to + 1):
            on = live & (s > col)
            mm, vv = em * b1, ev * b2
            t = (lr[s] * mm) / (np.sqrt(vv) + eps)
            em, ev, ew = np.where(on, mm, em), np.where(on, vv, ev), np.where(on, ew - t, ew)
            moved += np.where(on, np.abs(t), 0.0)
    assert ew.dtype == em.dtype == ev.dtype == np.float32, "the sweep left fp32"
    return ew, em, ev, moved


def bounded_catchup_error(got, exp, moved, what, check=True):
    """MI_CATCHUP_BOUNDED's contract (include/mi355x_rec.h) for every variable: |w - w_sweep| <= 3 ulp(w) + 2e-6 sum_j |t_j|.
    Prints and returns (worst |err| / bound, share bit-identical, share within 1e-7 relative); asserts the bound unless
    check is False (a tool that only measures)."""
    d = np.abs(got.astype(np.float64) - exp.astype(np.float64))
    bound = 3 * np.spacing(np.abs(exp)).astype(np.float64) + 2e-6 * moved
    worst = float((d / bound).max())
    same = float((got.view(np.uint32) == exp.view(np.uint32)).mean())
    within = float((d <= 1e-7 * np.abs(exp)).mean())
    print("bounded catch-up, %s: worst |err| / (3 ulp + 2e-6 sum|t|) = %.3f, bit-identical %.4f, within 1e-7 relative %.4f, "
          "max relative error %.3g" % (what, worst, same, within, float((d / np.maximum(np.abs(exp), 1e-30)).max())))
    assert not check or worst <= 1.0, (what, worst)
    return worst, same, within
