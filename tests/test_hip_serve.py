"""GPU: serving — mi_predict_fused (csrc/serve.hip) through DeepFM.predict_fused, the bound entry and the
`python -m trainers.predict` CLI.

Fused logits against the fp64 oracle on identical weights (the project's logit contract: max_err_scaled < 1e-5), the
head's outputs bit for bit against mi_binary_predictions, the engine's own forward after lazily-updated Adam steps,
determinism and independence of a request from its neighbours, the entry's limits, and the CLI end to end."""
import csv

import numpy as np
import pytest
import torch

from mi355x_rec import _lib
from mi355x_rec.engine import DeepFM, HipKernels, OptimizerSpec
from oracle import deepfm as O
from tests.cases import RANK_CASES, VOCAB26
from tests.util import _run_module, dev, make_problem, max_err_scaled

pytestmark = pytest.mark.gpu

BATCHES = (1, 31, 32, 33, 257, 4096)
# the model cases of tests.cases.RANK_CASES (E, hidden, activation, part flags), each once
MODELS = list(dict.fromkeys((E, tuple(h), a, fl) for E, h, a, fl, _, _ in RANK_CASES))


def _ids(rng, vocab, B):
    return np.stack([rng.integers(0, v, B) for v in vocab], 1).astype(np.int32)


@pytest.mark.parametrize("E,hidden,act,flags", MODELS)
def test_fused_logits_match_oracle(E, hidden, act, flags):
    use_linear, use_mf, use_dnn = flags
    hidden = list(hidden)
    p, _, _, _ = make_problem(3, VOCAB26, E, hidden, 4, use_dnn=use_dnn)
    m = DeepFM(VOCAB26, embedding_size=E, hidden_units=hidden, use_linear=use_linear, use_mf=use_mf, use_dnn=use_dnn,
               activation=act, device="cuda")
    m.load_oracle_params(p)
    p64 = p.astype(np.float64)
    for B in BATCHES:
        ids = _ids(np.random.default_rng(B), VOCAB26, B)
        got = m.predict_fused(dev(ids))["logits"].cpu().numpy()[:, 0]
        ref = O.forward(p64, ids, use_linear=use_linear, use_mf=use_mf, use_dnn=use_dnn,
                        activation=act if act != "identity" else None)["logits"]
        err = max_err_scaled(got, ref)
        print("E=%d hidden=%s act=%s flags=%s B=%d err=%.3g" % (E, hidden, act, flags, B, err))
        assert err < 1e-5, (B, err)


@pytest.mark.parametrize("numeric", ["embed", "raw"])
def test_fused_logits_numeric_columns(numeric):
    vocab = VOCAB26[:6]
    p, _, _, _ = make_problem(5, vocab, 4, [16, 16], 4, n_numeric=2, use_dnn=True)
    use_mf = numeric == "embed"
    if numeric == "raw":
        k0, b0 = p.mlp[0]
        rng0 = np.random.default_rng(1)
        p.mlp[0] = (np.concatenate([k0[:6 * 4], (rng0.standard_normal((2, k0.shape[1])) * 0.3).astype(np.float32)]), b0)
    m = DeepFM(vocab, n_numeric=2, embedding_size=4, hidden_units=[16, 16], use_mf=use_mf, numeric=numeric, device="cuda")
    m.load_oracle_params(p)
    for B in BATCHES:
        rng = np.random.default_rng(B + 1)
        ids, x = _ids(rng, vocab, B), rng.standard_normal((B, 2)).astype(np.float32)
        got = m.predict_fused(dev(ids), dev(x))["logits"].cpu().numpy()[:, 0]
        ref = O.forward(p.astype(np.float64), ids, x.astype(np.float64), use_mf=use_mf, numeric=numeric)["logits"]
        err = max_err_scaled(got, ref)
        print("numeric=%s B=%d err=%.3g" % (numeric, B, err))
        assert err < 1e-5, (B, err)


def test_fused_logits_canned_wide_and_deep():
    """DNNLinearCombinedClassifier with narrower embedding columns and columns outside the wide part"""
    vocab = VOCAB26[:8]
    dims = [4, 2, 4, 3, 4, 1, 4, 4]
    wide = [True, False, True, True, False, True, True, False]
    p, _, _, _ = make_problem(6, vocab, 4, [16, 8], 4, use_dnn=True)
    p.emb = [a[:, :d].copy() for a, d in zip(p.emb, dims)]
    k0, b0 = p.mlp[0]
    keep = [f * 4 + j for f, d in enumerate(dims) for j in range(d)]
    p.mlp[0] = (k0[keep].copy(), b0)
    p.lin_w = [w if on else np.zeros_like(w) for w, on in zip(p.lin_w, wide)]
    m = DeepFM(vocab, embedding_size=4, hidden_units=[16, 8], use_mf=False, reduction="sum", field_dims=dims,
               wide_fields=wide, device="cuda")
    m.load_oracle_params(p)
    # (the unused slots of lin_w hold something: the mask, not their value, must keep them out)
    for f, on in enumerate(wide):
        if not on:
            m.lin_w[slice(*m._field_rows(f))] = 7.0
    for B in BATCHES:
        ids = _ids(np.random.default_rng(B + 2), vocab, B)
        got = m.predict_fused(dev(ids))["logits"].cpu().numpy()[:, 0]
        ref = O.forward(p.astype(np.float64), ids, use_mf=False, wide_fields=wide)["logits"]
        err = max_err_scaled(got, ref)
        print("wide and deep B=%d err=%.3g" % (B, err))
        assert err < 1e-5, (B, err)


def test_fused_logits_config3_shape():
    """26 fields x E = 64, hidden [512, 256, 128] (config 3 of BASELINE.json) with small vocabularies"""
    vocab = [40 + 3 * i for i in range(26)]
    p, _, _, _ = make_problem(9, vocab, 64, [512, 256, 128], 4)
    m = DeepFM(vocab, embedding_size=64, hidden_units=[512, 256, 128], device="cuda")
    m.load_oracle_params(p)
    for B in BATCHES:
        ids = _ids(np.random.default_rng(B + 3), vocab, B)
        got = m.predict_fused(dev(ids))["logits"].cpu().numpy()[:, 0]
        ref = O.forward(p.astype(np.float64), ids)["logits"]
        err = max_err_scaled(got, ref)
        print("config 3 shape B=%d err=%.3g" % (B, err))
        assert err < 1e-5, (B, err)


def test_one_field_fm_is_exactly_zero():
    vocab = [1000]
    for E in (4, 64):
        m = DeepFM(vocab, embedding_size=E, use_linear=False, use_mf=True, use_dnn=False, device="cuda")
        m.table.copy_(torch.randn(1000, E, device="cuda") * 3.0)
        ids = _ids(np.random.default_rng(E), vocab, 333)
        out = m.predict_fused(dev(ids))
        assert (out["logits"] == 0).all() and (out["logistic"] == 0.5).all() and (out["class_ids"] == 0).all()


def test_head_outputs_are_binary_predictions_bit_for_bit():
    p, _, _, _ = make_problem(4, VOCAB26, 4, [16, 16], 4)
    p.lin_bias[:] = -1.0
    m = DeepFM(VOCAB26, embedding_size=4, hidden_units=[16, 16], device="cuda")
    m.load_oracle_params(p)
    B = 1000
    out = m.predict_fused(dev(_ids(np.random.default_rng(0), VOCAB26, B)))
    x = out["logits"].reshape(-1).contiguous()
    lg = torch.empty(B, 1, device="cuda")
    pr = torch.empty(B, 2, device="cuda")
    cl = torch.empty(B, 1, dtype=torch.int64, device="cuda")
    m.k.mi_binary_predictions(x, None, B, lg, pr, cl, None)
    assert torch.equal(out["logistic"].view(torch.int32), lg.view(torch.int32))
    assert torch.equal(out["probabilities"].view(torch.int32), pr.view(torch.int32))
    assert torch.equal(out["class_ids"], cl) and out["classes"] is out["class_ids"]
    assert 0 < int(cl.sum()) < B                                     # both classes occur


@pytest.mark.parametrize("catchup", ["bounded", "exact"])
@pytest.mark.parametrize("E,hidden", [(4, [16, 16]), (64, [512, 256, 128])])
def test_fused_matches_engine_forward_after_lazy_adam(E, hidden, catchup):
    vocab = [50 + 3 * i for i in range(26)]
    rng = np.random.default_rng(11)
    p, _, _, _ = make_problem(12, vocab, E, hidden, 4)
    m = DeepFM(vocab, embedding_size=E, hidden_units=hidden, optimizer=OptimizerSpec("Adam", 0.01), catchup=catchup, device="cuda")
    m.load_oracle_params(p)
    for _ in range(4):                          # small batches: most rows sit out most steps (lazy catch-up)
        ids = _ids(rng, vocab, 16)
        y = (rng.random(16) < 0.4).astype(np.uint8)
        m.train_step(dev(ids), dev(y))
    q = dev(_ids(rng, vocab, 23 * 61))
    got = m.predict_fused(q)["logits"].cpu().numpy()[:, 0]         # (no explicit finalize_rows)
    ref = m.predict_logits(q).cpu().numpy()
    err = max_err_scaled(got, ref)
    print("after lazy Adam E=%d %s err=%.3g" % (E, catchup, err))
    assert err < 1e-5, err


@pytest.mark.parametrize("E,hidden", [(4, [16, 16]), (64, [512, 200, 48])])
def test_deterministic_and_independent_of_neighbours(E, hidden):
    p, _, _, _ = make_problem(7, VOCAB26, E, hidden, 4)
    m = DeepFM(VOCAB26, embedding_size=E, hidden_units=hidden, device="cuda")
    m.load_oracle_params(p)
    ids = _ids(np.random.default_rng(1), VOCAB26, 33)
    a = m.predict_fused(dev(ids))
    b = m.predict_fused(dev(ids))
    for k in ("logits", "logistic", "probabilities"):
        assert torch.equal(a[k].view(torch.int32), b[k].view(torch.int32))
    assert torch.equal(a["class_ids"], b["class_ids"])
    c = m.predict_fused(dev(ids[:32]))
    assert torch.equal(a["logits"][:32].view(torch.int32), c["logits"].view(torch.int32))
    assert torch.equal(a["probabilities"][:32].view(torch.int32), c["probabilities"].view(torch.int32))


def test_limits_raise_before_anything_is_launched():
    k = HipKernels()
    dev = "cuda"
    SENT = 12345.0

    def build(B=4, F=3, E=4, hidden=(8,), **over):
        """the entry's arguments on a tiny model, sizes overridden one at a time, and the sentinel-filled outputs"""
        vocab = 5
        widths = [F * E] + list(hidden) + [1]
        offs, o = [], 0
        for fi, fo in zip(widths[:-1], widths[1:]):
            offs += [o, o + fi * fo]
            o += fi * fo + fo
        dense = torch.zeros(o + 16, device=dev)
        table = torch.zeros(F * vocab, max(E, 4), device=dev)
        lin_w = torch.zeros(F * vocab, device=dev)
        off = torch.arange(F, dtype=torch.int64, device=dev) * vocab
        ids = torch.zeros(max(B, 1), F, dtype=torch.int32, device=dev)
        n = max(B, 1)
        outs = [torch.full((n,), SENT, device=dev), torch.full((n,), SENT, device=dev), torch.full((n, 2), SENT, device=dev),
                torch.full((n,), 12345, dtype=torch.int64, device=dev)]
        args = dict(table=table, ts=0, lin_w=lin_w, ls=1, off=off, ids=ids, x=None, B=B, F=F, E=E, nd=0, dense=dense,
                    layer_off=torch.tensor(offs, dtype=torch.int64), widths=torch.tensor(widths, dtype=torch.int32),
                    n_layers=len(widths) - 1, act=1, lin=1, fm=1, dnn=1, raw=0, lb=o, ne=-1, ln=-1, wide=min((1 << F) - 1, 2 ** 64 - 1))
        args.update(over)
        return list(args.values()) + outs + [None, 0], outs

    untouched = lambda outs: all(bool((t == 12345).all()) for t in outs)
    args, outs = build()
    k.mi_predict_fused(*args)                                        # the tiny model itself runs, and writes every output
    torch.cuda.synchronize()
    assert not any(bool((t == 12345).any()) for t in outs)
    for kw, msg in ((dict(B=0), "at least one request"), (dict(F=65), "at most 64"), (dict(E=6), "embedding size 6"),
                    (dict(E=260), "embedding size 260"), (dict(E=0), "embedding size 0"),
                    (dict(hidden=(4,) * 9), "9 hidden layers"), (dict(hidden=(8, 513)), "hidden width 513"),
                    (dict(hidden=(1024,)), "hidden width 1024"), (dict(act=4), "activation 4"),
                    (dict(lin=0, fm=0, dnn=0, n_layers=0), "no part of the model")):
        args, outs = build(**kw)
        with pytest.raises(_lib.MiError, match=msg):
            k.mi_predict_fused(*args)
        torch.cuda.synchronize()
        assert untouched(outs), kw                                   # nothing was launched


# ---- end to end: train, then python -m trainers.predict in both modes ------------------------------------------------
def test_predict_cli_end_to_end(tmp_path):
    job = str(tmp_path / "job")
    _run_module("trainers.deep_fm", ["--synthetic", "4000", "--job-dir", job, "--train-steps", "48", "--batch-size", "32"])
    logits, cls = {}, {}
    for mode in ("fused", "layered"):
        out = str(tmp_path / (mode + ".csv"))
        _run_module("trainers.predict", ["--job-dir", job, "--input", "synthetic:400:2", "--mode", mode, "--output", out])
        rows = list(csv.DictReader(open(out)))
        assert len(rows) == 400
        logits[mode] = np.asarray([float(r["logit"]) for r in rows])
        cls[mode] = np.asarray([int(r["class_id"]) for r in rows])
    # each mode is within 1e-5 of the exact value (the tests above), so their distance is at most the sum
    err = max_err_scaled(logits["fused"], logits["layered"])
    print("fused vs layered CLI err=%.3g" % err)
    assert err < 2e-5, err
    rms = np.sqrt(np.mean(logits["layered"] ** 2))
    clear = np.abs(logits["layered"]) > 2e-5 * rms
    assert clear.any() and np.array_equal(cls["fused"][clear], cls["layered"][clear])
