"""Models, flat arrays and an fp64 reference for the one-launch serving forward of csrc/serve.hip (mi_predict_fused,
mi_predict_group) at the edges of its loops.  Host only: numpy, no device, no fixtures.  The CPU half is
test_serve_cases_cpu.py, the GPU half test_hip_serve_edges.py; what was measured is in profiles/serve_edges.md.

What the kernel does (restated here once).  A workgroup of 4 waves serves 32 requests.
  layer 1    the concat is walked in float4 chunks, cpf = E / 4 per field; the two lane halves take neighbouring chunks, a
             block covers 8 chunks, two blocks alternate.  Numeric columns follow two k per step: kn = n_numeric E columns
             (numeric embeddings) or n_numeric (raw values), so kn is odd only with an odd count of raw columns.
  later      16 k per block, two blocks alternating; the second block of a round is computed only if k0 + 16 < fan-in.
  tiles      nt = ceil(fan-out / 128) selects the form with 1, 2 or 4 output tiles per wave (nt = 3 takes the 4-tile form).
  wide part  8 threads per request, up to 8 fields each: 64 fields fill every slot, bit f of wide_fields switches field f on.
The entry reads the caller's arrays in place: table rows `table_stride` floats apart, linear weights `lin_stride` apart,
kernel_0 with widths[0] >= the input columns, the dense buffer with anything between its variables.  build() fills every
place the kernel must not read with poison, so a read outside an extent shows as NaN (or as 1e30) in the logit."""
from collections import namedtuple
from types import SimpleNamespace

import numpy as np

F32 = np.float32
ACT_NAMES = {0: None, 1: "relu", 2: "sigmoid", 3: "tanh"}            # the engine's code -> the oracle's name
BATCHES = (1, 31, 32, 33, 65)
B_MAX = max(BATCHES)
MAX_INPUT_COLUMNS = 1664                                             # config 3: where the 1e-5 contract has been measured
ROW_POISON = 1e30                                                    # rows of kernel_0 past the input columns (0 x finite = 0)

Case = namedtuple("Case", "name F E nd mode hidden act parts wide ts ls pad guard")


def _case(name, F, E, hidden, guard, nd=0, mode=None, act=1, parts=(1, 1, 1), wide=None, ts=0, ls=1, pad=0):
    """wide: None = every field; ts: table_stride (0 = E); ls: lin_stride; pad: widths[0] - input columns"""
    assert (mode is None) == (nd == 0) and mode in (None, "embed", "raw") and not (mode == "raw" and parts[1])
    full = (1 << F) - 1
    return Case(name, F, E, nd, mode, tuple(hidden), act, tuple(parts), full if wide is None else wide & full, ts, ls, pad, guard)


EDGE_BITS = (1 << 0) | (1 << 31) | (1 << 32) | (1 << 63)
CHAIN = (15, 16, 17, 31, 32, 33, 47, 49)
RAW = dict(mode="raw", parts=(1, 0, 1))

CASES = [
    # ---- layer 1: the lane halves' walk over (field, chunk) ----
    _case("walk_e12", 3, 12, [16], "cpf = 3: the halves sit in different fields and wrap at different steps; 9 chunks; "
          "table_stride = E + 4, lin_stride = 2", ts=16, ls=2),
    _case("walk_e20", 5, 20, [16], "cpf = 5; 25 chunks; table_stride = 2 E, lin_stride = 5", ts=40, ls=5),
    _case("one_field", 1, 4, [8], "F = 1: one chunk, the upper lane half starts past the concat; widths[0] = d_in + 4", pad=4),
    _case("two_fields", 2, 4, [8], "F = 2: two chunks, one per lane half"),
    # ---- layer 1: blocks of 8 chunks ----
    _case("e256", 2, 256, [33], "E = 256: 64 chunks per field, 128 in all; fan-out 33"),
    _case("chunks7", 7, 4, [16], "7 chunks: one short of a block"),
    _case("chunks8", 2, 16, [16], "8 chunks: exactly one block, the second is all off"),
    _case("chunks17", 17, 4, [16], "17 chunks: two blocks and one chunk"),
    # ---- the wide part's slots and mask bits ----
    _case("f63_full", 63, 4, [16], "F = 63: the last slot of the last thread is past F"),
    _case("f63_edge_bits", 63, 4, [16], "F = 63, only bits {0, 31, 32}", wide=EDGE_BITS),
    _case("f63_edge_clear", 63, 4, [16], "F = 63, bits {0, 31, 32} clear", wide=~EDGE_BITS),
    _case("f64_full", 64, 4, [16], "F = 64: all 8 slots of every thread, mask bits 32..63"),
    _case("f64_edge_bits", 64, 4, [16], "F = 64, only bits {0, 31, 32, 63}", wide=EDGE_BITS),
    _case("f64_edge_clear", 64, 4, [16], "F = 64, bits {0, 31, 32, 63} clear", wide=~EDGE_BITS),
    # (the three masks above read the same whether bit f or bit f % 32 is taken: this one tells a 32-bit shift from a 64-bit one)
    _case("f64_high_word", 64, 4, [16], "F = 64, only bits 32 .. 62: the two words of the mask differ", wide=0x7FFFFFFF << 32),
    # ---- later layers: fan-ins around 16, 32 and 48; 8 hidden layers = 9 buffer swaps; 3 chunks ----
    _case("chain_identity", 3, 4, CHAIN, "fan-ins 15 .. 49, 8 hidden layers, identity", act=0),
    _case("chain_relu", 3, 4, CHAIN, "fan-ins 15 .. 49, 8 hidden layers, relu", act=1),
    _case("chain_sigmoid", 3, 4, CHAIN, "fan-ins 15 .. 49, 8 hidden layers, sigmoid", act=2),
    _case("chain_tanh", 3, 4, CHAIN, "fan-ins 15 .. 49, 8 hidden layers, tanh", act=3),
    # ---- tile dispatch ----
    _case("tiles_129_257_1", 4, 8, [129, 257, 1], "nt = 2 with one row in its last tile, nt = 3 (4-tile form), width 1 and fan-in 1"),
    _case("tiles_512_511", 4, 8, [512, 511], "nt = 4 full, then one row short; fan-ins 512 and 511"),
    _case("tiles_384_385", 4, 8, [384, 385], "nt = 3 with one wave idle on its last tile, then nt = 4 with one row in tile 12"),
    # ---- the largest legal launch ----
    _case("largest", 64, 4, [512, 512], "F = 64 with widths 512 / 512: 139,264 bytes of dynamic LDS"),
    # ---- numeric columns ----
    _case("raw1", 6, 4, [16], "one raw column: kn = 1, the upper lane half is off in the only step", nd=1, **RAW),
    _case("raw3", 6, 4, [16], "three raw columns: kn = 3, an odd last column; widths[0] = d_in + 4", nd=3, pad=4, **RAW),
    _case("embed1", 6, 4, [48, 16], "one embedded column: kn = E; fan-ins 48 and 16", nd=1, mode="embed"),
    _case("embed3", 6, 12, [31], "three embedded columns at odd cpf", nd=3, mode="embed"),
    _case("f0_embed3", 0, 4, [16], "F = 0: no table, three embedded columns, all parts on", nd=3, mode="embed"),
    _case("f0_raw1", 0, 4, [16], "F = 0, one raw column, DNN only: fan-in 1 of layer 1", nd=1, mode="raw", parts=(0, 0, 1)),
]
# one ensemble: three members over the same five fields that differ most in LDS need (the plan's is the largest member's)
GROUP = [
    _case("group_no_hidden", 5, 4, [], "member 0: the logits layer alone, 768 bytes of LDS"),
    _case("group_chain", 5, 12, CHAIN, "member 1: odd cpf and the fan-in chain"),
    _case("group_512_512", 5, 4, [512, 512], "member 2: 4 tiles per wave in both buffers"),
]
BY_NAME = {c.name: c for c in CASES + GROUP}
# The seed of a case's weights and requests: the lowest at which the fp32 evaluation of the formula stays within a quarter
# of the kernel's contract at every batch size (test_serve_cases_cpu.py asserts it).  With one request max_err_scaled is a
# plain relative error, and a request whose parts cancel to a logit near zero misses 1e-5 in exact fp32 arithmetic.
SEED = dict({c.name: 0 for c in CASES + GROUP}, chain_identity=1, raw1=1, group_no_hidden=1)


def vocab(case):
    """small vocabularies that differ by field (one row at least, so id 0 and id vocab - 1 may coincide); with one or two
    fields 40 rows more, so that the 65 requests are not three models' worth of distinct inputs"""
    return [1 + (5 * f + 2) % 9 + (40 if case.F <= 2 else 0) for f in range(case.F)]


def input_columns(case):
    return case.F * case.E + case.nd * (1 if case.mode == "raw" else case.E)


def n_layers(case):
    return len(case.hidden) + 1 if case.parts[2] else 0


def lds_bytes(case):
    """dynamic LDS of a workgroup: the rows [F][32] int32 and the two activation buffers, which hold the outputs of the
    even and of the odd layers (the logits layer included)"""
    outs = (list(case.hidden) + [1]) if case.parts[2] else []
    return 4 * 32 * (case.F + max(outs[0::2], default=0) + max(outs[1::2], default=0))


def _trunc_normal(rng, shape, std):
    return (np.clip(rng.standard_normal(shape), -2, 2) * std).astype(F32)


def build(case, seed=None):
    """The entry's flat arrays for `case`, as numpy (fp32 unless noted):
      table [R, ts]  columns E .. ts - 1 NaN                       field_off [F] int64
      lin_w [R ls]   the weight of row r at r ls, NaN between the weights and in the slots of fields outside the mask
      dense          kernel_i [widths[i], widths[i + 1]] and bias_i at layer_off[2 i], layer_off[2 i + 1] (int64), then the
                     wide bias, the numeric embeddings [nd, E] (offset a multiple of 4) and the numeric linear weights; NaN
                     between and after them, 1e30 in the rows of kernel_0 past the input columns
      widths [n_layers + 1] int32, lin_bias_off / num_emb_off / lin_num_off (-1 = absent)
    and the extents: table_ok, lin_ok, dense_ok (what the kernel may read), dense_pad (the 1e30 rows)."""
    rng = np.random.default_rng(SEED[case.name] if seed is None else seed)
    F, E, nd = case.F, case.E, case.nd
    voc = vocab(case)
    R = int(sum(voc))
    ts = case.ts or E
    a = SimpleNamespace(ts=ts, ls=case.ls, R=R, vocab=voc)
    a.field_off = np.concatenate([[0], np.cumsum(voc)[:-1]]).astype(np.int64) if F else np.zeros(0, np.int64)
    a.table = np.full((R, ts), np.nan, F32)
    a.table[:, :E] = _trunc_normal(rng, (R, E), 1.0 / np.sqrt(E))
    a.table_ok = np.zeros((R, ts), bool)
    a.table_ok[:, :E] = True
    a.lin_w = np.full(R * case.ls, np.nan, F32)
    a.lin_ok = np.zeros(R * case.ls, bool)
    for f in range(F):
        if (case.wide >> f) & 1:
            at = (a.field_off[f] + np.arange(voc[f])) * case.ls
            a.lin_w[at] = (rng.standard_normal(voc[f]) * 0.3).astype(F32)
            a.lin_ok[at] = True

    segs, oks, pads = [], [], []
    pos = [0]

    def gap(n):
        segs.append(np.full(n, np.nan, F32)); oks.append(np.zeros(n, bool)); pads.append(np.zeros(n, bool))
        pos[0] += n

    def put(values, pad_from=None):
        v = np.ascontiguousarray(values, F32).reshape(-1)
        ok = np.ones(v.size, bool)
        if pad_from is not None:
            ok[pad_from:] = False
        at = pos[0]
        segs.append(v); oks.append(ok); pads.append(~ok)
        pos[0] += v.size
        return at

    d_in = input_columns(case)
    L = n_layers(case)
    widths = ([d_in + case.pad] + list(case.hidden) + [1]) if L else []
    layer_off = []
    gap(3)
    for i in range(L):
        fi, fo = widths[i], widths[i + 1]
        fan = d_in if i == 0 else fi
        lim = np.sqrt(6.0 / (fan + fo))
        k = np.full((fi, fo), ROW_POISON, F32)
        k[:fan] = rng.uniform(-lim, lim, (fan, fo))
        layer_off.append(put(k, pad_from=fan * fo))
        gap(5)
        bias = rng.standard_normal(fo) * 0.05
        if fo == 1 and i + 1 < L:
            bias[:] = 1.0                                              # (a hidden layer of one unit: relu must not cut every request off)
        layer_off.append(put(bias))
        gap(1 + i % 3)
    a.lin_bias_off = put([0.1]) if case.parts[0] else -1
    gap(2)
    a.num_emb_off = a.lin_num_off = -1
    if nd and case.mode == "embed":
        gap(4 + (-pos[0]) % 4)                                         # (16-byte aligned: the kernel reads float4)
        lim = np.sqrt(6.0 / (nd + E))
        a.num_emb_off = put(rng.uniform(-lim, lim, (nd, E)))
        gap(3)
    if nd and case.parts[0]:
        a.lin_num_off = put(rng.standard_normal(nd) * 0.3)
    gap(7)
    a.dense, a.dense_ok, a.dense_pad = np.concatenate(segs), np.concatenate(oks), np.concatenate(pads)
    a.layer_off = np.asarray(layer_off, np.int64)
    a.widths = np.asarray(widths, np.int32)
    a.n_layers = L
    return a


def requests(case, seed=None, B=B_MAX):
    """(ids [B, F] int32, x [B, nd] fp32 or None): request 0 holds id 0 of every field, request 1 the last id, the rest
    are uniform.  A smaller batch of the same case is a prefix of this one."""
    rng = np.random.default_rng(1000 + (SEED[case.name] if seed is None else seed))
    voc = vocab(case)
    ids = np.stack([rng.integers(0, v, B) for v in voc], 1).astype(np.int32) if case.F else np.zeros((B, 0), np.int32)
    if case.F:
        ids[0] = 0
        if B > 1:
            ids[1] = np.asarray(voc) - 1
    x = rng.standard_normal((B, case.nd)).astype(F32) if case.nd else None
    return ids, x


def group_requests():
    """the ids every member of GROUP is asked (the members share their fields): the first member's own"""
    return requests(GROUP[0])[0]


def _act(code, v):
    one = v.dtype.type(1)
    if code == 1:
        return np.maximum(v, v.dtype.type(0))
    if code == 2:
        return one / (one + np.exp(-v))
    if code == 3:
        return np.tanh(v)
    return v


def reference(case, a, ids, x, dtype=np.float64):
    """The forward of include/mi355x_rec.h on the flat arrays, one request and one field at a time, in `dtype` (fp64: the
    reference; fp32: the same formula at the kernel's precision).  Returns the parts [B] on their own — lin (the wide sum
    plus its bias), fm, dnn, zero where the case lacks the data for one — and logits = ((lin) + fm) + dnn over the parts
    the case switches on.  Reads exactly the extents: a poisoned neighbour never enters."""
    dt = np.dtype(dtype).type
    F, E, nd, raw = case.F, case.E, case.nd, case.mode == "raw"
    B = ids.shape[0]
    table, lin_w, dense = a.table.reshape(-1).astype(dt), a.lin_w.astype(dt), a.dense.astype(dt)
    xs = None if x is None else x.astype(dt)
    V = dense[a.num_emb_off:a.num_emb_off + nd * E].reshape(nd, E) if a.num_emb_off >= 0 else None
    d_in = input_columns(case)
    out = {k: np.zeros(B, dt) for k in ("lin", "fm", "dnn", "logits")}
    for b in range(B):
        lin, s, q, cols = dt(0), np.zeros(E, dt), np.zeros(E, dt), []
        for f in range(F):
            r = int(a.field_off[f]) + int(ids[b, f])
            row = table[r * a.ts:r * a.ts + E]
            if (case.wide >> f) & 1:
                lin = lin + lin_w[r * a.ls]
            s, q = s + row, q + row * row
            cols.append(row)
        for j in range(nd):
            if a.lin_num_off >= 0:
                lin = lin + xs[b, j] * dense[a.lin_num_off + j]
            if raw:
                cols.append(xs[b, j:j + 1])
            else:
                row = xs[b, j] * V[j]
                s, q = s + row, q + row * row
                cols.append(row)
        if a.lin_bias_off >= 0:
            lin = lin + dense[a.lin_bias_off]
        out["lin"][b] = lin
        if not raw:
            out["fm"][b] = dt(0.5) * (s * s - q).sum(dtype=dt)
        if a.n_layers:
            h = np.concatenate(cols)
            assert h.shape == (d_in,)
            for i in range(a.n_layers):
                fi, fo = int(a.widths[i]), int(a.widths[i + 1])
                w0, b0 = int(a.layer_off[2 * i]), int(a.layer_off[2 * i + 1])
                W = dense[w0:w0 + fi * fo].reshape(fi, fo)[:h.size]    # (kernel_0: the rows of the input columns)
                h = h @ W + dense[b0:b0 + fo]
                if i + 1 < a.n_layers:
                    h = _act(case.act, h)
            out["dnn"][b] = h[0]
    z = np.zeros(B, dt)
    for on, part in zip(case.parts, ("lin", "fm", "dnn")):
        if on:
            z = z + out[part]
    out["logits"] = z
    return out
