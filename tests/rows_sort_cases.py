"""Inputs and references for the int32 sorts of csrc/sort.hip and the routing helpers beside them — mi_sort_unique_rows (its
three forms), mi_shard_keys -> mi_sort_unique_rows_slots -> mi_route_requests as parallel._route chains them,
mi_catchup_rows_by_gap and mi_sort_unique_fields: the key ranges that select every digit plan, the sizes around the
one-workgroup limit and the tile, the key patterns that stress the ballot ranking and the head compaction, and references
that never pack a key.  No GPU code and no fixtures; the CPU half is test_rows_sort_cases_cpu.py, the GPU half
test_hip_rows_sort.py.

What the entries do (restated here once).  The rows sort orders the entries by (row, entry index): a stable sort.  Up to
SMALL_N keys one workgroup sorts (key << 10 | index) bitonically; above it an LSD radix sort of 4,096-key tiles runs
`passes` passes of `nbits`-bit digits, planned from the key range alone:
  bits = max(1, ceil(log2 num_rows_total)),  passes = ceil(bits / 9),  nbits = ceil(bits / passes).
The passes alternate between two workspace buffers, so the plan decides which buffer the compaction reads, and with
uniq_rows == NULL the last pass writes the caller's sorted_entry itself.  Nothing here has a tolerance: every output is an
integer with one right value."""
import numpy as np

INT32_MAX = 2 ** 31 - 1
SMALL_N = 1024                   # sort.hip's kSmallN: the last size of the one-workgroup kernel
TILE = 4096                      # radix.h's kTile
MAX_BITS = 9                     # radix.h's kMaxBits
GUARD = 64                       # elements of FILL before and after every output
FILL = -7


def plan(num_rows_total):
    """(passes, nbits) of the rows sort for keys in [0, num_rows_total)"""
    bits = max(1, int(num_rows_total - 1).bit_length())                 # ceil(log2 R) for R >= 1
    passes = -(-bits // MAX_BITS)
    return passes, -(-bits // passes)


# num_rows_total -> the plan it must select (test_rows_sort_cases_cpu.py holds plan() to this table)
KEY_RANGES = [(1, (1, 1)), (2, (1, 1)), (512, (1, 9)), (513, (2, 5)), (2 ** 18, (2, 9)), (2 ** 18 + 1, (3, 7)),
              (2 ** 27, (3, 9)), (2 ** 27 + 1, (4, 7)), (INT32_MAX, (4, 8))]

# around a wave (64), a workgroup (256), the one-workgroup limit (1,024), one, two and three tiles
SIZES = [1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097, 8192, 8193, 12289]
PATTERNS = ["uniform", "constant", "descending", "ascending", "mod3", "distinct"]
ALL_PATTERNS_AT = (1024, 1025, 4097, 8193)


def patterns_for(n, R):
    """every pattern at the four sizes where the kernels change, uniform + constant elsewhere; distinct needs R >= n"""
    if n not in ALL_PATTERNS_AT:
        return ["uniform", "constant"]
    return [p for p in PATTERNS if p != "distinct" or R >= n]


def keys(pattern, n, R, rng):
    """int32 [n], every key in [0, R)"""
    i = np.arange(n, dtype=np.int64)
    if pattern == "uniform":
        k = rng.integers(0, R, n)
        if n >= 2:
            k[0], k[n - 1] = R - 1, 0
        if n >= 4:
            k[n // 2] = R - 1                               # a duplicate far from its first entry at every range
    elif pattern == "constant":                             # one bin holds everything: U = 1, stability
        k = np.full(n, R - 1)
    elif pattern == "descending":                           # strictly descending where R >= n
        k = ((n - 1 - i) * R) // n
    elif pattern == "ascending":                            # already sorted
        k = (((n - 1 - i) * R) // n)[::-1]
    elif pattern == "mod3":                                 # three values: sorted, long runs across wave and tile edges
        k = np.minimum(i % 3, R - 1)
    else:
        assert pattern == "distinct" and R >= n, (pattern, n, R)
        k = (i * R) // n                                    # strictly ascending (R >= n), holds 0
        k[n - 1] = R - 1                                    # (above k[n - 2]: (n - 1) R // n <= R - 1)
        k = k[rng.permutation(n)]
    k = np.ascontiguousarray(k).astype(np.int32)
    assert k.shape == (n,) and k.min() >= 0 and int(k.max()) < R
    return k


class SortRef:
    """sorted_entry [n], uniq [U], seg_start [U + 1] (closing n), U, slot_of_entry [n]"""

    def __init__(self, sorted_entry, uniq, seg_start, slot_of_entry):
        self.sorted_entry, self.uniq, self.seg_start, self.slot_of_entry = sorted_entry, uniq, seg_start, slot_of_entry
        self.U = len(uniq)


def sort_reference(rows):
    rows = np.asarray(rows)
    order = np.argsort(rows, kind="stable")
    uniq, inverse = np.unique(rows, return_inverse=True)
    sr = rows[order]
    starts = np.flatnonzero(np.r_[True, sr[1:] != sr[:-1]])
    return SortRef(order.astype(np.int32), uniq.astype(np.int32), np.r_[starts, len(rows)].astype(np.int32),
                   inverse.reshape(-1).astype(np.int32))


# ---- routing -------------------------------------------------------------------------------------------------------------------
class RouteRef:
    """slot [n], send_rows [U], counts [chunks * world], sorted_entry [n], U, chunks"""

    def __init__(self, slot, send_rows, counts, sorted_entry, chunks):
        self.slot, self.send_rows, self.counts, self.sorted_entry, self.chunks = slot, send_rows, counts, sorted_entry, chunks
        self.U = len(send_rows)


def route_triples(rows, world, self_rank, entries_per_chunk):
    """(chunk, pos, local) per entry: chunk = i // epc (0 when epc == 0), owner = r % world, local = r // world; pos is the
    owner (self_rank = -1), else the other ranks in rank order and the asking rank last"""
    r = np.asarray(rows).astype(np.int64)
    n = len(r)
    chunk = np.arange(n) // entries_per_chunk if entries_per_chunk > 0 else np.zeros(n, np.int64)
    owner, local = r % world, r // world
    pos = owner.copy()
    if self_rank >= 0:
        pos[owner > self_rank] -= 1
        pos[owner == self_rank] = world - 1
    return chunk, pos, local


def route_reference(rows, world, self_rank, entries_per_chunk, rows_per_rank):
    """the routing chain from tuples: the requests are the lexicographically sorted distinct (chunk, pos, local)"""
    chunk, pos, local = route_triples(rows, world, self_rank, entries_per_chunk)
    n = len(chunk)
    assert n == 0 or int(local.max()) < rows_per_rank
    chunks = -(-n // entries_per_chunk) if entries_per_chunk > 0 else 1
    req, inverse = np.unique(np.stack([chunk, pos, local], 1), axis=0, return_inverse=True)
    counts = np.zeros((chunks, world), np.int64)
    np.add.at(counts, (req[:, 0], req[:, 1]), 1)
    return RouteRef(inverse.reshape(-1).astype(np.int32), req[:, 2].astype(np.int32), counts.reshape(-1).astype(np.int32),
                    np.lexsort((np.arange(n), local, pos, chunk)).astype(np.int32), chunks)


ROUTE_R = 10_007                 # a prime: no multiple of any world below
ROUTE_WORLDS = [1, 2, 3, 8]
ROUTE_SIZES = [1, 1024, 1025, 4097, 8200]
ROUTE_SHORT = [(1025, 512), (4097, 1366)]     # (n, entries_per_chunk) with n % epc != 0: three chunks, the last one short


def route_ranks(world):
    """-1, the first, the last and — from three ranks on — one middle rank"""
    return sorted({-1, 0, world - 1} | ({world // 2} if world >= 3 else set()))


def route_cases(world):
    """(self_rank, n, entries_per_chunk, chunks): C in {1, 2, 4} where it divides n (C = 1 passes 0 entries per chunk, as
    parallel._route does), then the short last chunks"""
    out = []
    for self_rank in route_ranks(world):
        for n in ROUTE_SIZES:
            for C in (1, 2, 4):
                if n % C == 0 and n >= C:
                    out.append((self_rank, n, n // C if C > 1 else 0, C))
        for n, epc in ROUTE_SHORT:
            out.append((self_rank, n, epc, -(-n // epc)))
    return out


def route_rows(n, rng):
    """rows in [0, ROUTE_R) with duplicates, holding the first and the last row"""
    r = rng.integers(0, ROUTE_R, n)
    if n >= 4:
        r[n // 2] = r[0]
        r[1], r[n - 2] = ROUTE_R - 1, 0
    return r.astype(np.int32)


# ---- the catch-up's order --------------------------------------------------------------------------------------------------------
GAP_STEP_TO = 1500
GAP_NMAX = [1, 1024, 1025, 4096, 4097, 8193]
GAP_STRIDES = [1, 4]
# gaps 0 (= stamp == step_to), 1, 61, 62, 63, 64, 1,000; never applied (0); stamped after step_to
GAP_STAMPS = [GAP_STEP_TO - g for g in (0, 1, 61, 62, 63, 64, 1000)] + [0, GAP_STEP_TO + 5]


def gap_us(n_max):
    return sorted({0, 1, n_max - 1, n_max})


def gap_case(n_max, stride, rng):
    """(uniq_rows [n_max] ascending distinct rows of a table of R rows, stamps as the flat [R * stride] int32 array whose
    element r * stride is row r's stamp — the other elements hold a stamp that would sort differently)"""
    R = 3 * n_max + 7
    rows = np.sort(rng.choice(R, n_max, replace=False)).astype(np.int32)
    stamps = np.asarray(GAP_STAMPS, np.int32)[rng.integers(0, len(GAP_STAMPS), R)]
    stamps[rows[:len(GAP_STAMPS)]] = GAP_STAMPS[:len(rows)]             # every class among the first rows asked for
    rec = np.full((R, stride), GAP_STEP_TO - 30, np.int32)
    rec[:, 0] = stamps
    return rows, rec.reshape(-1)


def gap_reference(uniq_rows, U, stamps, stride, step_to):
    """the first U rows in the stable order of key = min(step_to - s, 62) where 0 < s < step_to, else 0"""
    rows = np.asarray(uniq_rows)[:U]
    s = np.asarray(stamps)[rows.astype(np.int64) * stride].astype(np.int64)
    key = np.where((s > 0) & (s < step_to), np.minimum(step_to - s, 62), 0)
    return rows[np.argsort(key, kind="stable")]


# ---- the per-field sort ----------------------------------------------------------------------------------------------------------
def field_ids(B, vocabs, rng):
    """ids [B, F] int32, field f uniform in [0, vocabs[f]) and holding 0 and vocabs[f] - 1"""
    cols = []
    for f, v in enumerate(vocabs):
        c = rng.integers(0, v, B)
        c[(7 + f) % B], c[(B - 3 - f) % B] = v - 1, 0
        cols.append(c)
    return np.stack(cols, 1).astype(np.int32)


def field_offsets(vocabs):
    off = np.zeros(len(vocabs), np.int64)
    off[1:] = np.cumsum(vocabs)[:-1]
    return off


def fields_reference(ids, off):
    """(sorted_entry [B F], uniq global rows [U], seg_start [U + 1]): every field's ids sorted on their own, stable, the
    fields one after the other"""
    B, F = ids.shape
    se, uq, sg = [], [], []
    for f in range(F):
        col = ids[:, f]
        if int(col.max()) < 2 ** 15:
            col = col.astype(np.int16)                     # (numpy's stable sort of 16-bit integers is a radix sort)
        order = np.argsort(col, kind="stable")
        sc = ids[order, f]
        first = np.flatnonzero(np.r_[True, sc[1:] != sc[:-1]])
        se.append(order * F + f)
        uq.append(off[f] + sc[first])
        sg.append(f * B + first)
    sg.append(np.array([B * F]))
    return np.concatenate(se).astype(np.int32), np.concatenate(uq).astype(np.int32), np.concatenate(sg).astype(np.int32)


FIELD_MAX_VOCABS = [512, 2 ** 27, 2 ** 28, 2 ** 28 + 1, 2 ** 30]


def field_vocabs(max_vocab):
    """[max_vocab, 1000] — the second held to max_vocab, which bounds every field's range"""
    return [max_vocab, min(1000, max_vocab)]
