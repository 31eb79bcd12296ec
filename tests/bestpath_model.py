"""The contract of sctc_ctc_bestpath_batch (include/sctc.h) in NumPy: the arg-max of every
frame, the collapse of repeats with a set of symbols that are never emitted, the frames of every label and the
float64 sum of the arg-max entries.  Also the case tables that tests/test_gpu_bestpath.py runs on the device;
tests/test_bestpath_model_cpu.py checks without a GPU that every table holds what its name says."""
import math

import numpy as np

FB = 256        # frames a workgroup takes at a time (csrc/ctc_bestpath.hip, _sctc.BESTPATH_FRAMES_PER_BLOCK)
WAVE = 64
LANE_MAX_A = 4096   # alphabets up to this take a row per lane, larger ones a row per wave

T_SWEEP = (0, 1, 2, 63, 64, 65, 255, 256, 257, FB - 1, FB + 1, 2 * FB + 1)
A_SWEEP = (1, 2, 33, 64, 65)
# both sides of the mapping switch: rows of 16 KB and more, so fewer lengths -- none, one, a wave edge, a block edge
A_SWITCH = (LANE_MAX_A, LANE_MAX_A + 1)
T_SWITCH = (0, 1, 65, FB + 1)


def argmax_rows(rows):
    """int32 [T]: the column of the first maximum of every row of [T, A]; a row of only -inf gives 0"""
    rows = np.asarray(rows)
    if rows.shape[0] == 0:
        return np.zeros(0, dtype=np.int32)
    return np.argmax(rows, axis=1).astype(np.int32)     # the first maximum; every entry equal (-inf): 0


def runs(best):
    """[(symbol, first, last)] of the maximal runs of equal neighbours"""
    out = []
    for t, b in enumerate(best):
        if t == 0 or b != best[t - 1]:
            out.append([int(b), t, t])
        else:
            out[-1][2] = t
    return [tuple(r) for r in out]


def collapse(best, drop=()):
    """(ids int32 [U], spans int32 [U, 2]): frame t emits best[t] iff (t == 0 or best[t] != best[t-1]) and best[t]
    is not in drop; the span of a label is the run of equal best it starts"""
    drop = set(int(d) for d in drop)
    kept = [r for r in runs(best) if r[0] not in drop]
    ids = np.array([r[0] for r in kept], dtype=np.int32)
    spans = np.array([[r[1], r[2]] for r in kept], dtype=np.int32).reshape(-1, 2)
    return ids, spans


def decode(rows, drop=()):
    """(best, ids, spans, score): score = sum_t rows[t, best[t]] in float64, correctly rounded (math.fsum; -inf
    if any term is)"""
    rows = np.asarray(rows)
    best = argmax_rows(rows)
    ids, spans = collapse(best, drop)
    vals = rows[np.arange(rows.shape[0]), best].astype(np.float64) if rows.shape[0] else np.zeros(0)
    score = -np.inf if np.isneginf(vals).any() else math.fsum(vals)
    return best, ids, spans, float(score)


def abs_sum(rows, best):
    vals = np.asarray(rows)[np.arange(len(best)), best].astype(np.float64)
    return float(np.abs(vals).sum()) if len(best) else 0.0


# ---- inputs ----

def plant(best, A, dtype, rs):
    """[T, A] rows on the dyadic grid (multiples of 2^-10 in [-8, 0]) whose first maximum of row t is column
    best[t]: every other column is strictly smaller.  Sums of such values are exact in float64 in any order."""
    best = np.asarray(best, dtype=np.int64)
    T = best.shape[0]
    rows = rs.randint(-8 * 1024, -1024, size=(T, A)).astype(np.float64) / 1024.0
    if T:
        rows[np.arange(T), best] = rs.randint(-1023, 1, size=T).astype(np.float64) / 1024.0
    return rows.astype(dtype)


def random_path(T, A, rs, mean_run=3.0):
    """a path of runs of geometric length over symbols 0..A-1, blank (0) runs about every other run"""
    out = []
    while len(out) < T:
        s = 0 if (A == 1 or rs.rand() < 0.4) else int(rs.randint(1, A)) if A > 1 else 0
        out.extend([s] * int(rs.geometric(1.0 / mean_run)))
    return np.array(out[:T], dtype=np.int32)


def log_softmax_rows(T, A, dtype, rs):
    x = rs.randn(T, A) * 3.0
    x = x - x.max(axis=1, keepdims=True)
    return (x - np.log(np.exp(x).sum(axis=1, keepdims=True))).astype(dtype)


# ---- planted paths: name -> (best, drop); symbols assume A >= 10 ----

REF_DROP = (0, 1, 2, 8)     # ctc_fast.pyx:168-179 with blank 0


def edges(T):
    return [e for e in range(WAVE, T, WAVE)]


def planted_paths():
    T = 2 * FB + 90                         # 602 frames: nine wave edges, two of them block edges
    cases = {}
    # every edge e lies strictly inside a run: the runs change 5 frames after an edge
    b = np.zeros(T, dtype=np.int32)
    for i, start in enumerate([0] + [e + 5 for e in edges(T)]):
        b[start:] = 3 + i % 5               # 3..7: none dropped, neighbours differ
    cases["run_over_every_edge"] = (b, (0,))
    # a run ends on the frame in front of every edge: a new symbol starts on the edge itself
    b = np.zeros(T, dtype=np.int32)
    for i, start in enumerate([0] + edges(T)):
        b[start:] = 3 + i % 5
    cases["run_ends_on_every_edge"] = (b, (0,))
    cases["one_symbol"] = (np.full(2 * FB + 1, 5, dtype=np.int32), (0,))
    cases["new_symbol_every_frame"] = ((3 + np.arange(2 * FB + 1) % 4).astype(np.int32), (0,))
    cases["all_blank"] = (np.zeros(FB + 7, dtype=np.int32), (0,))
    cases["dropped_between_equal"] = (np.array([3, 0, 3, 3, 1, 3, 2, 3, 8, 3, 0, 0, 3, 4, 1, 1, 4], dtype=np.int32), REF_DROP)
    # a run that starts in the first block, outlives the second and ends on the last frame
    b = np.zeros(3 * FB + 9, dtype=np.int32)
    b[10:] = 6
    cases["long_run_to_last_frame"] = (b, (0,))
    # a dropped run that ends on the last frame, behind a label whose run ended two blocks earlier
    b = np.zeros(3 * FB + 9, dtype=np.int32)
    b[3:40] = 7
    cases["dropped_run_to_last_frame"] = (b, (0,))
    # the first frame is dropped, the first label starts exactly on a block edge
    b = np.zeros(FB + 3, dtype=np.int32)
    b[FB:] = 4
    cases["label_starts_on_block_edge"] = (b, (0,))
    return cases


def tie_rows(A, dtype):
    """rows with several equal maxima; the first wins.  With A > 64 the tied columns also lie on different
    lanes of the row-per-wave mapping (5 and 70 = lane 6), on one lane in different passes (5 and 69) and with
    the later column on the LOWER lane (70 and 128 = lane 0)"""
    cols = [(0, A - 1)] + ([(1, 2)] if A > 2 else [])
    if A > 129:
        cols += [(5, 70), (5, 69), (70, 128), (3, 67, 131)]
    elif A > 8:
        cols += [(5, 7), (2, A - 1), (4, 5, 6)]
    rows = np.full((len(cols) + 1, A), -2.0, dtype=dtype)
    for t, cs in enumerate(cols):
        rows[t, list(cs)] = -0.5
    rows[-1, :] = -1.0                      # every column equal
    want = np.array([min(cs) for cs in cols] + [0], dtype=np.int32)
    return rows, want


def neg_inf_rows(A, dtype):
    """rows of only -inf between ordinary rows: best 0, the score -inf"""
    rows = np.full((5, A), -np.inf, dtype=dtype)
    rows[1, A - 1] = -1.0
    rows[3, min(1, A - 1)] = -0.25
    return rows


# ---- sctc_log_rows ----

def log_rows(p):
    """float32: the float32 rounding of the float64 logarithm of float32 probabilities"""
    with np.errstate(divide="ignore"):
        return np.log(np.asarray(p, dtype=np.float32).astype(np.float64)).astype(np.float32)


def ulp_distance(a, b):
    """distance in float32 units in the last place between equal-shaped arrays; equal infinities are 0 apart"""
    a = np.asarray(a, dtype=np.float32)
    b = np.asarray(b, dtype=np.float32)

    def key(x):
        i = x.view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7fffffff), i)
    return np.abs(key(a) - key(b))
