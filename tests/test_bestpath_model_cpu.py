"""The NumPy statement of best-path decoding (tests/bestpath_model.py) against the two host loops it restates,
mutation checks that name the case that catches each mistake, and checks that the case tables of the GPU test
hold what their names say.  No GPU."""
import numpy as np
import pytest

from tests import bestpath_model as bm


@pytest.fixture(scope="module")
def ctc_fast():
    import __graft_entry__ as ge
    ge._paths()
    import ctc_fast
    return ctc_fast


def argmax_decoder_loop(best):
    """the loop of ArgmaxDecoder.decode (new_decoder/decoder.py, decoder.pyx:90-98) on symbol ids"""
    hyp, pm = [], -1
    for t in range(len(best)):
        if best[t] != pm:
            pm = best[t]
            if pm > 0:
                hyp.append(int(pm))
    return hyp


def paths_with_dropped_between(rs, n, A):
    out = []
    for _ in range(n):
        p = bm.random_path(int(rs.randint(1, 80)), A, rs, mean_run=2.0)
        for _ in range(4):      # x d x: a dropped symbol between two equal ones
            if len(p) >= 3:
                i = int(rs.randint(0, len(p) - 2))
                x = int(rs.randint(3, 8))
                p[i], p[i + 1], p[i + 2] = x, int(rs.choice([0, 1, 2, 8])), x
        out.append(p)
    return out


def test_model_equals_collapse_best_path(ctc_fast):
    rs = np.random.RandomState(0)
    seen_between = 0
    for blank in (0, 4, 11):
        for p in paths_with_dropped_between(rs, 60, 12):
            hyp, align = ctc_fast.collapse_best_path(p, blank)
            ids, spans = bm.collapse(p, (blank, 1, 2, 8))
            assert ids.tolist() == hyp and spans[:, 1].tolist() == align
            seen_between += sum(1 for i in range(len(p) - 2)
                                if p[i] == p[i + 2] and p[i] not in (blank, 1, 2, 8) and p[i + 1] in (1, 2, 8))
    assert seen_between > 50
    # the example of tests/test_abi.py
    ids, spans = bm.collapse(np.array([0, 3, 3, 0, 3, 1, 4, 4, 8, 5, 0, 5]), bm.REF_DROP)
    assert ids.tolist() == [3, 3, 4, 5, 5] and spans[:, 1].tolist() == [2, 4, 7, 9, 11]
    assert spans[:, 0].tolist() == [1, 4, 6, 9, 11]


def test_model_equals_argmax_decoder_loop():
    rs = np.random.RandomState(1)
    for _ in range(200):
        p = bm.random_path(int(rs.randint(0, 60)), int(rs.choice([1, 2, 6, 12])), rs, mean_run=2.0)
        assert bm.collapse(p, (0,))[0].tolist() == argmax_decoder_loop(p)


def test_argmax_and_score():
    rows = np.array([[-1.0, -0.5, -0.5], [-np.inf, -np.inf, -np.inf], [-3.0, -3.0, -2.0]])
    best, ids, spans, score = bm.decode(rows, ())
    assert best.tolist() == [1, 0, 2] and ids.tolist() == [1, 0, 2] and score == -np.inf
    best, ids, spans, score = bm.decode(rows[[0, 2]], (1,))
    assert ids.tolist() == [2] and spans.tolist() == [[1, 1]] and score == -2.5
    best, ids, spans, score = bm.decode(np.zeros((0, 4)), (0,))
    assert best.shape == (0,) and ids.shape == (0,) and spans.shape == (0, 2) and score == 0.0


# ---- mutants of the collapse, each caught by a named case of the table ----

def mutant_compare_last_emitted(best, drop):
    ids, last = [], None
    for b in best:
        if b in drop:
            continue
        if b != last:
            ids.append(int(b))
            last = b
    return ids


def mutant_frame0_silent(best, drop):
    return [int(b) for t, b in enumerate(best) if t > 0 and b != best[t - 1] and b not in drop]


def mutant_dropped_do_not_separate(best, drop):
    kept = [b for b in best if b not in drop]
    return [int(b) for t, b in enumerate(kept) if t == 0 or b != kept[t - 1]]


def test_mutants_are_caught():
    cases = bm.planted_paths()
    best, drop = cases["dropped_between_equal"]
    want = bm.collapse(best, drop)[0].tolist()
    assert want == [3, 3, 3, 3, 3, 3, 4, 4]
    assert mutant_compare_last_emitted(best, set(drop)) != want
    assert mutant_dropped_do_not_separate(best, set(drop)) != want
    best, drop = cases["one_symbol"]
    ids, spans = bm.collapse(best, drop)
    assert ids.tolist() == [5] and mutant_frame0_silent(best, set(drop)) == []
    # `last` taken as `first`
    assert spans.tolist() == [[0, len(best) - 1]] and spans[0, 1] != spans[0, 0]


# ---- the tables hold what they claim ----

def test_planted_paths_hold_what_they_claim():
    cases = bm.planted_paths()
    assert bm.FB == 256 and bm.WAVE == 64 and bm.FB % bm.WAVE == 0
    best, drop = cases["run_over_every_edge"]
    T = len(best)
    rr = bm.runs(best)
    assert len(bm.edges(T)) >= 9 and any(e % bm.FB == 0 for e in bm.edges(T))
    for e in bm.edges(T):
        assert any(f < e <= l and s not in drop for s, f, l in rr), e
    best, drop = cases["run_ends_on_every_edge"]
    rr = bm.runs(best)
    for e in bm.edges(len(best)):
        assert any(l == e - 1 and s not in drop for s, f, l in rr) and any(f == e for s, f, l in rr), e
    best, drop = cases["one_symbol"]
    ids, spans = bm.collapse(best, drop)
    assert len(best) > 2 * bm.FB and ids.shape == (1,) and spans.tolist() == [[0, len(best) - 1]]
    best, drop = cases["new_symbol_every_frame"]
    assert len(best) > 2 * bm.FB and bm.collapse(best, drop)[0].shape[0] == len(best)
    best, drop = cases["all_blank"]
    assert len(best) > bm.FB and bm.collapse(best, drop)[0].shape[0] == 0
    best, drop = cases["dropped_between_equal"]
    for d in (0, 1, 2, 8):
        assert any(best[i] == best[i + 2] == 3 and best[i + 1] == d for i in range(len(best) - 2)), d
    best, drop = cases["long_run_to_last_frame"]
    ids, spans = bm.collapse(best, drop)
    assert spans.tolist() == [[10, len(best) - 1]] and spans[0, 0] < bm.FB and spans[0, 1] >= 3 * bm.FB
    best, drop = cases["dropped_run_to_last_frame"]
    ids, spans = bm.collapse(best, drop)
    assert best[-1] in drop and spans.tolist() == [[3, 39]] and len(best) > 3 * bm.FB
    best, drop = cases["label_starts_on_block_edge"]
    ids, spans = bm.collapse(best, drop)
    assert best[0] in drop and spans.tolist() == [[bm.FB, len(best) - 1]]
    assert max(int(b.max()) for b, _ in cases.values()) < 10       # every table fits an alphabet of 10


@pytest.mark.parametrize("A", [1, 2, 10, 33, 65, 300])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_plant_and_special_rows(A, dtype):
    rs = np.random.RandomState(A)
    best = bm.random_path(100, A, rs)
    rows = bm.plant(best, A, dtype, rs)
    assert rows.dtype == dtype and np.array_equal(bm.argmax_rows(rows), best)
    assert np.array_equal(rows.astype(np.float64) * 1024, np.round(rows.astype(np.float64) * 1024))
    assert rows.min() >= -8 and rows.max() <= 0
    if A > 1:
        trows, want = bm.tie_rows(A, dtype)
        assert np.array_equal(bm.argmax_rows(trows), want)
        for r, w in zip(trows, want):
            assert (r == r[w]).sum() >= 2 and r.max() == r[w]       # a tie, and the first of it
        if A > 129:     # tied columns on different lanes of a row-per-wave scan, the later one on the lower lane
            tied = [np.nonzero(r == r.max())[0] for r in trows[:-1]]
            assert any(c[0] % 64 != c[1] % 64 for c in tied) and any(c[1] % 64 < c[0] % 64 for c in tied)
            assert any(c[0] % 64 == c[1] % 64 for c in tied)
    nrows = bm.neg_inf_rows(A, dtype)
    best, ids, spans, score = bm.decode(nrows, ())
    assert np.isneginf(nrows[0]).all() and best[0] == 0 and score == -np.inf


def test_sweeps_cover_the_edges():
    for t in (0, 1, 2, 63, 64, 65, 255, 256, 257, bm.FB - 1, bm.FB + 1, 2 * bm.FB + 1):
        assert t in bm.T_SWEEP
    for a in (1, 2, 33, 64, 65):
        assert a in bm.A_SWEEP
    assert bm.A_SWITCH == (bm.LANE_MAX_A, bm.LANE_MAX_A + 1)
    assert 0 in bm.T_SWITCH and 1 in bm.T_SWITCH and any(t > bm.FB for t in bm.T_SWITCH)
    assert any(bm.WAVE < t < bm.FB for t in bm.T_SWITCH)
    import _sctc
    assert (_sctc.BESTPATH_FRAMES_PER_BLOCK, _sctc.BESTPATH_LANE_MAX_A) == (bm.FB, bm.LANE_MAX_A)


def test_log_rows_model_and_ulp():
    p = np.array([0.0, 1e-45, 0.25, 1.0], dtype=np.float32)
    want = bm.log_rows(p)
    assert want.dtype == np.float32 and np.isneginf(want[0]) and want[3] == 0.0 and want[1] < -103
    a = np.array([1.0, -np.inf, -1.0], dtype=np.float32)
    b = np.array([np.nextafter(np.float32(1.0), np.float32(2.0)), -np.inf, np.nextafter(np.float32(-1.0), np.float32(0))],
                 dtype=np.float32)
    assert bm.ulp_distance(a, b).tolist() == [1, 0, 1]
