"""sctc_ctc_loss_batch called the way ctc_fast never calls it (tests/ctc_entry_harness.py): padded rows, scattered
utterances, the BRNN engine's packed time-major minibatch (rowbase), junk around the labels, a workspace of exactly
sctc_ctc_workspace_bytes that is not fresh -- on every CTC path and both dtypes.

The batch: seven utterances that carry every special case in one launch -- [0] the one whose row width selects the
kernel instantiation (tests/test_gpu_ctc_paths._ROWS: T a little above U), [1] T = 1, [2] an empty band (T < U: cost
+inf, grad = probs), [3] one that skips (a zero column past the middle), [4] one label repeated throughout, [5] labels
equal to the blank, [6] an ordinary short one; [4] and [5] have the same length (a tie in the rank).

For every layout: (a) cost, skip and gradient BIT-equal to ctc_fast.ctc_loss_batch on the same batch under the same
path (the plan depends on (B, A, dtype, max_L, max_T) and the switches only, so a layout must not change a bit); (b)
against oracle.ctc.ctc_loss at the suite's standing bounds (cost 1e-11 relative; gradient 1e-9 absolute in float64,
2e-7 in float32 against the oracle on the float32-rounded inputs), so the file stands without (a); (c) no byte changed
outside the owned regions: probs (NaN in padding columns and gap rows) as sent, PATTERN in grad's padding columns and
gap rows, around cost[B], skip[B], the workspace and rowbase.

Worst |grad - oracle| observed on an MI355X, the same for every layout of a path (the layouts are bit-equal; each test
prints its own): float64 <= 1.2e-15 on every path; float32 fused / wide <= 5.9e-8, lattice / generic / lazy <= 3.0e-8.
Two defects were found by this file and corrected in csrc/: the wide fused kernel returned the cost of an utterance whose
zero band sum lies behind the middle only as far as alpha's first half ([3] of the batch: 92.48 where the oracle has
148.29), and the lazy schedule left out the band sums between the last rescaled frame and the dry one.
tests/test_ctc_plan_cpu.py checks off the GPU that ENTRY_ROWS reach every kernel family and each of NA = 1 / 2 / 4.

Sensitivity (a scratch build, not kept): with frame_row / the fused kernels' row tables taking rowbase[t] + row0 + 1
for the last frame of the shortest utterance, the rowbase layouts here fail (a) and (b) while tests/test_gpu_ctc.py and
tests/test_gpu_ctc_paths.py, which pass rowbase = NULL, do not notice; see DESIGN.md §5.
"""
import functools

import numpy as np
import pytest

from tests import ctc_entry_harness as eh
from tests.test_gpu_ctc_paths import _ROWS, _case, path

pytestmark = pytest.mark.gpu

# (path.ENV name, row width = key of _ROWS, alphabet, dtypes): alphabets 33 / 100 / 200 spread so that the fused, the
# wide and the lattice kernels each run with 1, 2 and 4 probability registers per frame
ENTRY_ROWS = [
    ("fused", 2, 33, "fd"), ("fused", 4, 100, "fd"), ("fused", 8, 200, "fd"), ("fused2w", 2, 100, "fd"), ("fused2wd", 2, 33, "f"),
    ("wide", 8, 33, "fd"), ("wide", 16, 100, "fd"), ("wide8", 8, 200, "fd"), ("wide8", 32, 33, "fd"), ("wide64", 16, 200, "f"),
    ("lattice", 2, 200, "fd"), ("lattice", 32, 33, "fd"), ("lattice4", 32, 100, "fd"), ("lattice8", 8, 200, "fd"),
    ("generic", 2, 33, "fd"), ("generic", 2, 300, "fd"), ("lazy", 2, 100, "f"), ("lazy", 16, 33, "f"),
]
B = 7
SHUFFLE = [3, 6, 0, 5, 2, 4, 1]
PLACE, GAPS = [4, 2, 6, 0, 5, 1, 3], [3, 0, 7, 1, 0, 5, 2]


def entry_cases():
    """(id, path, row, A, blank, numpy dtype): the blank id alternates between 0 and A - 1"""
    out = []
    for i, (which, row, A, dts) in enumerate(ENTRY_ROWS):
        for dt in dts:
            blank = 0 if (i + (dt == "d")) % 2 == 0 else A - 1
            out.append(("%s-r%d-A%d-b%d-%s" % (which, row, A, blank, "f64" if dt == "d" else "f32"), which, row, A, blank,
                        np.float64 if dt == "d" else np.float32))
    return out


CASES = entry_cases()
IDS = [c[0] for c in CASES]


def make_batch(row, A, blank, dt, seed=0, longer=0):
    U0, T0 = _ROWS[row]
    rs = np.random.RandomState(1000 * row + A + seed)
    utts = [_case(rs, A, T0 + longer, U0, blank=blank),
            _case(rs, A, 1, 1, blank=blank),
            _case(rs, A, 5, 9, blank=blank),                                  # empty band
            _case(rs, A, 40, 5, blank=blank),                                 # skips: a zero column past the middle
            _case(rs, A, 17, 6, blank=blank, all_same=True),
            _case(rs, A, 17, 7, blank=blank, with_blank_labels=True),
            _case(rs, A, 23, 9, blank=blank)]
    utts[3][0][:, 31] = 0.0
    utts[5][1][[1, 4]] = blank
    return [(np.asfortranarray(y.astype(dt)), seq) for y, seq in utts]


@functools.lru_cache(maxsize=None)
def _reference(which, row, A, blank, dt):
    """(batch, oracle results, the plain packed call's results) of a case, computed once"""
    import ctc_fast
    from oracle import ctc as octc
    batch = make_batch(row, A, blank, dt)
    with np.errstate(all="ignore"):
        refs = [octc.ctc_loss(np.asfortranarray(y.astype(np.float64)), seq, blank) for y, seq in batch]
        with path(which):
            plain = ctc_fast.ctc_loss_batch([y for y, _ in batch], [s for _, s in batch], blank)
    assert [bool(r[2]) for r in refs] == [False, False, False, True, False, False, False]
    assert np.isinf(refs[2][0]) and all(np.isfinite(refs[b][0]) for b in (0, 1, 4, 5, 6))
    return batch, refs, plain


def _check(tag, res, batch, refs, plain, dt):
    assert res["rc"] == 0, (tag, res["error"])
    assert res["untouched"] == [], (tag, res["untouched"])                    # (c)
    cost_p, grads_p, skip_p = plain
    worst = 0.0
    for b, ((y, seq), (c_ref, g_ref, s_ref)) in enumerate(zip(batch, refs)):
        # (a) bit for bit the plain packed call
        assert res["skip"][b] == skip_p[b] and res["skip_words"][b] in (0, 1), (tag, b)
        assert np.float64(res["cost"][b]).tobytes() == np.float64(cost_p[b]).tobytes(), (tag, b, res["cost"][b], cost_p[b])
        assert res["grads"][b].dtype == dt and res["grads"][b].tobytes() == np.asfortranarray(grads_p[b]).tobytes(), (tag, b)
        # (b) the oracle
        assert res["skip"][b] == bool(s_ref), (tag, b)
        g = res["grads"][b].astype(np.float64)
        if s_ref:
            assert not g.any(), (tag, b)
            assert abs(res["cost"][b] - c_ref) <= 1e-11 * abs(c_ref), (tag, b)
            continue
        if np.isinf(c_ref):
            assert np.isinf(res["cost"][b]) and res["cost"][b] > 0 and (res["grads"][b] == y).all(), (tag, b)
            continue
        assert abs(res["cost"][b] - c_ref) <= 1e-11 * abs(c_ref), (tag, b, res["cost"][b], c_ref)
        err = np.abs(g - g_ref).max()
        assert err < (1e-9 if dt == np.float64 else 2e-7), (tag, b, err)
        worst = max(worst, err)
    return worst


def _rank_order(batch):
    Ts = [y.shape[1] for y, _ in batch]
    return sorted(range(len(batch)), key=lambda u: (-Ts[u], u))


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_row_layouts(case):
    """padded rows (ld = A + 7 and round_up(A, 32) + 32), scattered utterances (frame_off in any order with NaN gap rows,
    label rows in another order with junk ids -7 and A + 5 around them), the packed time-major minibatch in rank order, in
    a shuffled batch order, and with the padded ld -- the BRNN engine's own call"""
    name, which, row, A, blank, dt = case
    batch, refs, plain = _reference(which, row, A, blank, dt)
    ld32 = (A + 31) // 32 * 32 + 32
    layouts = [("ld=A+7", dict(ld=A + 7)), ("ld=round32+32", dict(ld=ld32)),
               ("scattered", dict(place=PLACE, gaps=GAPS, label_junk=[-7, A + 5])),
               ("scattered, padded", dict(ld=A + 7, place=PLACE, gaps=GAPS, label_junk=[-7, A + 5], order=SHUFFLE)),
               ("rowbase, rank order", dict(rowbase=True, order=_rank_order(batch))),
               ("rowbase, shuffled order", dict(rowbase=True, order=SHUFFLE, label_junk=[-7, A + 5])),
               ("rowbase, rank order, padded: the engine's call", dict(rowbase=True, order=_rank_order(batch), ld=ld32))]
    worst = 0.0
    with path(which), np.errstate(all="ignore"):
        for lname, kw in layouts:
            worst = max(worst, _check((name, lname), eh.call(batch, blank, **kw), batch, refs, plain, dt))
    print("%s: worst |grad - oracle| %.1e over %d layouts" % (name, worst, len(layouts)))


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_workspace_reuse(case):
    """a workspace of exactly sctc_ctc_workspace_bytes that is not fresh: all zero bytes, all 0xFF, and what another
    batch of the same shapes (one row longer: the same plan, a larger workspace) left in it -- for the wide kernel the flag
    words of its two workgroups' meetings among it, which the launcher clears.  All three bit-equal to the plain call."""
    name, which, row, A, blank, dt = case
    batch, refs, plain = _reference(which, row, A, blank, dt)
    other = make_batch(row, A, blank, dt, seed=7, longer=8)
    with path(which), np.errstate(all="ignore"):
        assert eh.workspace_bytes(other, blank) >= eh.workspace_bytes(batch, blank) > 0
        for fill in (0x00, 0xFF, "leftover"):
            _check((name, "workspace", fill), eh.call(batch, blank, workspace_fill=fill, leftover=other), batch, refs, plain, dt)


@pytest.mark.parametrize("which,row,A,dt", [("fused", 2, 33, np.float32), ("fused", 8, 100, np.float64), ("wide", 16, 33, np.float32),
                                            ("lattice", 32, 200, np.float64), ("generic", 2, 300, np.float32),
                                            ("lazy", 16, 100, np.float32)])
def test_rowbase_with_one_utterance(which, row, A, dt):
    """B = 1: rowbase[t] = t, frame_off = 0 -- the engine's single-utterance step"""
    import ctc_fast
    from oracle import ctc as octc
    batch = make_batch(row, A, 0, dt)[:1]
    (y, seq), = batch
    with path(which), np.errstate(all="ignore"):
        plain = ctc_fast.ctc_loss_batch([y], [seq], 0)
        refs = [octc.ctc_loss(np.asfortranarray(y.astype(np.float64)), seq, 0)]
        _check((which, row, "B=1"), eh.call(batch, 0, rowbase=True, ld=A + 7), batch, refs, plain, dt)


@pytest.mark.parametrize("which", ["fused", "wide", "lattice", "generic"])
def test_short_workspace_is_refused_and_nothing_is_written(which):
    """256 bytes less than sctc_ctc_workspace_bytes: SCTC_ERR_WORKSPACE, and no byte of grad, cost, skip or the workspace
    changes (tests/test_abi.py has the return code off the GPU)"""
    batch = make_batch(8, 33, 0, np.float32)
    with path(which):
        res = eh.call(batch, 0, ld=40, ws_short=256)
    assert res["rc"] == -3 and b"workspace" in res["error"], (res["rc"], res["error"])
    assert res["untouched"] == [], res["untouched"]
