"""SCTC_CTC_LAZY=1 ("switches") on the GPU: ctc_lattice_kernel<float, K, NA, W, true>, which rescales
a float32 batch's rows every 4th frame only, and the p.lazy branch of ctc_grad_kernel, which brings both rows to unit
magnitude by a power of two before it multiplies them.  All through ctc_fast.ctc_loss_batch on float32 probabilities
under path("lazy") / "lazy1" / "lazy4" / "lazy8" (tests/test_ctc_plan_cpu.py checks off the GPU that LAZY_SHAPES reach
every (K, W) of ctc_lattice_shape with the lazy schedule, and each NA); the oracle runs on the float32-rounded inputs.

 (a) every shape of test_gpu_ctc_paths.SHAPES once, the 513..2047-state edges and the forced shapes against the oracle:
     gradient 2e-7, cost 1e-11 relative -- the bound of every other path, which the kernel's comment ("the same number")
     claims and which holds: observed on an MI355X: cost <= 1.4e-15 relative, gradient <= 3.0e-8 (53 shapes);
 (b) the schedule's tails: T = 1..13 at U = 1, 2, 3 over one and two distinct labels, T = 4k - 1, 4k, 4k + 1 around the
     prefetch blocks, alone and in ragged batches;
 (c) skip, empty band and zero columns: the ctc_skip.npz / ctc_tiny.npz fixtures rounded to float32, and a zero column
     at every t % 4: skip, an all-zero gradient, and the cost -llForward as far as alpha got;
 (d) extreme magnitudes: peaked inputs and four consecutive frames of float32 denormals (1e-45) against the oracle and
     tests/ctc_exact_model.py, then the input on which the reference's overlap is 0 or a denormal in most frames
     (T = 8000, U = 800), with the distance to the exact models printed for the lazy and the default schedule;
 (f) through the network: NNet.costAndGradBatch with and without the switch.
((e), the row layouts and stale workspaces, is in tests/test_gpu_ctc_entry.py: its "lazy" rows.)
"""
import numpy as np
import pytest

from tests.test_gpu_ctc_paths import _ROWS, SHAPES, _case, path

pytestmark = pytest.mark.gpu

EDGES = [(33, 1100, 511), (33, 1300, 512), (33, 1100, 1023), (3, 1700, 800)]
# (path.ENV name, (A, T, U)): (a)'s cases; the forced shapes take the rows and alphabets the bit-pinned lattice1 / 4 / 8
# cases take (test_gpu_ctc_paths._BITS_PATHS)
LAZY_SHAPES = ([("lazy", s) for s in SHAPES + EDGES]
               + [("lazy1", (A, _ROWS[r][1], _ROWS[r][0])) for r in (8, 16, 32) for A in (33, 100, 200)]
               + [("lazy4", (A, _ROWS[32][1], _ROWS[32][0])) for A in (33, 100, 200)]
               + [("lazy8", (A, _ROWS[8][1], _ROWS[8][0])) for A in (33, 100, 200)]
               + [("lazy", (A, _ROWS[r][1], _ROWS[r][0])) for r in (2, 4, 16) for A in (100, 200)])


@pytest.fixture(scope="module")
def mods():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    import ctc_fast
    from oracle import ctc as octc
    return ctc_fast, octc


def _f32(y):
    return np.asfortranarray(y.astype(np.float32))


def _oracle(octc, y32, seq, blank=0):
    with np.errstate(all="ignore"):
        return octc.ctc_loss(np.asfortranarray(y32.astype(np.float64)), seq, blank)


def _check(tag, got, ref, y32):
    """one utterance against the oracle at the standing bounds; returns (relative cost error, gradient error)"""
    cost, grad, skip = got
    c_ref, g_ref, s_ref = ref
    assert bool(skip) == bool(s_ref), (tag, skip, s_ref)
    if s_ref:
        assert not grad.any(), tag
        assert abs(cost - c_ref) <= 1e-11 * abs(c_ref), (tag, cost, c_ref)     # -llForward as far as alpha got
        return 0.0, 0.0
    if np.isinf(c_ref):
        assert np.isinf(cost) and cost > 0 and (grad == y32).all(), (tag, cost)
        return 0.0, 0.0
    ec = abs(cost - c_ref) / max(abs(c_ref), 1e-30)
    assert ec <= 1e-11, (tag, cost, c_ref)
    eg = np.abs(grad.astype(np.float64) - g_ref).max()
    assert eg < 2e-7, (tag, eg)
    return ec, eg


def _run(cf, which, ys, seqs, blank=0):
    with path(which), np.errstate(all="ignore"):
        cost, grads, skip = cf.ctc_loss_batch(ys, seqs, blank)
    assert all(g.dtype == np.float32 for g in grads)
    return [(cost[b], grads[b], skip[b]) for b in range(len(ys))]


@pytest.mark.parametrize("which", ["lazy", "lazy1", "lazy4", "lazy8"])
def test_lazy_against_the_oracle(mods, which):
    cf, octc = mods
    rs = np.random.RandomState(31)
    worst_c = worst_g = 0.0
    mine = [s for w, s in LAZY_SHAPES if w == which]
    for i, (A, T, U) in enumerate(mine):
        blank = 0 if i % 2 == 0 else A - 1
        y, seq = _case(rs, A, T, U, blank=blank, with_blank_labels=(i % 5 == 4))
        y32 = _f32(y)
        (got,) = _run(cf, which, [y32], [seq], blank)
        ec, eg = _check((which, A, T, U, blank), got, _oracle(octc, y32, seq, blank), y32)
        worst_c, worst_g = max(worst_c, ec), max(worst_g, eg)
    print("%s: %d shapes, worst cost error %.1e relative, worst |grad - oracle| %.1e" % (which, len(mine), worst_c, worst_g))


def test_lazy_tails_of_the_every_fourth_frame_schedule(mods):
    cf, octc = mods
    rs = np.random.RandomState(37)
    cases = []
    for A in (2, 3):                                    # one and two distinct labels (blank 0)
        for U in (1, 2, 3):
            for T in range(1, 14):
                cases.append((A, T, U))
    small = [(7, 3), (9, 4), (33, 6), (33, 8), (33, 15)]      # (A, U) of SHAPES' small rows
    for A, U in small:
        for T in (7, 8, 9, 15, 16, 17, 31, 32, 33, 34, 63, 64, 65, 66):
            cases.append((A, T, U))
    by_A, worst = {}, 0.0
    for A, T, U in cases:
        y, seq = _case(rs, A, T, U)
        y32 = _f32(y)
        ref = _oracle(octc, y32, seq)
        (got,) = _run(cf, "lazy", [y32], [seq])
        worst = max(worst, _check((A, T, U), got, ref, y32)[1])
        by_A.setdefault(A, []).append((y32, seq, ref))
    # ragged batches mixing them: all of an alphabet in one launch, in the order given and reversed
    for A, utts in by_A.items():
        for sel in (utts, utts[::-1], utts[::3]):
            got = _run(cf, "lazy", [u[0] for u in sel], [u[1] for u in sel])
            for b, (y32, seq, ref) in enumerate(sel):
                worst = max(worst, _check((A, "batch", b, y32.shape, len(seq)), got[b], ref, y32)[1])
    print("lazy tails: %d utterances, worst |grad - oracle| %.1e" % (len(cases), worst))


def test_lazy_skip_empty_band_and_zero_columns(mods, golden):
    cf, octc = mods
    g = golden("ctc_skip.npz")
    t = golden("ctc_tiny.npz")
    fix = [(g["rep_y_T%d" % T], g["rep_seq"]) for T in (4, 5, 6, 7, 8)]
    fix += [(g["zero_y"], g["zero_seq"]), (g["short_y"], g["short_seq"])]
    fix += [(t["y%d" % i], t["seq%d" % i]) for i in range(int(t["n"]))]
    kinds = set()
    for i, (y, seq) in enumerate(fix):
        y32, seq = _f32(y), np.ascontiguousarray(seq, dtype=np.int32)
        ref = _oracle(octc, y32, seq)
        kinds.add("skip" if ref[2] else ("empty" if np.isinf(ref[0]) else "plain"))
        (got,) = _run(cf, "lazy", [y32], [seq])
        _check(("fixture", i), got, ref, y32)
    assert kinds == {"skip", "empty", "plain"}
    # a zero column at every t % 4, early, in the middle, and in the last frames; alone and all in one batch
    rs = np.random.RandomState(5)
    T, U, A = 41, 5, 6
    utts = []
    for col in (1, 2, 3, 4, 5, 6, 7, 20, 21, 22, 23, 36, 37, 38, 39, 40):
        y, seq = _case(rs, A, T, U)
        y[:, col] = 0.0
        y32 = _f32(y)
        ref = _oracle(octc, y32, seq)
        assert ref[2] and ref[0] > 0, col
        (got,) = _run(cf, "lazy", [y32], [seq])
        _check(("zero column", col), got, ref, y32)
        utts.append((y32, seq, ref))
    got = _run(cf, "lazy", [u[0] for u in utts], [u[1] for u in utts])
    for b, (y32, seq, ref) in enumerate(utts):
        _check(("zero columns, batch", b), got[b], ref, y32)


def test_lazy_extreme_magnitudes(mods):
    """peaked inputs (peaked = 6) and rows in which every symbol on the label path has the float32 denormal probability
    1e-45 for four consecutive frames (the unscaled float64 steps between two rescalings reach 1e-180: what the scalbn
    branch of ctc_grad_kernel exists for), in every position relative to the rescaled frames: the oracle's bounds, and
    2e-7 against the exact model on every frame whose overlap is sound (all of them here)"""
    cf, octc = mods
    from tests import ctc_exact_model as em
    rs = np.random.RandomState(43)
    cases = []
    for A, T, U in ((28, 200, 30), (33, 333, 63), (62, 300, 100), (33, 260, 127)):
        y, seq = _case(rs, A, T, U, peaked=6.0)
        cases.append(("peaked", _f32(y), seq))
    for first in (8, 9, 10, 11):
        y, seq = _case(rs, 12, 40, 5)
        on_path = np.unique(np.concatenate([[0], seq]))
        off_path = np.setdiff1d(np.arange(12), on_path)
        assert off_path.size > 0
        y32 = _f32(y)
        y32[:, first:first + 4][on_path] = np.float32(1e-45)
        assert y32[on_path[0], first] > 0 and y32[on_path[0], first] < 1.2e-38          # a float32 denormal
        cases.append(("1e-45 from frame %d" % first, np.asfortranarray(y32), seq))
    worst_o = worst_m = 0.0
    for name, y32, seq in cases:
        y64 = np.asfortranarray(y32.astype(np.float64))
        ref = _oracle(octc, y32, seq)
        assert not ref[2] and np.isfinite(ref[0])
        assert em.reference_overlap(y64, seq).min() > 1e-290, name
        c_m, g_m, s_m = em.exact(y64, seq, rows="element")
        for which in ("lazy", "lattice"):
            (got,) = _run(cf, which, [y32], [seq])
            worst_o = max(worst_o, _check((name, which), got, ref, y32)[1])
            assert abs(got[0] - c_m) <= 1e-11 * abs(c_m), (name, which)
            err = np.abs(got[1].astype(np.float64) - g_m).max()
            assert err < 2e-7, (name, which, err)
            worst_m = max(worst_m, err)
    print("extreme magnitudes: worst |grad - oracle| %.1e, |grad - exact model| %.1e" % (worst_o, worst_m))


def test_lazy_where_the_references_overlap_is_denormal(mods):
    """tests/test_ctc_store_model.inputs(8000, 800, 33, 12): the reference's overlap is 0 or a denormal in 6538 of the
    8000 frames (tests/test_ctc_exact_model_cpu.py).  Sound frames: 2e-7 against the oracle and against the exact model
    with the reference's rows.  Unsound frames: every value finite, and a gradient column either equals the probability
    column exactly or sums to zero (to sum(y) - 1) within 1e-6, the two outcomes of ctc_fast.pyx:141-145 -- with one
    correction to the issue that set this check: the oracle ITSELF has a third outcome (21 frames here, columns that sum to
    up to 0.167), where the products are nonzero denormals and sum_k g[k] / y[k] no longer equals Z.  So the third outcome
    is admitted exactly where a product of two rescaled rows can be a nonzero denormal: the exact model gives log2 of the
    overlap of the two rows scaled to a largest element in [0.5, 1); a kernel's rows are scaled to a largest element in
    [1, 2) (lazy: ilogb) or to the sum 1 (default: largest element in [1 / L, 1]), so its overlap is that times 2^-23 .. 2^2
    (L = 1601), and the sum of L products, each below 2^-1075, is 0: below 2^-1112 the column must equal y, above 2^-997
    the overlap is a normal number and the column must sum to zero, in between all three outcomes are admitted.

    Observed on an MI355X (cost; worst / mean |grad - model| over the unsound frames; columns of the 6538):
      lazy     25397.206771   row model 1.0 / 0.14   element model 1.0 / 0.65   6462 equal y, 24 the third outcome (sum <= 0.15)
      lattice  25392.863410   row model 1.0 / 0.14   element model 1.0 / 0.65   6464 equal y, 21 the third outcome (sum <= 0.17)
    (the oracle's cost is 25392.863410 -- the default schedule reproduces the oracle, noise included, to 3e-8 in EVERY
    frame -- the row model's 25392.641568, the likelihood's 25186.541044); sound frames: both 3.1e-8 against either.
    The lazy schedule is no closer to either model than the default one in the unsound frames: it brings the ROWS to unit
    magnitude, not their overlap, and the states that carry the overlap lie 2^-500 below each row's largest.  The sentence
    "no underflow of the forward-backward overlap" in csrc/ctc_kernels.hip and INTEGRATION.md was corrected accordingly.
    The costs differ by 4e-4 relative on this input, where the paths at the flush threshold carry the likelihood."""
    cf, octc = mods
    from tests import ctc_exact_model as em
    from tests import test_ctc_store_model as store_model
    y, seq = store_model.inputs(8000, 800, 33, 12)
    y32 = _f32(y)
    assert (y32.astype(np.float64) == y).all()
    c_ref, g_ref, s_ref = _oracle(octc, y32, seq)
    overlap = em.reference_overlap(y, seq)
    sound = overlap >= 2.2250738585072014e-308
    assert not s_ref and 20 <= (~sound).sum() < 8000 - 1000
    c_row, g_row, _, mag = em.exact(y, seq, rows="row", overlap_log2=True)
    c_el, g_el, _ = em.exact(y, seq, rows="element")
    surely_zero, surely_normal = mag < -1112, mag > -997
    assert (surely_zero & ~sound).sum() > 1000 and not (surely_zero & sound).any()     # (157 frames lie in between)
    colsum_y = y.sum(axis=0)
    for which in ("lazy", "lattice"):
        (got,) = _run(cf, which, [y32], [seq])
        cost, grad, skip = got
        g = grad.astype(np.float64)
        e_or = np.abs(g - g_ref).max(axis=0)
        e_row = np.abs(g - g_row).max(axis=0)
        e_el = np.abs(g - g_el).max(axis=0)
        is_y = (grad == y32).all(axis=0)
        col = np.abs(g.sum(axis=0) - (colsum_y - 1.0))
        third = ~sound & ~is_y & (col >= 1e-6)
        print("%s: cost %.6f (oracle %.6f, row model %.6f, element model %.6f); sound frames (%d): |grad - oracle| %.1e, "
              "|grad - row model| %.1e; unsound frames (%d): |grad - oracle| %.1e, |grad - row model| %.1e (mean %.1e), "
              "|grad - element model| %.1e (mean %.1e), %d columns equal y, %d neither y nor a zero sum (worst sum %.1e)"
              % (which, cost, c_ref, c_row, c_el, sound.sum(), e_or[sound].max(), e_row[sound].max(), (~sound).sum(),
                 e_or[~sound].max(), e_row[~sound].max(), e_row[~sound].mean(), e_el[~sound].max(), e_el[~sound].mean(),
                 is_y[~sound].sum(), third.sum(), col[third].max() if third.any() else 0.0))
        assert not skip and np.isfinite(cost) and np.isfinite(grad).all(), which
        assert e_or[sound].max() < 2e-7, (which, e_or[sound].max())
        assert e_row[sound].max() < 2e-7, (which, e_row[sound].max())
        assert is_y[surely_zero].all(), which
        assert (col[surely_normal] < 1e-6).all(), which
        assert not (third & (surely_zero | surely_normal)).any(), (which, third.sum())


def test_lazy_through_the_network(mods):
    """NNet.costAndGradBatch on a small network, twelve ragged utterances: SCTC_CTC_LAZY=1 reaches the engine's CTC call
    (the packed time-major minibatch, ld padded) -- costs equal to 1e-9 relative, the flat gradient within 1e-5 in
    relative norm of the default schedule's and not bit-equal to it"""
    cf, octc = mods
    from nnets import brnnet
    D, A, H, NL, TL, B = 8, 20, 32, 2, 1, 12
    rs = np.random.RandomState(14)
    Ts = [int(rs.randint(20, 121)) for _ in range(B)]
    Us = [int(rs.randint(1, max(2, t // 3))) for t in Ts]
    datas = [rs.randn(D, t) for t in Ts]
    labs = [rs.randint(1, A, size=u).astype(np.int32) for u in Us]
    np.random.seed(3)
    net = brnnet.NNet(D, A, H, NL, max(Ts), temporalLayer=TL, maxUtts=B)
    net.initParams()
    res = {}
    for which in ("fused", "lazy"):                 # "fused": no switch set
        with path(which):
            costs, _, skips = net.costAndGradBatch(datas, labs)
        assert not skips.any()
        res[which] = (costs.copy(), net.grad.flat.clone())
    np.testing.assert_allclose(res["lazy"][0], res["fused"][0], rtol=1e-9)
    d = float((res["lazy"][1] - res["fused"][1]).double().norm() / res["fused"][1].double().norm())
    print("through the network: relative distance of the flat gradients %.1e" % d)
    assert d < 1e-5, d
    assert d > 0, "both runs took the same kernels?"
