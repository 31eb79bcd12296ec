"""ctc_torch.mwer_loss / MWERLoss / mwer_nbest on the GPU against tests/mwer_model.py: the CPU float64 model on the same
input (rounded to float32 first for float32 runs).  PyTorch's device CTC loss is never called.

Shapes are the smallest at which each piece can go wrong: C = 5 (the prologue's row per lane), 33 (row per wave), 70
(a second column per lane in the combine kernel); K = 1, 2, 3, 8, and 256 once; N = 1..5 with ragged T_n in 2..40 and
ragged K_n; the lattice and the generic CTC path once each by natural dispatch.

float64 bounds.  Posterior, expected error and loss within relative 1e-12 of the plain model fed the device's own
log-likelihoods (the bound of tests/test_gpu_nbest_mbr.py for the same arithmetic); loss within 1e-10 relative + 1e-10
max|W| of the full oracle; gradient rtol 1e-7 / atol 1e-11 max(1, scale max|W|): the project's float64 CTC tolerances
(tests/test_gpu_ctc_torch.py) scaled by the factor the coefficients carry.

float32 bounds.  Measured on an MI355X over the seeded cases of this file (profiles/mwer.md): worst loss error of an
utterance 2.69e-8 max|W| (the loss is formed in float64 and rounded once), worst gradient ratio per utterance
|g - w| / (|w| + 5e-3 M) = 3.06e-7 with M = max(1, scale max|W|) -- the floor keeps the proportion of the project's
float32 CTC bound (2e-4 relative + 1e-6 absolute).  Asserted: 8 x those, the margin for
an exp() that differs by an ulp between compiler releases and so moves every probability; both stay inside the
project's float32 CTC bounds (loss 1e-4 relative + 1e-4 absolute, gradient norm 2e-4 relative + 1e-6, each times M),
which are asserted as well."""
import os
import subprocess

import numpy as np
import pytest
import torch

from tests import mwer_model as mm

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "stanford-ctc_amd", "csrc")
DTYPES = [torch.float64, torch.float32]
INF = float("inf")
F32_LOSS = 8 * 2.69e-8          # |loss - oracle| <= F32_LOSS * max|W|
F32_GRAD = 8 * 3.06e-7          # |g - w| <= F32_GRAD * (|w| + 5e-3 * M)
WORST = {"loss32": 0.0, "grad32": 0.0, "rel12": 0.0, "loss64": 0.0}


@pytest.fixture(scope="module")
def ct():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    import ctc_torch
    yield ctc_torch
    print("\nmwer worst figures: float32 loss error / max|W| %.3g, float32 gradient ratio %.3g; float64 stats against "
          "the plain model %.3g (relative), float64 loss against the oracle %.3g" %
          (WORST["loss32"], WORST["grad32"], WORST["rel12"], WORST["loss64"]))


# ---------------------------------------------------------------- cases

def labels(rs, U, C, repeats=True):
    """U labels in [1, C), now and then a repeat where the frames allow it (the caller leaves room)"""
    out = []
    for _ in range(U):
        k = int(rs.randint(1, C))
        while out and k == out[-1] and not (repeats and rs.rand() < 0.3):
            k = int(rs.randint(1, C))
        out.append(k)
    return out


def feasible(seq, T):
    return len(seq) + sum(a == b for a, b in zip(seq, seq[1:])) <= T


class Case(object):
    """hyps [N, K, S] with garbage (-1, C + 7) wherever the contract does not read"""

    def __init__(self, seed, T, N, K, C, logits, il=None, K_n=None, max_U=6, garbage=True):
        rs = np.random.RandomState(seed)
        self.T, self.N, self.K, self.C, self.logits = T, N, K, C, logits
        if il is None:
            il = [int(rs.randint(2, T + 1)) for _ in range(N)]
            il[N // 2] = T
        if K_n is None:
            K_n = [int(rs.randint(1, K + 1)) for _ in range(N)]
            K_n[N - 1] = K
        self.il, self.K_n = list(il), list(K_n)
        rows = [[None] * K for _ in range(N)]
        for n in range(N):
            for k in range(K):
                seq = labels(rs, int(rs.randint(1, max_U + 1)), C)
                while not feasible(seq, il[n]):
                    seq = seq[:-1]
                rows[n][k] = seq
        self.rows = rows
        self.W = rs.randint(0, 9, size=(N, K)).astype(np.float64)
        x = torch.from_numpy(rs.randn(T, N, C) * 1.5)
        self.x = x if logits else x.log_softmax(2)
        self.garbage = garbage
        self.pack()

    def pack(self):
        N, K = self.N, self.K
        S = max(1, max(len(s) for row in self.rows for s in row))
        self.S = S
        fill = -1 if self.garbage else 1
        hyps = np.full((N, K, S), fill, dtype=np.int64)
        U = np.zeros((N, K), dtype=np.int64)
        for n in range(N):
            for k in range(K):
                s = self.rows[n][k]
                hyps[n, k, :len(s)] = s
                U[n, k] = len(s)
                if self.garbage and k >= self.K_n[n]:
                    hyps[n, k] = self.C + 7
                    U[n, k] = -3
        self.hyps, self.U = hyps, U
        return self

    def max_w(self):
        w = self.W[np.isfinite(self.W)]
        return float(np.abs(w).max()) if w.size else 0.0


def rounded(case, dtype):
    return case.x.to(dtype)


def oracle(case, dtype, **kw):
    return mm.oracle(rounded(case, dtype).double(), case.hyps, case.U, case.W, case.il, case.K_n, logits=case.logits, **kw)


def run(ct, case, dtype, weight=None, x=None, **kw):
    """the loss on the device: (loss, gradient with respect to the input, stats)"""
    xd = (rounded(case, dtype).cuda() if x is None else x).detach().requires_grad_()
    loss, stats = ct.mwer_loss(xd, torch.from_numpy(case.hyps), torch.from_numpy(case.U), torch.from_numpy(case.W), case.il,
                               case.K_n, logits=case.logits, return_stats=True, **kw)
    (loss if weight is None else loss * weight.to(loss.dtype).cuda()).sum().backward()
    assert loss.dtype == dtype and xd.grad.dtype == dtype and xd.grad.shape == xd.shape
    assert not any(v.requires_grad for v in stats.values())
    return loss.detach(), xd.grad, stats


def rel(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape
    err = np.abs(got - want)
    with np.errstate(all="ignore"):
        r = np.where(err == 0, 0.0, err / np.abs(want))
    return float(r.max()) if r.size else 0.0


def check(ct, case, dtype, weight=None, dead=(), scale=1.0, reduction="none", subtract_mean=True):
    """device against the model; returns (loss, grad, stats)"""
    kw = dict(scale=scale, reduction=reduction, subtract_mean=subtract_mean)
    want_loss, want_grad, st = oracle(case, dtype, weight=weight, **kw)
    loss, grad, stats = run(ct, case, dtype, weight=weight, **kw)
    N, K, il = case.N, case.K, case.il
    M = max(1.0, scale * case.max_w())
    maxw = case.max_w()
    unit = maxw or 1.0
    real = stats["real"].cpu().numpy()
    assert real.dtype == np.bool_ and np.array_equal(real, st["real"])
    ll = stats["loglik"].cpu().numpy()
    assert np.array_equal(np.isfinite(ll), real) and (ll[~real] == -INF).all()
    # the coefficient kernel's arithmetic: the plain model fed the device's own log-likelihoods
    plain = mm.batch(ll, case.W, case.K_n, il, scale, subtract_mean)
    assert np.array_equal(plain["real"], real)
    figures = [rel(stats["posterior"].cpu().numpy(), plain["posterior"]), rel(stats["expected"].cpu().numpy(), plain["expected"])]
    if dtype == torch.float64:
        per_utt = loss if reduction == "none" else run(ct, case, dtype, scale=scale, subtract_mean=subtract_mean,
                                                        reduction="none")[0]
        figures.append(rel(per_utt.cpu().numpy(), plain["loss"]))
    WORST["rel12"] = max(WORST["rel12"], *figures)
    print("stats against the plain model, relative:", figures)
    assert max(figures) <= 1e-12
    # the whole thing: the oracle
    got, want = loss.double().cpu().reshape(-1).numpy(), want_loss.reshape(-1).numpy()
    err = float(np.abs(got - want).max()) if got.size else 0.0
    if dtype == torch.float64:
        WORST["loss64"] = max(WORST["loss64"], err / unit)
        print("float64 loss error / max|W|: %.3g" % (err / unit))
        assert (np.abs(got - want) <= 1e-10 * np.abs(want) + 1e-10 * maxw).all(), (got, want)
    else:
        if reduction == "none":
            WORST["loss32"] = max(WORST["loss32"], err / unit)
        print("float32 loss error / max|W|: %.3g" % (err / unit))
        assert (np.abs(got - want) <= 1e-4 * np.abs(want) + 1e-4 * M).all(), (got, want)       # the project's bound
        if reduction == "none":
            assert err <= F32_LOSS * maxw, (err, maxw)
    g, w = grad.detach().double().cpu(), want_grad
    assert g.shape == w.shape and torch.isfinite(g).all()
    for n in range(N):
        assert not g[il[n]:, n].any(), "padded frames of utterance %d" % n
        if n in dead:
            assert not g[:, n].any(), "utterance %d" % n
            continue
        gn, wn = g[:il[n], n], w[:il[n], n]
        assert not w[il[n]:, n].any()
        if dtype == torch.float64:
            np.testing.assert_allclose(gn.numpy(), wn.numpy(), rtol=1e-7, atol=1e-11 * M)
        else:
            d, nw = (gn - wn).norm().item(), wn.norm().item()
            floor = 5e-3 * M
            if nw + floor > 0:
                WORST["grad32"] = max(WORST["grad32"], d / (nw + floor))
                print("float32 gradient ratio, utterance %d: %.3g" % (n, d / (nw + floor)))
            assert d <= 2e-4 * nw + 1e-6 * M, (n, d, nw)         # the project's bound
            assert d <= F32_GRAD * (nw + floor), (n, d, nw)
    return loss, grad, stats


# ---------------------------------------------------------------- against the model

SHAPES = [  # T, N, K, C
    (9, 1, 1, 5), (12, 2, 2, 5), (40, 3, 3, 5), (23, 5, 8, 5),
    (17, 4, 2, 33), (40, 3, 8, 33), (11, 2, 3, 70), (31, 5, 8, 70), (8, 1, 3, 33),
]


@pytest.mark.parametrize("logits", [False, True])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "T%d-N%d-K%d-C%d" % s)
def test_against_the_model(ct, shape, dtype, logits):
    T, N, K, C = shape
    case = Case(sum(shape), T, N, K, C, logits)
    assert max(case.il) == T and min(case.il) >= 2 and max(case.K_n) == K
    rs = np.random.RandomState(1)
    weight = torch.from_numpy(rs.rand(N) + 0.5)             # grad_output per utterance
    loss, grad, stats = check(ct, case, dtype, weight=weight)
    if K == 1:
        assert not grad.any() and not loss.any()            # one hypothesis: P = 1, R = W = Wbar


@pytest.mark.parametrize("subtract_mean", [True, False])
@pytest.mark.parametrize("reduction", ["none", "sum", "mean"])
@pytest.mark.parametrize("scale", [0.5, 1.0, 5.0])
@pytest.mark.parametrize("dtype", DTYPES)
def test_reductions_scales_and_the_baseline(ct, dtype, scale, reduction, subtract_mean):
    case = Case(5, 14, 3, 4, 6, True)
    check(ct, case, dtype, scale=scale, reduction=reduction, subtract_mean=subtract_mean)


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_baseline_never_changes_the_gradient(ct, dtype):
    case = Case(6, 10, 2, 3, 7, False)
    with_mean = run(ct, case, dtype, reduction="none", subtract_mean=True)
    without = run(ct, case, dtype, reduction="none", subtract_mean=False)
    assert torch.equal(with_mean[1], without[1]) and not torch.equal(with_mean[0], without[0])
    assert torch.equal(without[0], without[2]["expected"].to(dtype))                    # return_stats: loss = R
    wbar = np.array([case.W[n, :case.K_n[n]].mean() for n in range(case.N)])
    np.testing.assert_allclose((without[0] - with_mean[0]).double().cpu().numpy(), wbar, rtol=1e-5)


@pytest.mark.parametrize("dtype", DTYPES)
def test_an_empty_hypothesis_and_equal_hypotheses_among_the_real_ones(ct, dtype):
    for logits in (False, True):
        case = Case(7, 12, 3, 4, 5, logits, K_n=[4, 4, 3])
        case.rows[0][1] = []                                # an all-blank hypothesis
        case.rows[1][0] = []
        case.rows[1][2] = list(case.rows[1][1])             # the same labels at two ranks
        case.rows[2][2] = []
        case.W[1, 1], case.W[1, 2] = 2.0, 5.0
        case.pack()
        loss, grad, stats = check(ct, case, dtype)
        ll, post = stats["loglik"].cpu().numpy(), stats["posterior"].cpu().numpy()
        assert ll[1, 1] == ll[1, 2] and post[1, 1] == post[1, 2]
        assert stats["real"].cpu().numpy().sum() == 11


# ---------------------------------------------------------------- exact identities

@pytest.mark.parametrize("dtype", DTYPES)
def test_exact_zeros(ct, dtype):
    for logits in (False, True):
        case = Case(8, 10, 3, 3, 33, logits)
        base = run(ct, case, dtype, reduction="none")
        assert base[1].any() and base[0].any()
        one = Case(8, 10, 3, 1, 33, logits)                 # K = 1
        loss, grad, _ = run(ct, one, dtype, reduction="none")
        assert not loss.any() and not grad.any()
        case.W[:] = 0.0                                     # errors all 0
        loss, grad, _ = run(ct, case, dtype, reduction="none")
        assert not loss.any() and not grad.any()
        case = Case(8, 10, 3, 3, 33, logits)
        loss, grad, stats = run(ct, case, dtype, reduction="none", scale=0.0)
        assert not grad.any()
        assert (loss.double().abs() <= 1e-12 * case.max_w()).all()
        post = stats["posterior"].cpu().numpy()
        for n in range(case.N):
            assert (post[n, :case.K_n[n]] == 1.0 / case.K_n[n]).all()


def excluded_case(logits, variant):
    """N = 5: utterance 0 is ordinary; 1 has one frame; 2 has no real rank; 3 has a rank beyond K_n, a rank with a
    non-finite error and two infeasible rows; 4 has an empty hypothesis whose blank is impossible in one frame, and one
    real rank beside it.  `variant` changes only what the contract does not read."""
    case = Case(9, 9, 5, 4, 6, logits, il=[9, 1, 6, 5, 7], K_n=[4, 4, 2, 3, 2])
    bad = [INF, float("nan")][variant]
    junk = [-1, 6 + 40][variant]
    case.W[2, 0] = bad
    case.rows[2][1] = [1, 2, 3, 4, 5, 1, 2]                 # more labels than its 6 frames
    case.W[3, 1] = -INF if variant else float("nan")
    case.rows[3][0] = [2, 2, 2, 2]                          # repeats without room in 5 frames
    case.rows[3][2] = [1, 2, 3, 4, 5, 4]                    # more labels than frames
    case.rows[4][0] = []
    case.rows[4][1] = [3]
    case.W[4, 1] = 2.0
    case.pack()
    case.hyps[1] = junk                                     # the one-frame utterance: nothing of it is read
    case.U[1] = -7 if variant else 99
    case.hyps[3, 1], case.U[3, 1] = junk, 50 + variant      # the rank with the non-finite error
    case.hyps[2, 0], case.U[2, 0] = junk, -1
    case.hyps[3, 3], case.U[3, 3] = junk, 1000              # beyond K_n
    if not logits:
        case.x[2, 4, 0] = -INF                              # the blank of utterance 4 in frame 2; label 3 carries it
        case.x[2, 4, 3] = 0.0
    return case


@pytest.mark.parametrize("dtype", DTYPES)
def test_what_is_excluded_contributes_nothing(ct, dtype):
    case = excluded_case(False, 0)
    loss, grad, stats = check(ct, case, dtype, dead=(1, 2, 3, 4))
    real = stats["real"].cpu().numpy()
    assert real.tolist() == [[True] * 4, [False] * 4, [False] * 4, [False] * 4, [False, True, False, False]]
    assert not loss[1:].any() and loss[0].item() != 0 and grad[:, 0].any()
    assert stats["loglik"][4, 0].item() == -INF and stats["expected"][4].item() == 2.0
    assert not stats["expected"][1:4].any() and not stats["posterior"][1:4].any()
    # what the contract does not read may hold anything: bit-equal
    other = run(ct, excluded_case(False, 1), dtype, reduction="none")
    assert torch.equal(loss, other[0]) and torch.equal(grad, other[1])
    for key in stats:
        assert torch.equal(stats[key], other[2][key]), key
    # utterance 3 with one real rank left
    case = excluded_case(True, 0)
    case.rows[3][0] = [2, 1, 2]
    case.pack()
    case.hyps[1], case.U[1] = -1, 99
    case.hyps[3, 1], case.hyps[3, 3] = -1, -1
    loss, grad, stats = check(ct, case, dtype, dead=(1, 2, 3))
    assert stats["real"].cpu().numpy()[3].tolist() == [True, False, False, False]
    assert stats["real"].cpu().numpy()[4].tolist() == [True, True, False, False] and grad[:, 4].any()


@pytest.mark.parametrize("logits", [False, True])
@pytest.mark.parametrize("dtype", DTYPES)
def test_strided_inputs_and_two_runs_are_bit_equal(ct, dtype, logits):
    for C in (5, 33, 70):
        case = Case(10 + C, 13, 4, 3, C, logits)
        base = check(ct, case, dtype)
        again = run(ct, case, dtype, reduction="none")
        assert torch.equal(base[0], again[0]) and torch.equal(base[1], again[1])
        x = rounded(case, dtype).cuda()
        T, N = case.T, case.N

        def view_run(view):
            assert view.shape == (T, N, C) and not view.is_contiguous() and torch.equal(view, x)
            out = run(ct, case, dtype, x=view, reduction="none")
            assert torch.equal(out[0], base[0]) and torch.equal(out[1], base[1])

        view_run(x.transpose(0, 1).contiguous().transpose(0, 1))            # an [N, T, C] tensor seen as [T, N, C]
        wide = torch.zeros(T, N, 2 * C + 1, dtype=dtype).cuda()
        wide[:, :, 1::2] = x
        view_run(wide[:, :, 1::2])                                          # stride_c == 2


def test_hypotheses_and_lengths_on_the_device_or_as_lists(ct):
    case = Case(11, 9, 2, 3, 5, True)
    base = run(ct, case, torch.float64, reduction="none")
    x = rounded(case, torch.float64).cuda().requires_grad_()
    loss = ct.mwer_loss(x, torch.from_numpy(case.hyps).cuda().to(torch.int32), torch.from_numpy(case.U).cuda(),
                        case.W.tolist(), torch.tensor(case.il).cuda(), torch.tensor(case.K_n, dtype=torch.int32),
                        logits=True, reduction="none")
    assert torch.equal(loss, base[0])
    with torch.no_grad():
        quiet = ct.mwer_loss(x, torch.from_numpy(case.hyps), case.U.tolist(), torch.from_numpy(case.W).float(), case.il,
                             case.K_n, logits=True, reduction="none")
    assert torch.equal(quiet, base[0]) and not quiet.requires_grad
    full = ct.mwer_loss(x.detach(), torch.from_numpy(np.where(case.hyps < 0, 1, case.hyps)[:, :1]), np.abs(case.U[:, :1]),
                        case.W[:, :1], case.il, logits=True)               # hyp_counts=None: K everywhere
    assert full.item() == 0.0 and not full.requires_grad


# ---------------------------------------------------------------- K = 256, and the other CTC paths

@pytest.mark.parametrize("dtype", DTYPES)
def test_256_hypotheses(ct, dtype):
    case = Case(12, 4, 1, 256, 5, True, max_U=2)
    case.rows[0][17] = []
    case.pack()
    assert case.K_n == [256]
    check(ct, case, dtype)


@pytest.fixture(scope="module")
def plan_query(tmp_path_factory):
    """the kernels csrc/ctc_plan.h names for a call, under this process's (unset) switches"""
    exe = str(tmp_path_factory.mktemp("ctc_plan") / "ctc_plan_dump")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", CSRC, os.path.join(ROOT, "tests", "ctc_plan_dump.cpp"), "-o", exe])

    def query(B, A, dtype, max_L, max_T):
        out = subprocess.run([exe, "query"], input="%d %d %d %d %d\n" % (B, A, 1 if dtype == torch.float64 else 0, max_L, max_T),
                             stdout=subprocess.PIPE, universal_newlines=True, check=True).stdout
        return [line.strip() for line in out.splitlines() if line.strip() != "end"]
    return query


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ["lattice", "generic"])
def test_the_other_ctc_paths(ct, plan_query, name, dtype):
    for k in os.environ:
        assert not k.startswith("SCTC_CTC_"), "natural dispatch: %s is set" % k
    ri = "double" if dtype == torch.float64 else "float"
    if name == "lattice":                                   # a hypothesis of 300 labels: 601 states
        case = Case(13, 620, 1, 2, 5, True, il=[620], K_n=[2])
        rs = np.random.RandomState(2)
        case.rows[0][0] = labels(rs, 300, 5, repeats=False)
        case.rows[0][1] = case.rows[0][0][:280] + labels(rs, 15, 5, repeats=False)
        case.W[0] = [3.0, 0.0]
        case.pack()
        # a flat posterior would leave one hypothesis with all the weight: the input is peaked on both label rows
        x = 0.3 * torch.from_numpy(rs.randn(620, 1, 5))
        for k, row in enumerate(case.rows[0]):
            for i, s in enumerate(row):
                x[2 * i + k, 0, s] += 1.0
        case.x = x
        want = "ctc_lattice_kernel<%s," % ri
        names = plan_query(2, 5, dtype, 2 * 300 + 1, 620)
    else:
        case = Case(14, 12, 2, 2, 300, True, il=[10, 12], K_n=[2, 2], max_U=3)
        want = "ctc_lattice_generic_kernel<%s>" % ri
        names = plan_query(4, 300, dtype, 2 * max(len(s) for row in case.rows for s in row) + 1, 12)
    assert names[0].startswith(want), (names, want)
    loss, grad, stats = check(ct, case, dtype)
    assert stats["real"].all() and grad.any()
    post = stats["posterior"].cpu().numpy()
    assert post.min() > 1e-6, post                          # every hypothesis carries weight: the sum is not one term


# ---------------------------------------------------------------- gradcheck, the module in a model

def test_gradcheck_in_both_modes(ct):
    rs = np.random.RandomState(15)
    T, N, K, C = 6, 2, 3, 4
    il, K_n = [6, 5], [3, 2]
    hyps = torch.tensor([[[1, 2], [3, 0], [2, 2]], [[1, 3], [2, 0], [-1, -1]]])
    U = torch.tensor([[2, 1, 2], [2, 1, 7]])
    W = torch.tensor([[1.0, 0.0, 3.0], [2.0, 1.0, INF]])
    base = torch.from_numpy(rs.randn(T, N, C))
    for logits in (True, False):
        # logits=False: raw log-probabilities, no log_softmax in the graph -- the perturbed rows do not sum to one
        x = (base if logits else base.log_softmax(2)).cuda().requires_grad_()
        for reduction in ("mean", "sum", "none"):
            for scale in (1.0, 2.5):
                assert torch.autograd.gradcheck(
                    lambda v: ct.mwer_loss(v, hyps, U, W, il, K_n, scale=scale, reduction=reduction, logits=logits), (x,),
                    eps=1e-6, atol=1e-6, rtol=1e-5)


def test_module_in_a_model_one_sgd_step(ct):
    rs = np.random.RandomState(16)
    T, N, D, C = 12, 3, 6, 5
    case = Case(16, T, N, 3, C, True)
    feats = torch.from_numpy(rs.randn(T, N, D))

    def model():
        torch.manual_seed(4)
        return torch.nn.Linear(D, C).double()

    for logits in (True, False):
        ref = model()
        opt = torch.optim.SGD(ref.parameters(), lr=0.1)
        out = ref(feats) if logits else ref(feats).log_softmax(2)
        _, grad, _ = mm.oracle(out.detach(), case.hyps, case.U, case.W, case.il, case.K_n, scale=2.0, logits=logits)
        out.backward(grad)
        opt.step()
        net = model().cuda()
        opt = torch.optim.SGD(net.parameters(), lr=0.1)
        crit = ct.MWERLoss(scale=2.0, logits=logits)
        out = net(feats.cuda())
        loss = crit(out if logits else out.log_softmax(2), torch.from_numpy(case.hyps), torch.from_numpy(case.U),
                    torch.from_numpy(case.W), case.il, case.K_n)
        assert loss.requires_grad and loss.dim() == 0
        loss.backward()
        opt.step()
        moved = False
        for got, want, start in zip(net.parameters(), ref.parameters(), model().parameters()):
            np.testing.assert_allclose(got.detach().cpu().numpy(), want.detach().numpy(), rtol=1e-7,
                                       atol=1e-11 * max(1.0, 2.0 * case.max_w()))
            moved = moved or not torch.equal(want.detach(), start.detach())
        assert moved


# ---------------------------------------------------------------- mwer_nbest

@pytest.mark.parametrize("unit", ["char", "word"])
def test_nbest_lists_from_the_beam_search(ct, unit):
    import ctc_fast
    from tests import beam_trace
    rs = np.random.RandomState(17)
    A, N, K, space = 8, 3, 4, 3
    il = [30, 22, 27]
    lps = [beam_trace.peaked(rs, A, t) for t in il]
    x = torch.full((30, N, A), -1.0, dtype=torch.float64)
    for n, lp in enumerate(lps):
        x[:il[n], n] = torch.from_numpy(lp.T)
    refs = [labels(rs, 7, A), labels(rs, 4, A), []]
    ref_t = torch.zeros(N, 7, dtype=torch.int64)
    for n, r in enumerate(refs):
        ref_t[n, :len(r)] = torch.tensor(r, dtype=torch.int64)
    hyps, lengths, counts, errors = ct.mwer_nbest(x.cuda(), il, ref_t, [7, 4, 0], K, beam=6, unit=unit, space=space)
    assert hyps.dtype == torch.int64 and hyps.shape[:2] == (N, K) and lengths.shape == (N, K) and counts.shape == (N,)
    assert errors.dtype == torch.float64 and not any(t.is_cuda for t in (hyps, lengths, counts, errors))
    by_hand, scores = ctc_fast.decode_beam_batch(lps, beam=6, nbest=K)
    for n in range(N):
        kept = [k for k in range(K) if scores[n, k] != -INF]
        assert counts[n].item() == len(kept) >= 1
        for i, k in enumerate(kept):
            h = [int(s) for s in by_hand[n][k]]
            assert lengths[n, i].item() == len(h) and hyps[n, i, :len(h)].tolist() == h
            a, b = np.array(refs[n], dtype=np.int32), np.array(h, dtype=np.int32)
            if unit == "char":
                want = ctc_fast.edit_distance_batch([a], [b])[0, 0]
            else:
                want = ctc_fast.word_errors_batch([a], [b], space, A=A)[0, 0]
            assert errors[n, i].item() == float(want)
    assert counts.max().item() > 1 and errors.max().item() > 0
    xd = x.cuda().requires_grad_()
    loss = ct.mwer_loss(xd, hyps, lengths, errors, il, counts)
    loss.backward()
    assert torch.isfinite(loss) and torch.isfinite(xd.grad).all() and xd.grad.any()
    # activations in place of log-probabilities: the search sees their log_softmax
    again = ct.mwer_nbest((x + 3.0).cuda(), il, ref_t, [7, 4, 0], K, beam=6, unit=unit, space=space, logits=True)
    assert again[0].shape[:2] == (N, K) and again[2].min().item() >= 1
    with pytest.raises(ValueError, match="blank"):
        ct.mwer_nbest(x.cuda(), il, ref_t, [7, 4, 0], K, unit=unit, space=space, blank=A - 1)
