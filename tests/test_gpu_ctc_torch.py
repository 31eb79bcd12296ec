"""ctc_torch.ctc_loss / CTCLoss on the GPU against torch.nn.functional.ctc_loss on CPU tensors in float64, fed the
log_softmax of the same activations (logits=True) or the same log-probabilities (logits=False).  For float32 runs
the input is rounded to float32 and then widened for the oracle.  PyTorch's device CTC loss is never called.

Tolerances are the project's own (tests/test_gpu_ctc.py): float64 loss 1e-10 relative, gradient rtol 1e-7 / atol
1e-11; float32 loss 1e-4 relative + 1e-4 absolute, gradient norm 2e-4 relative + 1e-6.

The padded, unsorted [T, N, C] layout (rowbase[t] = t * N, frame_off[n] = n) is new ground for all four CTC paths:
test_padded_layout_through_each_path drives each by natural dispatch and asserts the path with the plan header's own
answer (tests/ctc_plan_dump.cpp, `query`)."""
import os
import subprocess

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "stanford-ctc_amd", "csrc")
DTYPES = [torch.float64, torch.float32]
INF = float("inf")


@pytest.fixture(scope="module")
def ct():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    import ctc_torch
    return ctc_torch


# ---------------------------------------------------------------- the oracle and the comparison

def oracle(x64, targets, il, tl, blank=0, reduction="mean", zero_infinity=False, logits=False, weight=None):
    """PyTorch's CPU float64 loss and its gradient with respect to x64 (activations through log_softmax when
    `logits`, else the log-probabilities themselves: PyTorch's native backward)"""
    x = x64.detach().clone().requires_grad_()
    lp = x.log_softmax(2) if logits else x
    loss = F.ctc_loss(lp, targets.cpu() if isinstance(targets, torch.Tensor) else targets, torch.as_tensor(il).cpu(),
                      torch.as_tensor(tl).cpu(), blank=blank, reduction=reduction, zero_infinity=zero_infinity)
    (loss if weight is None else loss * weight).sum().backward()
    return loss.detach(), x.grad


def make_input(rs, T, N, C, logits, dtype, scale=1.0):
    """CPU tensor of `dtype`: activations, or their float64 log_softmax rounded to dtype"""
    x = torch.from_numpy(rs.randn(T, N, C) * scale)
    return (x if logits else x.log_softmax(2)).to(dtype)


def labels_without_repeats(rs, U, C, blank=0):
    """U labels, none equal to the blank or to its predecessor: feasible from T = U frames on"""
    pool = [k for k in range(C) if k != blank]
    out = []
    for _ in range(U):
        k = pool[rs.randint(len(pool))]
        while out and k == out[-1] and len(pool) > 1:
            k = pool[rs.randint(len(pool))]
        out.append(k)
    return out


def padded(seqs, fill=0):
    S = max(1, max(len(s) for s in seqs))
    return torch.tensor([list(s) + [fill] * (S - len(s)) for s in seqs], dtype=torch.int64)


def assert_loss(got, want, dtype):
    got, want = got.detach().double().cpu().reshape(-1), want.double().reshape(-1)
    assert got.shape == want.shape
    for g, w in zip(got.tolist(), want.tolist()):
        if np.isinf(w):
            assert g == w, (g, w)
        elif dtype == torch.float64:
            assert g == pytest.approx(w, rel=1e-10), (g, w)
        else:
            assert g == pytest.approx(w, rel=1e-4, abs=1e-4), (g, w)


def assert_grad(got, want, dtype, il, dead=()):
    """utterance by utterance; exact zeros in padded frames and in the utterances of `dead` (where the oracle holds
    NaN or zeros)"""
    got = got.detach().double().cpu()
    assert got.shape == want.shape and torch.isfinite(got).all()
    for n, T_n in enumerate(il):
        T_n = int(T_n)
        assert not got[T_n:, n].any(), "padded frames of utterance %d" % n
        if n in dead:
            assert not got[:, n].any(), "infeasible utterance %d" % n
            continue
        g, w = got[:T_n, n], want[:T_n, n]
        assert not want[T_n:, n].any()
        if dtype == torch.float64:
            np.testing.assert_allclose(g.numpy(), w.numpy(), rtol=1e-7, atol=1e-11)
        else:
            assert (g - w).norm().item() <= 2e-4 * w.norm().item() + 1e-6, (n, (g - w).norm().item(), w.norm().item())


def run(ct, x, targets, il, tl, weight=None, **kw):
    """the loss on the device; returns (loss, gradient with respect to the input)"""
    xd = x.cuda().requires_grad_()
    loss = ct.ctc_loss(xd, targets, il, tl, **kw)
    (loss if weight is None else loss * weight.to(loss.dtype).cuda()).sum().backward()
    assert loss.dtype == x.dtype and xd.grad.dtype == x.dtype and xd.grad.shape == x.shape
    return loss, xd.grad


def check(ct, x, targets, il, tl, dead=(), weight=None, **kw):
    want_loss, want_grad = oracle(x.double(), targets, il, tl, weight=weight, **kw)
    loss, grad = run(ct, x, targets, il, tl, weight=weight, **kw)
    assert_loss(loss, want_loss, x.dtype)
    assert_grad(grad, want_grad, x.dtype, il, dead)
    return loss, grad


# ---------------------------------------------------------------- the small ragged batch

SMALL_T, SMALL_N, SMALL_C = 7, 3, 5
SMALL_IL, SMALL_TL = (7, 4, 3), (3, 1, 3)
SMALL_TARGETS = [[1, 2, 2], [3], [4, 4, 4]]      # the third is infeasible: T = 3 < U + repeats = 5


@pytest.mark.parametrize("zero_infinity", [False, True])
@pytest.mark.parametrize("reduction", ["none", "sum", "mean"])
@pytest.mark.parametrize("logits", [False, True])
@pytest.mark.parametrize("dtype", DTYPES)
def test_small_ragged_batch(ct, dtype, logits, reduction, zero_infinity):
    x = make_input(np.random.RandomState(0), SMALL_T, SMALL_N, SMALL_C, logits, dtype)
    tg = padded(SMALL_TARGETS)
    loss, grad = check(ct, x, tg, SMALL_IL, SMALL_TL, dead=(2,), reduction=reduction, zero_infinity=zero_infinity,
                       logits=logits)
    per_utt, _ = run(ct, x, tg, SMALL_IL, SMALL_TL, reduction="none", zero_infinity=zero_infinity, logits=logits)
    per_utt = per_utt.detach().cpu()
    assert torch.isfinite(per_utt[:2]).all() and per_utt[2].item() == (0.0 if zero_infinity else INF)
    g = grad.cpu()
    assert not g[:, 2].any() and not g[4:, 1].any() and not g[3:, 2].any()      # exact zeros
    assert g[:, 0].any() and g[:4, 1].any()
    if reduction != "none" and not zero_infinity:
        assert loss.item() == INF


# ---------------------------------------------------------------- each CTC path by natural dispatch

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


PATHS = {  # name: (U, T, N, C, the first kernel's name starts with)
    "fused2": (5, 12, 4, 7, "ctc_fused_kernel<%s, %s, 2,"),
    "fused8": (200, 260, 3, 6, "ctc_fused_kernel<%s, %s, 8,"),
    "lattice": (257, 300, 2, 4, "ctc_lattice_kernel<%s,"),
    "wide": (257, 300, 24, 4, "ctc_fusedw_kernel<%s, %s,"),
    "generic": (3, 8, 2, 260, "ctc_lattice_generic_kernel<%s>"),
}


def ragged(rs, U, T, N, C):
    """lengths unsorted: the longest utterance is never the first, one utterance has U labels and every frame"""
    tl = [int(rs.randint(max(1, U // 2), U + 1)) for _ in range(N)]
    tl[N // 2] = U
    il = [int(rs.randint(u, T + 1)) for u in tl]
    il[N // 2] = T
    il[0] = max(tl[0], min(il[0], T - 1 - T // 8))
    seqs = [labels_without_repeats(rs, u, C) for u in tl]
    for n in range(N):              # a repeat (two, if the third label follows suit) where two frames are to spare
        if il[n] >= tl[n] + 2 and tl[n] > 1:
            seqs[n][1] = seqs[n][0]
    return il, tl, seqs


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", list(PATHS))
def test_padded_layout_through_each_path(ct, plan_query, name, dtype):
    for k in os.environ:
        assert not k.startswith("SCTC_CTC_"), "natural dispatch: %s is set" % k
    U, T, N, C, kernel = PATHS[name]
    rs = np.random.RandomState(len(name) + U)
    il, tl, seqs = ragged(rs, U, T, N, C)
    assert max(tl) == U and max(il) == T and il[0] < T and sorted(il, reverse=True) != il
    ri, st = ("double", "double") if dtype == torch.float64 else ("float", "unsigned int")
    names = plan_query(N, C, dtype, 2 * U + 1, T)
    want = kernel % ((ri, st)[:kernel.count("%s")])
    assert names[0].startswith(want), (names, want)
    x = make_input(rs, T, N, C, True, dtype)
    weight = torch.from_numpy(rs.rand(N) + 0.5)
    check(ct, x, padded(seqs), il, tl, reduction="none", logits=True, weight=weight)


# ---------------------------------------------------------------- strides

@pytest.mark.parametrize("logits", [False, True])
@pytest.mark.parametrize("dtype", DTYPES)
def test_strided_inputs_are_read_in_place(ct, dtype, logits):
    rs = np.random.RandomState(3)
    T, N, C = 9, 4, 6
    il, tl = [9, 5, 7, 8], [3, 2, 0, 4]
    tg = padded([labels_without_repeats(rs, u, C) for u in tl])
    x = make_input(rs, T, N, C, logits, dtype)
    base, base_grad = check(ct, x, tg, il, tl, reduction="none", logits=logits)

    def again(view):
        assert view.shape == (T, N, C) and not view.is_contiguous() and torch.equal(view.cpu(), x)
        v = view.detach().requires_grad_()
        loss = ct.ctc_loss(v, tg, il, tl, reduction="none", logits=logits)
        loss.sum().backward()
        assert torch.equal(loss, base) and torch.equal(v.grad, base_grad)       # bit-equal
        return v

    ntc = x.cuda().transpose(0, 1).contiguous()             # an [N, T, C] tensor ...
    v = again(ntc.transpose(0, 1))                          # ... seen as [T, N, C]
    assert v.stride() == (C, T * C, 1)
    wide = torch.zeros(T, N, 2 * C + 1, dtype=dtype).cuda()
    wide[:, :, 1::2] = x.cuda()
    v = again(wide[:, :, 1::2])                             # stride_c == 2
    assert v.stride()[2] == 2


# ---------------------------------------------------------------- grad_output

@pytest.mark.parametrize("dtype", DTYPES)
def test_grad_output_weights_and_backward_twice(ct, dtype):
    rs = np.random.RandomState(4)
    T, N, C = 8, 4, 5
    il, tl = [6, 8, 5, 8], [2, 3, 1, 2]
    tg = padded([labels_without_repeats(rs, u, C) for u in tl])
    x = make_input(rs, T, N, C, True, dtype)
    weight = torch.tensor([0.5, 3.0, 0.0, -2.0], dtype=torch.float64)      # exact in float32: one rounding either way
    _, unit = check(ct, x, tg, il, tl, reduction="none", logits=True)
    _, weighted = check(ct, x, tg, il, tl, reduction="none", logits=True, weight=weight)
    assert torch.equal(weighted, unit * weight.to(dtype).cuda()[None, :, None])
    assert not weighted[:, 2].any() and unit[:il[2], 2].any()
    xd = x.cuda().requires_grad_()
    loss = ct.ctc_loss(xd, tg, il, tl, reduction="sum", logits=True)
    g1, = torch.autograd.grad(loss, xd, retain_graph=True)
    g2, = torch.autograd.grad(loss, xd, retain_graph=True)
    assert torch.equal(g1, g2) and torch.equal(g1, unit)
    assert g1.data_ptr() != g2.data_ptr()                   # a fresh tensor per call


# ---------------------------------------------------------------- edge shapes

@pytest.mark.parametrize("dtype", DTYPES)
def test_edge_shapes(ct, dtype):
    rs = np.random.RandomState(5)
    for logits in (False, True):
        # N = 1
        check(ct, make_input(rs, 6, 1, 4, logits, dtype), padded([[1, 3]]), [6], [2], logits=logits)
        # T = 1 with U = 1: the one case where the reference's cost, -log(p_blank + p_label), is not the CTC loss
        check(ct, make_input(rs, 1, 2, 4, logits, dtype), padded([[2], [1]]), [1, 1], [1, 1], reduction="none", logits=logits)
        # ... among longer utterances, with the label equal to the blank, next to one frame for two labels (infeasible)
        x = make_input(rs, 5, 4, 4, logits, dtype)
        loss, _ = check(ct, x, padded([[2, 0], [3, 1], [0, 0], [1, 3]]), [1, 5, 1, 1], [1, 2, 1, 2], dead=(3,),
                        reduction="none", logits=logits)
        assert loss[3].item() == INF and torch.isfinite(loss[:3]).all()
        # blank = C - 1, and a label equal to the blank (0 is then a label like any other)
        C = 5
        x = make_input(rs, 9, 3, C, logits, dtype)
        check(ct, x, padded([[0, 1], [3, 0, 3], [2]]), [9, 7, 4], [2, 3, 1], blank=C - 1, reduction="sum", logits=logits)
        # (not as the LAST label: test_last_label_equal_to_the_blank)
        check(ct, x, padded([[0, 4, 1], [4, 2], [2, 3]]), [9, 7, 4], [3, 2, 2], blank=C - 1, reduction="none", logits=logits)
        check(ct, x, padded([[0, 1], [3, 0, 3], [2]]), [9, 7, 4], [2, 3, 1], blank=0, reduction="none", logits=logits)


@pytest.mark.parametrize("dtype", DTYPES)
def test_last_label_equal_to_the_blank(ct, dtype):
    """PyTorch documents that targets cannot be blank, and where the LAST label is the blank its CPU backward is off in
    the last frame: there it assigns the two end states' terms to their symbols instead of adding them, and the
    second (the label's) overwrites the first (the final blank's) -- e.g. T = 7, C = 5, blank = 4, target [4]: its
    d loss / d log p[6, 4] is -0.2266 where p - 1 = -0.9766 (the project's C oracle: -0.9766).  Its loss is right.  So
    for the target [blank] the loss is held against PyTorch and the gradient against the closed form: every alignment
    emits the blank in every frame, the gradient is p - onehot(blank)."""
    rs = np.random.RandomState(14)
    T, N, C = 7, 2, 5
    il, tl = [7, 5], [1, 1]
    tg = padded([[4], [4]])
    for logits in (False, True):
        x = make_input(rs, T, N, C, logits, dtype)
        want_loss, _ = oracle(x.double(), tg, il, tl, blank=4, reduction="none", logits=logits)
        loss, grad = run(ct, x, tg, il, tl, blank=4, reduction="none", logits=logits)
        assert_loss(loss, want_loss, dtype)
        p = x.double().softmax(2) if logits else x.double().exp()
        want_grad = p - torch.eye(C, dtype=torch.float64)[4]
        want_grad[5:, 1] = 0
        assert_grad(grad, want_grad, dtype, il)


def test_target_and_length_forms_agree(ct):
    rs = np.random.RandomState(6)
    T, N, C = 8, 3, 5
    il, tl = [8, 6, 7], [3, 1, 2]
    seqs = [labels_without_repeats(rs, u, C) for u in tl]
    x = make_input(rs, T, N, C, False, torch.float64)
    base, base_grad = check(ct, x, padded(seqs), il, tl, reduction="none")
    garbage = padded(seqs, fill=-1)
    garbage[1, 1], garbage[2, 2] = C + 7, C + 7
    cat = torch.tensor(sum(seqs, []), dtype=torch.int64)
    cat_tail = torch.cat([cat, torch.tensor([-1, C + 7])])
    forms = [
        (garbage, il, tl), (cat, il, tl), (cat_tail, tuple(il), tuple(tl)),
        (garbage.cuda(), il, tl), (cat.cuda().to(torch.int32), il, tl),                     # targets on the device
        (padded(seqs), torch.tensor(il), torch.tensor(tl)),                                 # lengths as tensors
        (padded(seqs).cuda(), torch.tensor(il).cuda(), torch.tensor(tl, dtype=torch.int32).cuda()),
    ]
    for tg, i, t in forms:
        loss, grad = run(ct, x, tg, i, t, reduction="none")
        assert torch.equal(loss, base) and torch.equal(grad, base_grad)


# ---------------------------------------------------------------- empty targets

@pytest.mark.parametrize("logits", [False, True])
@pytest.mark.parametrize("dtype", DTYPES)
def test_empty_targets(ct, dtype, logits):
    rs = np.random.RandomState(7)
    T, N, C = 70, 4, 6                      # more frames than one round of the empty-target wave's 64 lanes
    x = make_input(rs, T, N, C, logits, dtype)
    il = [70, 65, 3, 64]
    # one empty target among others; several; all of them
    for tl in ([2, 0, 1, 3], [0, 2, 0, 0], [0, 0, 0, 0]):
        tg = padded([labels_without_repeats(rs, u, C) for u in tl])
        for reduction in ("none", "mean"):
            check(ct, x, tg, il, tl, reduction=reduction, logits=logits)
        check(ct, x, tg, il, tl, blank=C - 1, reduction="sum", logits=logits)


@pytest.mark.parametrize("dtype", DTYPES)
def test_empty_target_with_an_impossible_blank(ct, dtype):
    rs = np.random.RandomState(8)
    T, N, C = 6, 3, 4
    il, tl = [6, 5, 6], [0, 2, 0]
    tg = padded([[], [1, 2], []])
    x = make_input(rs, T, N, C, False, dtype)
    x[2, 0, 0] = -INF                       # the first utterance's blank in one frame
    for zero_infinity in (False, True):
        loss, _ = check(ct, x, tg, il, tl, dead=(0,), reduction="none", zero_infinity=zero_infinity)
        assert loss[0].item() == (0.0 if zero_infinity else INF) and torch.isfinite(loss[1:]).all()
        total, _ = check(ct, x, tg, il, tl, dead=(0,), reduction="mean", zero_infinity=zero_infinity)
        assert np.isfinite(total.item()) == zero_infinity


# ---------------------------------------------------------------- skip

@pytest.mark.parametrize("logits", [False, True])
@pytest.mark.parametrize("dtype", DTYPES)
def test_skip_leaves_the_other_utterances_alone(ct, dtype, logits):
    rs = np.random.RandomState(9)
    T, N, C = 10, 3, 5
    il, tl = [9, 10, 8], [2, 3, 2]
    seqs = [[1, 2], [3, 4, 1], [2, 1]]
    tg = padded(seqs)
    x = make_input(rs, T, N, C, logits, dtype)
    clean, clean_grad = check(ct, x, tg, il, tl, reduction="none", logits=logits)
    x2 = x.clone()
    x2[:, 1, 4] = -INF                      # label 4 of the second utterance: impossible in every frame
    if not logits:
        x2[:, 1] = x2[:, 1].double().log_softmax(1).to(dtype)     # the rest of the row still sums to one
    for zero_infinity in (False, True):
        loss, grad = check(ct, x2, tg, il, tl, dead=(1,), reduction="none", zero_infinity=zero_infinity, logits=logits)
        assert loss[1].item() == (0.0 if zero_infinity else INF)
        assert not grad[:, 1].any()
        for n in (0, 2):                    # untouched, bit for bit
            assert loss[n].item() == clean[n].item() and torch.equal(grad[:, n], clean_grad[:, n])
        total, _ = check(ct, x2, tg, il, tl, dead=(1,), reduction="sum", zero_infinity=zero_infinity, logits=logits)
        assert np.isfinite(total.item()) == zero_infinity


# ---------------------------------------------------------------- gradient check, no_grad, requires_grad = False

def test_gradcheck(ct):
    rs = np.random.RandomState(10)
    T, N, C = 5, 2, 4
    il, tl = [5, 4], [2, 1]
    tg = padded([[1, 2], [3]])
    x = torch.from_numpy(rs.randn(T, N, C)).cuda().requires_grad_()
    for reduction in ("mean", "sum", "none"):
        assert torch.autograd.gradcheck(lambda v: ct.ctc_loss(v, tg, il, tl, reduction=reduction, logits=True), (x,),
                                        eps=1e-6, atol=1e-6, rtol=1e-5)
        assert torch.autograd.gradcheck(lambda v: ct.ctc_loss(v.log_softmax(2), tg, il, tl, reduction=reduction), (x,),
                                        eps=1e-6, atol=1e-6, rtol=1e-5)
    il0, tl0 = [5, 4], [0, 1]               # through the empty-target kernel
    assert torch.autograd.gradcheck(lambda v: ct.ctc_loss(v, tg, il0, tl0, logits=True), (x,), eps=1e-6, atol=1e-6, rtol=1e-5)


def test_no_grad_and_inputs_that_need_no_gradient(ct):
    rs = np.random.RandomState(11)
    T, N, C = 6, 2, 4
    il, tl = [6, 5], [2, 1]
    tg = padded([[1, 2], [3]])
    x = make_input(rs, T, N, C, True, torch.float32)
    want, _ = oracle(x.double(), tg, il, tl, logits=True)
    xd = x.cuda().requires_grad_()
    with torch.no_grad():
        loss = ct.ctc_loss(xd, tg, il, tl, logits=True)
    assert not loss.requires_grad and loss.grad_fn is None
    assert_loss(loss, want, torch.float32)
    loss = ct.ctc_loss(x.cuda(), tg, il, tl, logits=True)
    assert not loss.requires_grad
    assert_loss(loss, want, torch.float32)
    loss = ct.CTCLoss(logits=True)(xd, tg, il, tl)
    assert loss.requires_grad
    assert_loss(loss, want, torch.float32)


# ---------------------------------------------------------------- determinism

@pytest.mark.parametrize("dtype", DTYPES)
def test_two_runs_are_bit_equal(ct, dtype):
    rs = np.random.RandomState(12)
    T, N, C = 40, 5, 33                     # the prologue's row-per-wave mapping
    tl = [7, 0, 12, 3, 9]
    il = [30, 40, 25, 40, 18]
    tg = padded([labels_without_repeats(rs, u, C) for u in tl])
    for logits in (False, True):
        x = make_input(rs, T, N, C, logits, dtype)
        first = check(ct, x, tg, il, tl, logits=logits)
        second = run(ct, x, tg, il, tl, logits=logits)
        assert torch.equal(first[0], second[0]) and torch.equal(first[1], second[1])


# ---------------------------------------------------------------- the module inside a model

def test_module_in_a_model_one_sgd_step(ct):
    rs = np.random.RandomState(13)
    T, N, D, H, C = 12, 3, 6, 8, 5
    il, tl = [12, 9, 10], [3, 2, 4]
    tg = padded([labels_without_repeats(rs, u, C) for u in tl])
    feats = torch.from_numpy(rs.randn(T, N, D))

    def model():
        torch.manual_seed(3)
        return torch.nn.Sequential(torch.nn.Linear(D, H), torch.nn.Tanh(), torch.nn.Linear(H, C)).double()

    ref = model()
    opt = torch.optim.SGD(ref.parameters(), lr=0.1)
    F.ctc_loss(ref(feats).log_softmax(2), tg, torch.tensor(il), torch.tensor(tl)).backward()
    opt.step()
    for logits in (True, False):
        net = model().cuda()
        opt = torch.optim.SGD(net.parameters(), lr=0.1)
        crit = ct.CTCLoss(logits=logits)
        out = net(feats.cuda())
        crit(out if logits else out.log_softmax(2), tg, il, tl).backward()
        opt.step()
        for got, want in zip(net.parameters(), ref.parameters()):
            np.testing.assert_allclose(got.detach().cpu().numpy(), want.detach().numpy(), rtol=1e-7, atol=1e-11)
