"""The cudamat facade (stanford-ctc_amd/cudamat.py) as the REFERENCE trainer uses it, not only as this project's fused
rewrite does: INTEGRATION.md says ctc_fast/sgd.py drops in unchanged, and that file builds its velocity as standalone
CUDAMatrix objects, takes euclid_norm() per tensor, calls mult / add_mult per tensor and hands a plain list to
NNet.updateParams -- the non-flat branch, which no other test executes.

(a) the matrix object on dyadic data (multiples of 2^-4, so every result is exact in float32 and compared with
    array_equal): construction from float64 2-D, 1-D (a column) and (1, 1) arrays, empty(), the padded layout with its
    zero padding, copy_to_host / copy_to_device / asarray / assign(matrix) / assign(scalar), mult, add_mult between a
    standalone matrix and a view of a model's flat buffer in both directions (the rest of the flat buffer untouched),
    the shape check, euclid_norm, and `self` returned where the reference chains.

(b) the reference trainer's loop (ctc_fast/sgd.py:57-167) restated call for call through the facade, on the fixture of
    tests/test_gpu_sgd.py::test_sgd_matches_reference_loop (14 keys, one utterance that must skip, one longer than
    maxBatch, a clip that is taken at least three times), against the float64 NumPy loop on the oracle with the bars
    the fused sgd.SGD is held to (weights: relative norm < 2e-5; costs: rtol 2e-4; same iteration and cost counts), and
    against sgd.SGD itself from the same initial weights (same bound, same skip decisions).  The two differ only in
    where the clip factor is formed (host float64 here, on the device there) and in fused against separate multiply-adds.

OBSERVED (MI355X)
-----------------
reference loop through the facade vs the float64 oracle loop:  weights 9.2e-08 (bar 2e-5), velocity 1.9e-07
reference loop through the facade vs sgd.SGD (fused):          weights 6.6e-09 (bar 2e-5), costs 1.3e-07 relative
13 of the 14 utterances reach costAndGrad (u7 is filtered), u5 skips there; all three loops agree on both.
"""
import logging
import random

import numpy as np
import pytest

from tests.test_gpu_bf16x3 import print      # noqa: A004  also appends to the suite's test_notes.txt
from tests.test_gpu_sgd import flat, gflat, unflat

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (5, 1), (32, 64), (33, 65), (100, 200)]


@pytest.fixture(scope="module")
def mods():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    import cudamat as cm
    from nnets import brnnet
    import sgd
    from oracle import brnn as obrnn
    return cm, brnnet, sgd, obrnn, torch


def dyadic(rs, shape):
    return rs.randint(-256, 257, size=shape) / 16.0            # float64, like the arrays the reference passes


def whole(m):
    """the matrix's whole device buffer as [rows_p][ld], padding included"""
    import cudamat as cm
    rows_p, ld = cm.padded_layout(*m.shape)
    a = m._flat.cpu().numpy()
    assert a.size == rows_p * ld and a.dtype == np.float32
    return a.reshape(rows_p, ld)


def padded(a):
    import cudamat as cm
    a = np.asarray(a, dtype=np.float32)
    rows_p, ld = cm.padded_layout(*a.shape)
    out = np.zeros((rows_p, ld), dtype=np.float32)
    out[:a.shape[0], :a.shape[1]] = a
    return out


# ---------------------------------------------------------------- (a) the matrix object

@pytest.mark.parametrize("shape", SHAPES)
def test_construction_layout_and_copies(mods, shape):
    cm = mods[0]
    rs = np.random.RandomState(sum(shape))
    a = dyadic(rs, shape)
    assert a.dtype == np.float64
    m = cm.CUDAMatrix(a)
    assert m.shape == shape and m.numpy_array.dtype == np.float32
    np.testing.assert_array_equal(whole(m), padded(a))                  # zero padding to [ceil32][ceil64] (a column: [ceil32])
    host = m.copy_to_host()
    assert host is m.numpy_array and host.dtype == np.float32 and host.shape == shape
    np.testing.assert_array_equal(host, a.astype(np.float32))
    np.testing.assert_array_equal(m.asarray(), a.astype(np.float32))
    # the host copy is a copy: changing it and copy_to_device() is how fromFile loads (sgd.py:51-55)
    b = dyadic(rs, shape)
    m.numpy_array[:] = b
    np.testing.assert_array_equal(whole(m), padded(a))
    m.copy_to_device()
    np.testing.assert_array_equal(whole(m), padded(b))
    e = cm.empty(shape)
    assert e.shape == shape
    np.testing.assert_array_equal(whole(e), padded(np.zeros(shape)))
    assert e.assign(m) is e
    np.testing.assert_array_equal(whole(e), padded(b))
    np.testing.assert_array_equal(whole(m), padded(b))
    np.testing.assert_array_equal(e.copy_to_host(), b.astype(np.float32))


def test_one_dimensional_array_becomes_a_column(mods):
    cm = mods[0]
    a = dyadic(np.random.RandomState(1), (37,))
    m = cm.CUDAMatrix(a)
    assert m.shape == (37, 1) and whole(m).shape == (64, 1)
    np.testing.assert_array_equal(m.copy_to_host(), a.astype(np.float32).reshape(37, 1))
    np.testing.assert_array_equal(whole(m)[37:], 0)
    one = cm.CUDAMatrix(np.array([[2.5]]))
    assert one.shape == (1, 1) and one.copy_to_host().tolist() == [[2.5]] and one.euclid_norm() == 2.5


@pytest.mark.parametrize("shape", SHAPES)
def test_assign_scalar_mult_add_mult_and_norm(mods, shape):
    cm = mods[0]
    rs = np.random.RandomState(7 + sum(shape))
    a, b = dyadic(rs, shape), dyadic(rs, shape)
    m, o = cm.CUDAMatrix(a), cm.CUDAMatrix(b)
    ss = float(np.sum(a * a))                                   # exact: multiples of 2^-8 far below 2^53
    assert m.euclid_norm() == np.sqrt(ss)
    assert m.mult(0.25) is m
    np.testing.assert_array_equal(whole(m), padded(a * 0.25))
    assert m.add_mult(o, alpha=-0.5) is m
    np.testing.assert_array_equal(whole(m), padded(a * 0.25 - 0.5 * b))
    np.testing.assert_array_equal(whole(o), padded(b))          # the other operand is only read
    assert m.add_mult(o) is m                                   # alpha defaults to 1
    np.testing.assert_array_equal(whole(m), padded(a * 0.25 + 0.5 * b))
    assert m.euclid_norm() == np.sqrt(float(np.sum((a * 0.25 + 0.5 * b) ** 2)))
    # assign(scalar) fills the logical matrix and keeps the padding zero: the norm would count it
    assert m.assign(-0.5) is m
    np.testing.assert_array_equal(whole(m), padded(np.full(shape, -0.5)))
    assert m.euclid_norm() == 0.5 * np.sqrt(shape[0] * shape[1])
    assert m.assign(0) is m and m.euclid_norm() == 0.0
    with pytest.raises(ValueError):
        m.add_mult(cm.CUDAMatrix(np.zeros((shape[0] + 1, shape[1]))))
    with pytest.raises(ValueError):
        m.add_mult(cm.CUDAMatrix(np.zeros((shape[0], shape[1] + 1))))
    np.testing.assert_array_equal(whole(m), 0)


def test_standalone_matrices_and_views_of_a_flat_buffer_combine(mods):
    """add_mult with `other` a view of the model's flat parameter buffer and `self` standalone, and the reverse; the
    rest of the flat buffer keeps every bit"""
    cm, brnnet = mods[0], mods[1]
    rs = np.random.RandomState(21)
    D, A, H, NL, TL, T = 9, 5, 33, 2, 1, 8
    net = brnnet.NNet(D, A, H, NL, T, temporalLayer=TL)
    net._allocate()
    host = [[dyadic(rs, w.shape), dyadic(rs, b.shape)] for w, b in net.stack]
    net.setParams([[w, b if i <= NL else None] for i, (w, b) in enumerate(host)])
    for i in (0, 1, NL + 1):                            # an input layer, a hidden layer, a recurrent matrix
        for j in ((0, 1) if i <= NL else (0,)):         # weight and bias
            view, a = net.stack[i][j], host[i][j]
            np.testing.assert_array_equal(view.copy_to_host(), a.astype(np.float32))
            b = dyadic(rs, a.shape)
            alone = cm.CUDAMatrix(b)
            before = net._params.clone()
            assert alone.add_mult(view, alpha=0.5) is alone             # standalone += view
            np.testing.assert_array_equal(whole(alone), padded(b + 0.5 * a))
            assert bool((net._params == before).all())
            assert view.add_mult(alone, alpha=-2.0) is view             # view += standalone
            want = a - 2.0 * (b + 0.5 * a)
            np.testing.assert_array_equal(view.copy_to_host(), want.astype(np.float32))
            np.testing.assert_array_equal(whole(view), padded(want))
            changed = (net._params != before).cpu().numpy()
            lo = view._flat.data_ptr() - net._params.data_ptr()
            assert lo % 4 == 0
            lo //= 4
            assert not changed[:lo].any() and not changed[lo + view._flat.numel():].any()
            assert view.mult(0.5) is view
            np.testing.assert_array_equal(whole(view), padded(0.5 * want))
            assert view.euclid_norm() == np.sqrt(float(np.sum((0.5 * want) ** 2)))
            host[i][j] = 0.5 * want
    dummy = net.stack[NL + 1][1]
    assert dummy is net.stack[NL + 2][1] and dummy.shape == (1, 1) and dummy.euclid_norm() == 0.0


# ---------------------------------------------------------------- (b) the reference trainer's loop

ALPHA, MOMENTUM, CLIP = 1e-3, 0.9, 6.0             # a small clip, so that clipping is exercised
DIMS = (12, 7, 32, 3, 2, 30)                       # D, A, H, NL, TL, maxT


def weights(net, NL):
    return np.concatenate([np.concatenate([net.stack[i][0].copy_to_host().ravel(),
                                           net.stack[i][1].copy_to_host().ravel()]) for i in range(NL + 1)] +
                          [net.stack[NL + 1][0].copy_to_host().ravel(), net.stack[NL + 2][0].copy_to_host().ravel()])


def zeros_like_on_device(cm, matrix):
    """a standalone matrix of zeros with `matrix`'s logical shape, built from a float64 host array"""
    return cm.CUDAMatrix(np.zeros(matrix.shape))


def facade_loop(cm, net, maxBatch, data_dict, alis, keys):
    """ctc_fast/sgd.py restated through the facade: the same facade calls in the same order, cited by line.  Returns
    the bookkeeping and the velocity."""
    velocity = []                                                       # sgd.py:21-23: standalone, the dummy bias too
    for weight, bias in net.stack:
        velocity.append([zeros_like_on_device(cm, weight), zeros_like_on_device(cm, bias)])
    log = dict(it=0, costt=[], expcost=[], skipped=[], clipped=0, velocity=velocity)
    random.shuffle(keys)                                                # :68
    for step, key in enumerate(keys, start=1):                          # :71
        log["it"] = step
        momentum = MOMENTUM if step > 10 else 0.5                       # :64-65, :73-74
        frames = data_dict[key]
        n_frames = frames.shape[1]
        if n_frames > maxBatch:                                         # :77-80
            continue
        labels = np.array(alis[key], dtype=np.int32)                    # :82
        if len(labels) > n_frames:                                      # :84-88
            continue
        net.updateParams(momentum, velocity)                            # :93  a plain list: the non-flat branch
        cost, grad, skip = net.costAndGrad(frames, labels)              # :95
        net.updateParams(-momentum, velocity)                           # :100
        # :103-107, before the skip check: one euclid_norm() per tensor, weight before bias
        grad_norm = np.sqrt(sum(t.euclid_norm() ** 2 for pair in grad for t in pair))
        if skip:                                                        # :109-111
            log["skipped"].append(key)
            continue
        if np.isfinite(cost):                                           # :113-119
            history = log["expcost"]                                    # the first bookkept cost starts the average
            history.append(0.99 * history[-1] + 0.01 * cost if step > 1 and history else cost)
            log["costt"].append(cost)
        rate = ALPHA                                                    # :130-132
        if grad_norm > CLIP:
            rate = ALPHA * (CLIP / grad_norm)
            log["clipped"] += 1
        for (vel_w, vel_b), (grad_w, grad_b) in zip(velocity, grad):    # :133-139: both mult, then both add_mult
            for vel in (vel_w, vel_b):
                vel.mult(momentum)
            for vel, g in ((vel_w, grad_w), (vel_b, grad_b)):
                vel.add_mult(g, alpha=-rate)
        net.updateParams(1.0, velocity)                                 # :140-141,161
    return log


@pytest.fixture(scope="module")
def loops(mods):
    """the fixture of test_sgd_matches_reference_loop, run three ways from the same weights in the same key order"""
    cm, brnnet, sgd, obrnn, torch = mods
    rs = np.random.RandomState(3)
    D, A, H, NL, TL, maxT = DIMS
    params = obrnn.init_params(D, A, H, NL, TL, rng=rs)
    keys = ["u%d" % i for i in range(14)]
    data_dict, alis = {}, {}
    for i, k in enumerate(keys):
        T = int(rs.randint(8, maxT))
        data_dict[k] = (rs.randn(D, T) * 2.0).astype(np.float32)
        alis[k] = [str(v) for v in rs.randint(1, A, size=3)]
    alis["u5"] = ["2"] * 9
    data_dict["u5"] = data_dict["u5"][:, :12]                       # 9 repeats need 17 frames -> skip
    data_dict["u7"] = rs.randn(D, maxT + 5).astype(np.float32)      # longer than maxBatch -> filtered
    st = [[w, b] for w, b in zip(params["W"], params["b"])] + [[params["Wf"], None], [params["Wb"], None]]

    net = brnnet.NNet(D, A, H, NL, maxT, temporalLayer=TL)
    net.setParams(st)
    random.seed(11)
    order = list(keys)
    fac = facade_loop(cm, net, maxT, data_dict, alis, order)

    # sgd.SGD, the fused rewrite, on the same keys
    net2 = brnnet.NNet(D, A, H, NL, maxT, temporalLayer=TL)
    net2.setParams(st)
    opt = sgd.SGD(net2, maxT, alpha=ALPHA, momentum=MOMENTUM, maxGradNorm=CLIP)
    records = []

    class Grab(logging.Handler):
        def emit(self, r):
            records.append(r.getMessage())
    root, h = logging.getLogger(), Grab()
    old = root.level
    root.addHandler(h)
    root.setLevel(logging.INFO)
    try:
        random.seed(11)
        order2 = list(keys)
        opt.run(data_dict, alis, order2)
    finally:
        root.removeHandler(h)
        root.setLevel(old)
    assert order2 == order
    fused_skipped = [m.split("Key=")[1].split(",")[0] for m in records if m.startswith("SKIPPING: Key=")]

    # the float64 NumPy loop on the oracle
    w = flat(params).astype(np.float64)
    v = np.zeros_like(w)
    it, costt, clipped, skipped = 0, [], 0, []
    mom = 0.5
    with np.errstate(all="ignore"):
        for k in order:
            it += 1
            if it > 10:
                mom = MOMENTUM
            x = data_dict[k]
            if x.shape[1] > maxT:
                continue
            lab = np.array(alis[k], dtype=np.int32)
            if x.shape[1] < lab.shape[0]:
                continue
            cost, g, skip, _ = obrnn.cost_and_grad(unflat(w + mom * v, params), x, lab, TL, 20.0)
            if skip:
                skipped.append(k)
                continue
            gv = gflat(g)
            gnorm = np.sqrt(np.sum(gv ** 2))
            alph = ALPHA * (CLIP / gnorm) if gnorm > CLIP else ALPHA
            clipped += gnorm > CLIP
            v = mom * v - alph * gv
            w = w + v
            costt.append(cost)
    ref = dict(it=it, costt=costt, clipped=clipped, skipped=skipped, w=w, v=v, w0=flat(params))
    return dict(net=net, fac=fac, net2=net2, opt=opt, fused_skipped=fused_skipped, ref=ref, NL=NL, keys=keys)


def test_reference_loop_through_the_facade_matches_the_oracle(loops):
    fac, ref, net, NL = loops["fac"], loops["ref"], loops["net"], loops["NL"]
    assert type(fac["velocity"]) is list                                # the non-flat branch of updateParams ran
    assert all(type(p) is list and len(p) == 2 for p in fac["velocity"]) and len(fac["velocity"]) == NL + 3
    assert fac["velocity"][NL + 1][1] is not fac["velocity"][NL + 2][1]           # one velocity per dummy, like sgd.py:21-23
    assert ref["clipped"] >= 3 and fac["clipped"] == ref["clipped"]
    assert fac["it"] == ref["it"] == len(loops["keys"])
    assert fac["skipped"] == ref["skipped"] and "u5" in fac["skipped"]
    assert len(fac["costt"]) == len(ref["costt"]) == len(fac["expcost"])
    np.testing.assert_allclose(fac["costt"], ref["costt"], rtol=2e-4)
    got = weights(net, NL)
    err = np.linalg.norm(got - ref["w"]) / np.linalg.norm(ref["w"])
    print("cudamat facade, reference loop vs float64 oracle loop: weights relative norm %.2e (bound 2e-5)" % err)
    assert err < 2e-5
    assert np.linalg.norm(got - ref["w0"]) / np.linalg.norm(ref["w"]) > 1e-3        # it did move
    # the velocity against the oracle's: reported, the bars are on the weights
    vel =np.concatenate([np.concatenate([fac["velocity"][i][0].copy_to_host().ravel(),
                                          fac["velocity"][i][1].copy_to_host().ravel()]) for i in range(NL + 1)] +
                         [fac["velocity"][NL + 1][0].copy_to_host().ravel(),
                          fac["velocity"][NL + 2][0].copy_to_host().ravel()])
    verr = np.linalg.norm(vel - ref["v"]) / np.linalg.norm(ref["v"])
    print("cudamat facade, reference loop vs float64 oracle loop: velocity relative norm %.2e" % verr)
    for i in (NL + 1, NL + 2):
        assert fac["velocity"][i][1].euclid_norm() == 0.0               # the dummy bias never moves


def test_reference_loop_through_the_facade_matches_the_fused_trainer(loops):
    fac, opt, NL = loops["fac"], loops["opt"], loops["NL"]
    assert opt.it == fac["it"] and loops["fused_skipped"] == fac["skipped"]
    assert len(opt.costt) == len(fac["costt"])
    np.testing.assert_allclose(opt.costt, fac["costt"], rtol=2e-4)
    a, b = weights(loops["net"], NL), weights(loops["net2"], NL)
    diff = np.linalg.norm(a - b) / np.linalg.norm(b)
    cdiff = float(np.max(np.abs(np.array(opt.costt) - np.array(fac["costt"])) / np.abs(np.array(fac["costt"]))))
    print("cudamat facade, reference loop vs sgd.SGD: weights relative norm %.2e (bound 2e-5), costs %.2e" % (diff, cdiff))
    assert diff < 2e-5


def test_stack_still_views_the_flat_buffer_after_the_loop(loops):
    """a fused updateParams over the flat buffer must change what the stack's matrices return"""
    net, NL = loops["net"], loops["NL"]
    before = [net.stack[i][0].copy_to_host().copy() for i in range(NL + 3)]
    grads = [net.grad[i][0].copy_to_host().copy() for i in range(NL + 3)]
    assert all(np.abs(g).max() > 0 for g in grads)
    net.updateParams(0.5, net.grad)                                     # the flat fast path
    for i in range(NL + 3):
        after = net.stack[i][0].copy_to_host()
        assert not np.array_equal(after, before[i]), i
        np.testing.assert_allclose(after, before[i] + 0.5 * grads[i], rtol=1e-6, atol=1e-7)
