"""17..32 utterances at H = 1824 / 2048 (round 7): the default recurrence is the tiled kernel with 16 units x both
utterance tiles of a direction per CU (brnn_recurrent_t_kernel<..., UG = 1>, the tiles' steps alternating on one CU).
It keeps the K split, the MFMAs and the order of every addition of the two-chain kernel (brnn_recurrent_q_kernel,
SCTC_REC_VARIANT=51), so costs, skips and every gradient of a step are bit for bit the same -- both passes, equal and
ragged lengths, B = 17 (a second tile with one live utterance) -- and a repeated step gives the same bits."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mods():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from nnets import brnnet
    from oracle import brnn as obrnn
    return brnnet, obrnn


def _net(brnnet, dims, params, B):
    D, A, H, NL, TL, T = dims
    net = brnnet.NNet(D, A, H, NL, T, temporalLayer=TL, maxUtts=B)
    net.maxAct = 20.0
    st = [[w, b] for w, b in zip(params["W"], params["b"])] + [[params["Wf"], None], [params["Wb"], None]]
    net.setParams(st)
    return net


def _step(net, datas, labs, NL):
    costs, _, skips = net.costAndGradBatch(datas, labs)
    return costs.copy(), skips.copy(), [net.grad[i][0].copy_to_host().copy() for i in range(NL + 3)]


@pytest.mark.parametrize("ragged", [False, True])
@pytest.mark.parametrize("B", [17, 24, 32])
@pytest.mark.parametrize("H", [1824, 2048])
def test_recurrence_32_tiled_form_is_bit_identical_to_two_chain_kernel(mods, monkeypatch, H, B, ragged):
    brnnet, obrnn = mods
    rs = np.random.RandomState(7 * H + B + int(ragged))
    D, A, NL, TL, Tmax = 24, 33, 3, 2, 40
    params = obrnn.init_params(D, A, H, NL, TL, rng=rs)
    Ts = [int(t) for t in rs.randint(2, Tmax + 1, size=B)] if ragged else [Tmax] * B
    Ts[0] = Tmax
    datas = [rs.randn(D, T) for T in Ts]
    labs = [rs.randint(1, A, size=max(1, T // 5)).astype(np.int32) for T in Ts]
    res = {}
    for variant in ("0", "51"):
        monkeypatch.setenv("SCTC_REC_VARIANT", variant)
        net = _net(brnnet, (D, A, H, NL, TL, Tmax), params, B)
        res[variant] = _step(net, datas, labs, NL)
        assert net.recurrentPath()[:2] == (1, 1)
        if variant == "0":      # run-to-run: the same step again on the same net
            again = _step(net, datas, labs, NL)
            np.testing.assert_array_equal(res[variant][0], again[0])
            for a, b in zip(res[variant][2], again[2]):
                np.testing.assert_array_equal(a, b)
        del net
    new, old = res["0"], res["51"]
    np.testing.assert_array_equal(new[0], old[0])
    np.testing.assert_array_equal(new[1], old[1])
    assert np.isfinite(new[0][~new[1]]).all()
    for a, b in zip(new[2], old[2]):
        np.testing.assert_array_equal(a, b)
