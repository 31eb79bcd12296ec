"""GPU checks of NNet.forwardDevice / NNet.evaluate and of the scoring flags of runNNet.py:
the device route (forward pass, CTC cost, decoder, edit distance without leaving the device) against the host
route (forwardProbs, the NumPy collapse of tests/bestpath_model.py, the edit distance of tests/edit_model.py)."""
import json
import os
import pickle

import numpy as np
import pytest

from tests import bestpath_model as bm
from tests import edit_model
from tests.test_dataloader import write_shard

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
D, A, H, NL, TL = 20, 6, 30, 3, 2          # the network of __graft_entry__.smoke()
T_B = [10, 40, 1, 25, 17]
SYMBOLS = {1: "[space]", 2: "a", 3: "e", 4: "t", 5: "o"}


def make_net(train, maxUtts=2, seed=5):
    from nnets import brnnet
    np.random.seed(seed)
    net = brnnet.NNet(D, A, H, NL, 40, train=train, temporalLayer=TL, maxUtts=maxUtts)
    net.initParams()
    return net


def utterances():
    rs = np.random.RandomState(33)
    data = [rs.randn(D, T) for T in T_B]
    labels = [rs.randint(1, A, size=max(1, T // 5)).astype(np.int32) for T in T_B]
    labels[0] = rs.randint(1, A, size=14).astype(np.int32)      # longer than its 10 frames: no alignment
    return data, labels


def host_route(probs_list, labels, drop=(0,)):
    hyps = [bm.collapse(bm.argmax_rows(p.T), drop)[0] for p in probs_list]
    stats = np.stack([edit_model.edit_model(l, h)[0] for l, h in zip(labels, hyps)])
    return hyps, stats


def test_forward_device_is_forward_probs():
    import torch
    import ctc_fast
    net = make_net(train=False)
    data, _ = utterances()
    host = net.forwardProbs(data[:2])
    dev, T_b = net.forwardDevice(data[:2])
    assert T_b == T_B[:2] and dev.is_cuda and dev.dtype == torch.float32 and tuple(dev.shape) == (sum(T_b), A)
    got = dev.cpu().numpy()
    assert np.array_equal(got[:T_b[0]], host[0].T) and np.array_equal(got[T_b[0]:], host[1].T)
    assert host[0].flags.f_contiguous and host[0].shape == (A, T_b[0]) and host[0].dtype == np.float32
    logp, _ = net.forwardDevice(data[:2], log=True)
    assert int(bm.ulp_distance(logp.cpu().numpy(), bm.log_rows(got)).max()) <= 1
    assert torch.equal(logp, ctc_fast.log_rows(dev))
    with pytest.raises(ValueError):
        net.forwardDevice(data[:2], out=torch.empty((3, A), dtype=torch.float32, device="cuda"))


@pytest.mark.parametrize("train", [False, True])
def test_evaluate_best_path_against_the_host_route(train):
    import torch
    import ctc_fast
    net = make_net(train=train)
    data, labels = utterances()
    res = net.evaluate(data, labels, decode="best")
    probs = []
    for g in range(0, len(data), 2):                  # maxUtts = 2: three forward groups
        probs += net.forwardProbs(data[g:g + 2])
    hyps, stats = host_route(probs, labels)
    assert res["stats"].dtype == np.int32 and res["stats"].shape == (len(data), 5)
    assert np.array_equal(res["stats"], stats)
    assert len(res["hyps"]) == len(data) and sum(len(h) for h in hyps) >= len(data)     # not a batch of empty rows
    for got, want in zip(res["hyps"], hyps):
        assert got.dtype == np.int32 and np.array_equal(got, want)
    dev = torch.from_numpy(np.concatenate([np.ascontiguousarray(p.T) for p in probs])).cuda()
    cost, _, skip = ctc_fast.ctc_loss_batch(dev, labels, lengths=T_B)
    cost, skip = cost.cpu().numpy(), skip.cpu().numpy()
    assert res["cost"].dtype == np.float64 and res["skip"].dtype == bool
    np.testing.assert_array_equal(res["cost"], cost)
    np.testing.assert_array_equal(res["skip"], skip)
    assert res["skip"][0] or not np.isfinite(res["cost"][0])     # 14 labels in 10 frames
    assert np.isfinite(res["cost"][1:]).all() and not res["skip"][1:].any()
    # the ids of `drop` are never emitted
    res2 = net.evaluate(data, labels, decode="best", drop=(1, 2), cost=False)
    hyps2, stats2 = host_route(probs, labels, drop=(0, 1, 2))
    assert res2["cost"] is None and res2["skip"] is None and np.array_equal(res2["stats"], stats2)
    assert all(np.array_equal(g, w) for g, w in zip(res2["hyps"], hyps2))


def test_evaluate_beam_against_the_search_on_the_same_rows():
    import ctc_fast
    net = make_net(train=False)
    data, labels = utterances()
    lm = ctc_fast.DecodeLM(os.path.join(GOLDEN, "lm_char_2g.arpa"), SYMBOLS, A=A)
    try:
        res = net.evaluate(data, labels, decode="beam", lm=lm, beam=20, alpha=0.8, beta=0.5, cost=False)
        rows = []
        for g in range(0, len(data), 2):
            logp, T_b = net.forwardDevice(data[g:g + 2], log=True)
            host = logp.cpu().numpy()
            rows += [np.asfortranarray(r.T) for r in np.split(host, np.cumsum(T_b)[:-1])]
        hyps, _ = ctc_fast.decode_beam_batch(rows, beam=20, alpha=0.8, beta=0.5, lm=lm)
    finally:
        lm.close()
    stats = np.stack([edit_model.edit_model(l, h)[0] for l, h in zip(labels, hyps)])
    assert all(np.array_equal(g, w) for g, w in zip(res["hyps"], hyps))
    assert np.array_equal(res["stats"], stats)
    assert any(len(h) for h in hyps)


def test_a_training_step_after_evaluate_gives_the_same_gradient():
    import torch
    data, labels = utterances()
    net = make_net(train=True)
    c0, _, s0 = net.costAndGradBatch(data[1:3], labels[1:3])
    g0 = net.grad.flat.clone()
    net.grad.flat.zero_()
    net.evaluate(data, labels, decode="best")
    c1, _, s1 = net.costAndGradBatch(data[1:3], labels[1:3])
    assert torch.equal(net.grad.flat, g0) and np.array_equal(c0, c1) and np.array_equal(s0, s1)
    assert float(g0.abs().max()) > 0


def _shards(data_dir, n_files, rs):
    all_utts = {}
    for n in range(1, n_files + 1):
        utts = [("f%d_u%d" % (n, i), int(rs.randint(12, 30)), [int(x) for x in rs.randint(1, A, size=3)])
                for i in range(4)]
        write_shard(data_dir, n, utts, 12, rs)
        all_utts[n] = utts
    return all_utts


def _common(data):
    return ["--layerSize", "32", "--numLayers", "3", "--temporalLayer", "2", "--inputDim", "12", "--rawDim", "12",
            "--outputDim", str(A), "--maxUttLen", "40", "--numFiles", "2", "--dataDir", str(data) + "/", "--step", "1e-3",
            "--momentum", "0.9", "--save_every", "1"]


def _load_net(path, train=False, maxUtts=16):
    from nnets import brnnet
    net = brnnet.NNet(12, A, 32, 3, 40, train=train, temporalLayer=2, maxUtts=maxUtts)
    with open(path, "rb") as f:
        pickle.load(f)
        net.fromFile(f)
    return net


def test_runnnet_score_and_dev_flags(tmp_path):
    import dataLoader as dl
    import runNNet
    rs = np.random.RandomState(2)
    data, dev = tmp_path / "data", tmp_path / "dev"
    data.mkdir()
    dev.mkdir()
    _shards(data, 2, rs)
    dev_utts = _shards(dev, 2, rs)
    out = tmp_path / "run"
    runNNet.run(_common(data) + ["--epochs", "1", "--outputDir", str(out), "--devDir", str(dev) + "/", "--devFiles", "2"])
    # one dev_cer line for the one epoch; its CER is that of NNet.evaluate on the epoch's checkpoint
    lines = (out / "dev_cer").read_text().splitlines()
    assert len(lines) == 1
    epoch, cost, cer = lines[0].split()
    net = _load_net(out / "params.pk.epoch00", maxUtts=1)      # the trainer's model takes one utterance at a time
    loader = dl.DataLoader(str(dev) + "/", 12, 12)
    dist = refs = 0
    cost_sum = 0.0
    for n in (1, 2):
        dd, alis, keys, _ = loader.loadDataFileDict(n)
        labels = [np.array(alis[k], dtype=np.int32) for k in keys]
        res = net.evaluate([dd[k] for k in keys], labels)
        dist += int(res["stats"][:, 0].sum())
        refs += sum(len(l) for l in labels)
        cost_sum += float(res["cost"][~res["skip"]].sum())
    assert int(epoch) == 0 and refs == 24 and float(cer) == dist / float(refs)
    assert float(cost) == pytest.approx(cost_sum, rel=1e-12)
    assert "dev cost" in (out / "train.log").read_text()
    # test mode: --score writes cer.txt, equal to the host route, and leaves the likelihood files as they are
    plain, scored = tmp_path / "lik", tmp_path / "lik_score"
    test_args = ["--cfg_file", str(out / "cfg.json"), "--test", "--dataDir", str(dev) + "/", "--numFiles", "2"]
    runNNet.run(test_args + ["--likDir", str(plain)])
    assert not (plain / "cer.txt").exists()
    runNNet.run(test_args + ["--likDir", str(scored), "--score"])
    for name in sorted(os.listdir(plain)):
        assert (plain / name).read_bytes() == (scored / name).read_bytes(), name
    assert sorted(os.listdir(scored)) == sorted(os.listdir(plain) + ["cer.txt"])
    net = _load_net(out / "params.pk")               # the model and the grouping of test mode
    host_lines = []
    for n in (1, 2):
        dd, alis, keys, _ = loader.loadDataFileDict(n)
        labels = [np.array(alis[k], dtype=np.int32) for k in keys]
        hyps, stats = host_route(net.forwardProbs([dd[k] for k in keys]), labels)
        host_lines += ["%s %d %d %d %d %d" % (k, s[0], s[1], s[2], s[3], len(l)) for k, s, l in zip(keys, stats, labels)]
    assert (scored / "cer.txt").read_text().splitlines() == host_lines
    log = (out / "test.log").read_text()
    assert "File 1 cost" in log and "Total cost" in log and "CER" in log
    assert json.loads((out / "cfg.json").read_text())["devFiles"] == 2
    assert len(dev_utts) == 2
