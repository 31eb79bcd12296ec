"""GPU checks of the batched edit distance (csrc/edit_distance.hip): the
reference's own counts (tests/golden/edit_ref.npz), the restatement of the contract
(tests/edit_model.py) at every lane, panel and launch boundary, closed forms at the length
limit, the observable tie order, offsets and batch independence, the three Python surfaces
and runDecode.py.  Everything is integer-exact."""
import os
import pickle
import re

import numpy as np
import pytest

from tests import edit_model as em
from tests.test_dataloader import write_shard

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
PANEL = 256          # columns of b that one pass of the wave covers (edit_distance.hip)


def rand_seq(rs, n, A):
    return rs.randint(0, A, size=n).astype(np.int32)


def check_against_model(pairs, want=None):
    """stats and paths of one batched call equal the model's on every pair"""
    import ctc_fast
    stats, paths = ctc_fast.edit_distance_batch([a for a, _ in pairs], [b for _, b in pairs], ops=True)
    counts = ctc_fast.edit_distance_batch([a for a, _ in pairs], [b for _, b in pairs])
    assert stats.dtype == np.int32 and stats.shape == (len(pairs), 5)
    assert np.array_equal(stats, counts)
    for p, (a, b) in enumerate(pairs):
        ws, wp = want[p] if want is not None else em.edit_model(a, b)
        assert np.array_equal(stats[p], ws), (p, len(a), len(b), stats[p], ws)
        assert paths[p].dtype == np.int8 and np.array_equal(paths[p], wp), (p, len(a), len(b))
    return stats, paths


def test_reference_fixture():
    import ctc_fast
    z = np.load(os.path.join(GOLDEN, "edit_ref.npz"))
    ao = np.concatenate([[0], np.cumsum(z["a_len"])])
    bo = np.concatenate([[0], np.cumsum(z["b_len"])])
    P = len(z["a_len"])
    a = [z["a"][ao[p]:ao[p + 1]] for p in range(P)]
    b = [z["b"][bo[p]:bo[p + 1]] for p in range(P)]
    stats = ctc_fast.edit_distance_batch(a, b)
    assert P >= 300 and np.array_equal(stats, z["result"].astype(np.int32))
    stats2, _ = ctc_fast.edit_distance_batch(a, b, ops=True)
    assert np.array_equal(stats2, stats)


@pytest.mark.parametrize("A", [2, 30])
def test_lane_boundaries(A):
    rs = np.random.RandomState(100 + A)
    sizes = [0, 1, 2, 63, 64, 65, 127, 128, 129]
    check_against_model([(rand_seq(rs, n, A), rand_seq(rs, m, A)) for n in sizes for m in sizes])


def test_panel_boundaries():
    rs = np.random.RandomState(7)
    pairs = []
    for w in (PANEL - 1, PANEL, PANEL + 1, 2 * PANEL, 2 * PANEL + 1):
        for A in (2, 30):
            pairs.append((rand_seq(rs, w, A), rand_seq(rs, 70, A)))
            pairs.append((rand_seq(rs, 70, A), rand_seq(rs, w, A)))
    # 1100 x 1100: five panels, the path table in the workspace; one pair over two symbols and one that is mostly edits
    a = rand_seq(rs, 1100, 2)
    pairs.append((a, rand_seq(rs, 1100, 2)))
    b = a.copy()
    b[rs.randint(0, 1100, size=110)] ^= 1
    pairs.append((a, np.delete(b, rs.randint(0, 1100, size=40))))
    pairs.append((rand_seq(rs, 1100, 30), rand_seq(rs, 1100, 30)))
    check_against_model(pairs)


def test_length_limit_closed_forms():
    import ctc_fast
    N = 8191
    rs = np.random.RandomState(3)
    x = rand_seq(rs, N, 30)
    lo, hi = rand_seq(rs, N, 10), rand_seq(rs, 5000, 10) + 100      # disjoint alphabets: D[i,j] = max(i,j)
    a = [x, x, np.zeros(0, np.int32), lo, hi]
    b = [x, np.zeros(0, np.int32), x, hi, lo]
    stats = ctc_fast.edit_distance_batch(a, b)
    assert stats.tolist() == [[0, 0, 0, 0, N], [N, N, 0, 0, 0], [N, 0, N, 0, 0],
                              [N, N - 5000, 0, 5000, 0], [N, 0, N - 5000, 5000, 0]]
    # the paths of the disjoint pair: the priority rule puts the UPs (LEFTs) at the end of the longer sequence's
    # excess... wherever they fall, their counts are the stats and they walk both sequences to the end
    stats2, paths = ctc_fast.edit_distance_batch(a[1:], b[1:], ops=True)
    assert np.array_equal(stats2, stats[1:])
    for st, path, aa, bb in zip(stats2, paths, a[1:], b[1:]):
        assert [int((path == o).sum()) for o in (em.UP, em.LEFT, em.SUB, em.MATCH)] == st[1:].tolist()
        out, used = em.apply_path(aa, bb, path)
        assert used == len(aa) and np.array_equal(out, bb)
    with pytest.raises(ValueError):
        ctc_fast.edit_distance_batch([np.zeros(N + 1, np.int32)], [x])


def test_tie_order_is_the_references():
    import ctc_fast
    pairs = em.random_pairs(11, 3000, 13, [2, 3, 5, 30])
    want = [em.edit_model(a, b) for a, b in pairs]
    swapped = [em.edit_model(b, a) for a, b in pairs]
    differ = 0
    for (s, _), (t, _) in zip(want, swapped):
        assert s[0] == t[0]
        differ += (s[1], s[2], s[3]) != (t[2], t[1], t[3])       # swapping the arguments swaps UP and LEFT, no more
    assert differ >= 50, differ
    check_against_model(pairs, want)
    check_against_model([(b, a) for a, b in pairs], swapped)


def test_offsets_and_batch_independence():
    import ctc_fast
    rs = np.random.RandomState(5)
    ref = rand_seq(rs, 150, 34)
    hyps = [rand_seq(rs, int(rs.randint(100, 200)), 34) for _ in range(40)]
    shared = ctc_fast.edit_distance_batch([ref], hyps, a_index=[0] * 40)
    single = np.concatenate([ctc_fast.edit_distance_batch([ref], [h]) for h in hyps])
    assert np.array_equal(shared, single)
    assert np.array_equal(shared, ctc_fast.edit_distance_batch([ref] * 40, hyps))
    pairs = em.random_pairs(12, 3000, 40, [2, 5, 30])
    a, b = [x for x, _ in pairs], [y for _, y in pairs]
    stats, paths = ctc_fast.edit_distance_batch(a, b, ops=True)
    perm = rs.permutation(3000)
    stats_p, paths_p = ctc_fast.edit_distance_batch([a[i] for i in perm], [b[i] for i in perm], ops=True)
    assert np.array_equal(stats_p, stats[perm])
    assert all(np.array_equal(paths_p[k], paths[i]) for k, i in enumerate(perm))
    for i in (0, 1, 777, 1500, 2999):
        s1, p1 = ctc_fast.edit_distance_batch([a[i]], [b[i]], ops=True)
        assert np.array_equal(s1[0], stats[i]) and np.array_equal(p1[0], paths[i])
        ws, wp = em.edit_model(a[i], b[i])
        assert np.array_equal(stats[i], ws) and np.array_equal(paths[i], wp)
    empty = ctc_fast.edit_distance_batch([], [])
    assert empty.shape == (0, 5) and empty.dtype == np.int32
    s0, p0 = ctc_fast.edit_distance_batch([], [], ops=True)
    assert s0.shape == (0, 5) and p0 == []
    # any integer dtype
    got = ctc_fast.edit_distance_batch([np.array([1, 2, 3], np.int64), [4, 5], np.array([7], np.uint8)],
                                       [[1, 3], np.array([4, 5, 6], np.int16), []])
    assert got.tolist() == [[1, 1, 0, 0, 2], [1, 0, 1, 0, 2], [1, 1, 0, 0, 0]]


def test_editDistance_surface():
    import editDistance
    want = {("saturday", "sunday"): (3.0, 2, 0, 1, 5), ("kitten", "sitting"): (3.0, 0, 1, 2, 4),
            ("", "ab"): (2.0, 0, 2, 0, 0), ("ab", ""): (2.0, 2, 0, 0, 0)}
    for (ref, hyp), res in want.items():
        got = editDistance.edit_distance(list(ref), hyp)
        assert got == res and isinstance(got[0], float) and all(isinstance(v, int) for v in got[1:])
    got = editDistance.edit_distance("the cat sat".split(), "the bat sat down".split())
    assert got == (2.0, 0, 1, 1, 2)
    assert editDistance.edit_distance_many(["saturday", "kitten"], ["sunday", "sitting"]) == \
        [want[("saturday", "sunday")], want[("kitten", "sitting")]]


def test_editDist_surface():
    import editDist
    rs = np.random.RandomState(9)
    vocab = ["w%d" % i for i in range(12)]
    hyps = [[vocab[i] for i in rs.randint(0, 12, size=int(rs.randint(0, 25)))] for _ in range(200)]
    refs = []
    for p, h in enumerate(hyps):
        if p % 2:
            r = list(h)
            for _ in range(int(rs.randint(0, 6))):
                pos = int(rs.randint(0, len(r) + 1))
                if rs.rand() < 0.5 or not r:
                    r.insert(pos, vocab[int(rs.randint(0, 12))])
                else:
                    del r[min(pos, len(r) - 1)]
            refs.append(r)
        else:
            refs.append([vocab[i] for i in rs.randint(0, 4, size=int(rs.randint(0, 25)))])
    got = editDist.edit_distance_many(hyps, refs)
    for h, r, g in zip(hyps, refs, got):
        w = em.editdist_restated(h, r)
        assert g[:5] == w[:5], (h, r)
        assert g[5].dtype == w[5].dtype and np.array_equal(g[5], w[5]), (h, r, g[5], w[5])
        assert g[6] == w[6] and g[7] == w[7], (h, r)
    one = editDist.edit_distance(list("sunday"), list("saturday"))
    w = em.editdist_restated("sunday", "saturday")
    assert one[:5] == w[:5] and np.array_equal(one[5], w[5]) and one[6:] == w[6:]
    assert editDist.ref_to_hyp(one[6], one[7]) == [0, 1, 1, 1, 2, 3, 4, 5]


def test_nbest_oracle():
    import ctc_fast
    rs = np.random.RandomState(21)
    refs = [rand_seq(rs, int(rs.randint(5, 60)), 6) for _ in range(30)]
    lists = []
    for b, r in enumerate(refs):
        row = [rand_seq(rs, int(rs.randint(0, 60)), 6) for _ in range(int(rs.randint(1, 9)))]
        if b % 3 == 0:
            row.append(np.zeros(0, np.int32))             # an empty hypothesis is a hypothesis
        if b % 5 == 0:
            row.insert(1, r.copy())
            row.append(r.copy())                          # a tie at distance 0: the lower rank wins
        lists.append(row)
    refs.append(np.array([1, 2], np.int32))               # only the empty hypothesis
    lists.append([np.zeros(0, np.int32)])
    refs.append(np.array([3], np.int32))                  # a tie between different hypotheses
    lists.append([np.array([4, 4], np.int32), np.array([5], np.int32), np.array([6], np.int32)])
    best, dist, first = ctc_fast.nbest_oracle(refs, lists)
    for b, (r, row) in enumerate(zip(refs, lists)):
        d = [int(em.edit_model(r, h)[0][0]) for h in row]
        assert (best[b], dist[b], first[b]) == (d.index(min(d)), min(d), d[0]), b
    assert best[0] == 1 and dist[0] == 0 and best[-1] == 1 and dist[-1] == 1 and first[-1] == 2
    assert dist[-2] == 2 and best[-2] == 0


def test_run_decode_scores_on_the_device(tmp_path, capsys):
    import dataLoader as dl
    import runDecode
    import writeLikelihoods as wl
    from new_decoder import decoder
    from nnets import brnnet
    rs = np.random.RandomState(0)
    raw = img = 12
    A = 6
    data = tmp_path / "data"
    data.mkdir()
    utts = [("u%d" % i, int(rs.randint(12, 30)), list(rs.randint(1, A, size=3))) for i in range(5)]
    write_shard(data, 1, utts, raw, rs)
    net = brnnet.NNet(img, A, 32, 3, 40, train=False, temporalLayer=2)
    np.random.seed(1)
    net.initParams()
    loader = dl.DataLoader(str(data) + "/", raw, img)
    lik = tmp_path / "lik"
    lik.mkdir()
    wl.writeLogLikes(loader, net, 1, str(lik), writePickle=True)
    chars = tmp_path / "chars.txt"
    chars.write_text("".join(l for l in open(os.path.join(GOLDEN, "chars.txt")).readlines()[:A - 1]))
    lm = os.path.join(GOLDEN, "lm_char_2g.arpa")
    out, errf = tmp_path / "hyps.txt", tmp_path / "errs.txt"
    argv = ["--likelihoods", str(lik / "loglikelihoods_1.pk"), "--chars", str(chars), "--alis", str(data / "alis1.txt"),
            "--lm", lm, "--out", str(out), "--beam", "8", "--alpha", "0.5", "--batch", "2"]
    capsys.readouterr()
    cer = runDecode.main(argv)
    def summary():
        return [l for l in capsys.readouterr().out.splitlines() if l.startswith(("decoded ", "errors ", "oracle "))]
    plain = summary()
    hyps_plain = out.read_text()

    # the same CER from the host function, computed here
    with open(lik / "loglikelihoods_1.pk", "rb") as f:
        pk = pickle.load(f)
    alis = runDecode.load_alis(str(data / "alis1.txt"), str(chars))
    d = decoder.BeamLMDecoder()
    d.load_chars(str(chars))
    d.load_lm(lm)
    keys = sorted(pk)
    nbest = d.decode_batch([np.asfortranarray(pk[k], dtype=np.float64) for k in keys], 8, 0.5, 0.0, nbest=8)
    errs = sum(runDecode.edit_distance(alis[k], runDecode.tokens(row[0][0], d.char_int_map)) for k, row in zip(keys, nbest))
    n_ref = sum(len(alis[k]) for k in keys)
    assert n_ref > 0 and cer == errs / float(n_ref)
    assert plain == ["decoded 5 utterances, CER %.4f (%d / %d)" % (cer, errs, n_ref)]

    cer2 = runDecode.main(argv + ["--errors", str(errf), "--nbest-oracle", "8"])
    printed = summary()
    assert len(printed) == 3
    assert cer2 == cer and printed[0] == plain[0] and out.read_text() == hyps_plain
    rows = [l.split() for l in errf.read_text().splitlines()]
    assert [r[0] for r in rows] == keys
    tot = np.zeros(5, dtype=np.int64)
    for r in rows:
        v = np.array([int(x) for x in r[1:]])
        assert v[1] + v[2] + v[3] == v[0] and v[1] + v[3] + v[4] == len(alis[r[0]])
        tot += v
    assert tot[0] == errs
    assert printed[1] == "errors %d: ins %d, dels %d, subs %d, corr %d" % tuple(tot)
    oracle = 0
    for k, row in zip(keys, nbest):
        cands = [row[0][0]] + [h for h, s in row[1:] if s > -np.inf]
        oracle += min(runDecode.edit_distance(alis[k], runDecode.tokens(h, d.char_int_map)) for h in cands)
    m = re.match(r"oracle CER of 8-best ([0-9.]+) \((\d+) / (\d+)\), 1-best CER ([0-9.]+) \((\d+) / (\d+)\)$", printed[2])
    assert m, printed[2]
    assert (int(m.group(2)), int(m.group(3)), int(m.group(5)), int(m.group(6))) == (oracle, n_ref, errs, n_ref)
    assert oracle <= errs and m.group(1) == "%.4f" % (oracle / float(n_ref)) and m.group(4) == "%.4f" % cer
