"""sctc_intern_words_batch on the GPU against tests/mbr_model.py: ids, counts and status bit for bit,
whole output buffers with guard words behind them (a slot that holds no word keeps the fill), the exact workspace with a
guard behind it; and word_errors_batch against editDistance.edit_distance on the split strings."""
import ctypes

import numpy as np
import pytest

from tests import beam_trace as bt
from tests import mbr_model as M

pytestmark = pytest.mark.gpu

GUARD = -0x21524111
TAIL = 16
SP = 1


def run_intern(rows, groups, space=SP, A=65, labels=None, U=None, off=None):
    """the raw entry on `rows` (uploaded back to back), or on a device tensor with explicit lengths / offsets; returns
    the three whole buffers, guards included"""
    import torch
    import _sctc
    if labels is None:
        U = np.array([len(r) for r in rows], dtype=np.int32)
        off = np.concatenate([[0], np.cumsum(U)[:-1]]).astype(np.int64) if len(rows) else np.zeros(0, np.int64)
        flat = np.concatenate([np.asarray(r, dtype=np.int32).reshape(-1) for r in rows] + [np.zeros(1, np.int32)])
        labels = torch.from_numpy(flat).cuda()
    U = np.ascontiguousarray(U, dtype=np.int32)
    off = np.ascontiguousarray(off, dtype=np.int64)
    g = np.ascontiguousarray(groups, dtype=np.int32)
    N = U.shape[0]
    cfg = _sctc.InternConfig(N, g.shape[0] - 1, A, space, _sctc.i32(U), _sctc.i64(off), _sctc.i32(g))
    L = _sctc.lib()
    nbytes = ctypes.c_size_t(0)
    _sctc.check(L.sctc_intern_words_workspace_bytes(ctypes.byref(cfg), ctypes.byref(nbytes)), "test")
    slots = _sctc.intern_slots(U)[1]
    ids = torch.full((slots + TAIL,), GUARD, dtype=torch.int32, device="cuda")
    counts = torch.full((N + TAIL,), GUARD, dtype=torch.int32, device="cuda")
    status = torch.full((N + TAIL,), GUARD, dtype=torch.int32, device="cuda")
    ws = torch.full((nbytes.value + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    rc = L.sctc_intern_words_batch(ctypes.byref(cfg), labels.data_ptr(), ids.data_ptr(), counts.data_ptr(), status.data_ptr(),
                                   ws.data_ptr(), nbytes.value, _sctc.current_stream_ptr())
    _sctc.check(rc, "test")
    assert (ws[nbytes.value:].cpu().numpy() == 0xA5).all(), "the call wrote behind its workspace"
    return ids.cpu().numpy(), counts.cpu().numpy(), status.cpu().numpy()


def want_buffers(rows, groups, space=SP, A=65):
    flat, counts, status, _ = M.intern_buffers(rows, groups, space, A, fill=GUARD)
    tail = np.full(TAIL, GUARD, dtype=np.int32)
    return np.concatenate([flat, tail]), np.concatenate([counts, tail]), np.concatenate([status, tail])


def check(rows, groups, **kw):
    got = run_intern(rows, groups, **kw)
    want = want_buffers(rows, groups, **kw)
    for g, w, name in zip(got, want, ("ids", "counts", "status")):
        np.testing.assert_array_equal(g, w, err_msg=name)
    return got


def test_small_cases():
    rows = [
        [2, 3, 4],                                  # group 0: a group of one row
        [],                                         # group 1: an empty row
        [SP, SP, SP],                               # group 2: spaces only
        [SP, 2, 3, SP, SP, 4, SP],                  # group 3: leading, trailing and doubled spaces ...
        [2, 3, 5, SP, 2, 3, 4, SP, 2, 3],           #   ... words that differ in the last symbol only, and a prefix
        [4, SP, 2, 3, 5, SP, 4, SP, 9],             #   ... the same word in another row and twice in one row
        [7],                                        # group 4
        [7, SP, 7],
    ]
    ids, counts, status = check(rows, [0, 1, 2, 3, 6, 8])
    assert counts[:8].tolist() == [1, 0, 0, 2, 3, 4, 1, 2] and not status[:8].any()
    # hand-worked, group 3: "cd e" -> 0 1; "cdf cde cd" -> 2 3 0; "e cdf e j" -> 1 2 1 8
    first = np.concatenate([[0], np.cumsum([(len(r) + 1) // 2 for r in rows])])
    assert ids[first[3]:first[3] + 2].tolist() == [0, 1]
    assert ids[first[4]:first[4] + 3].tolist() == [2, 3, 0]
    assert ids[first[5]:first[5] + 4].tolist() == [1, 2, 1, 8]
    assert ids[first[7]:first[7] + 2].tolist() == [0, 0]


@pytest.mark.parametrize("n", [65, 4095])
def test_one_long_word(n):
    rs = np.random.RandomState(n)
    word = rs.randint(2, 65, size=n).astype(np.int32)
    other = word.copy()
    other[-1] = 2 + (other[-1] - 1) % 63            # differs in the last symbol only
    assert other[-1] != word[-1]
    ids, counts, _ = check([word, other, word], [0, 3])
    first = [0, (n + 1) // 2, 2 * ((n + 1) // 2)]
    assert [ids[f] for f in first] == [0, 1, 0] and counts[:3].tolist() == [1, 1, 1]


def test_more_tokens_than_any_on_chip_table():
    """2 048 distinct two-symbol words over four rows of one group, and a fifth row that repeats 600 of them in
    another order: 2 648 tokens in one group's table"""
    rs = np.random.RandomState(7)
    pairs = [(a, b) for a in range(2, 65) for b in range(2, 65)]
    pick = rs.permutation(len(pairs))[:2048]
    words = [pairs[i] for i in pick]

    def row(ws):
        out = []
        for w in ws:
            out += list(w) + [SP]
        return out[:-1]
    rows = [row(words[i:i + 512]) for i in range(0, 2048, 512)]
    again = rs.permutation(2048)[:600]
    rows.append(row([words[i] for i in again]))
    ids, counts, _ = check(rows, [0, 5])
    assert counts[:5].tolist() == [512] * 4 + [600]
    first = np.concatenate([[0], np.cumsum([(len(r) + 1) // 2 for r in rows])])
    assert ids[:512].tolist() == list(range(512))
    assert ids[first[4]:first[4] + 600].tolist() == again.tolist()


def test_status_2_and_guards():
    rows = [[2, 3, SP, 4], [2, 65, 3], [0], [4, SP, 2, 3], [SP, 64]]
    ids, counts, status = check(rows, [0, 5], A=65)
    assert status[:5].tolist() == [0, 2, 2, 0, 0] and counts[:5].tolist() == [2, 0, 0, 2, 1]
    assert (ids[2:5] == GUARD).all()                # the slots of the two bad rows


def test_in_place_on_a_search_with_repeated_offsets():
    """the rows lie in the ids tensor of a beam search and are addressed there, some of them twice"""
    import ctc_fast
    rs = np.random.RandomState(11)
    T_b, K, A = [30, 22], 4, 35
    lps = [bt.peaked(rs, A, T) for T in T_b]
    ids_dev, lens_dev, _ = ctc_fast.decode_beam_batch(lps, beam=8, nbest=K, device=True)
    flat, lens = ids_dev.cpu().numpy(), lens_dev.cpu().numpy()
    foff = np.array([0, T_b[0]], dtype=np.int64)
    loff = (K * foff[:, None] + np.arange(K)[None, :] * np.array(T_b)[:, None]).reshape(-1)
    take = [0, 1, 0, 2, 3, 3, 4, 5, 4, 7, 6, 5]     # rows of both utterances, repeated
    U, off = lens[take], loff[take]
    rows = [flat[o:o + u] for o, u in zip(off, U)]
    assert sum(len(r) for r in rows) > 30
    space = int(np.bincount(np.concatenate(rows), minlength=A)[1:].argmax()) + 1     # the commonest symbol cuts the words
    groups = [0, 6, 12]
    got = run_intern(None, groups, space=space, A=A, labels=ids_dev, U=U, off=off)
    want = want_buffers(rows, groups, space=space, A=A)
    for g, w in zip(got, want):
        np.testing.assert_array_equal(g, w)
    assert got[1][:12].sum() > 12                   # there are words to speak of
    # the Python surface on the same triple, and the same bits from a second call
    a_ids, a_counts = ctc_fast.intern_words((ids_dev, U, off), groups, space, A=A, device=True)
    b_ids, b_counts = ctc_fast.intern_words((ids_dev, U, off), groups, space, A=A, device=True)
    assert (a_ids == b_ids).all() and (a_counts == b_counts).all()
    host_ids, host_counts = ctc_fast.intern_words(rows, groups, space, A=A)
    m_ids, m_counts, _ = M.intern(rows, groups, space, A)
    assert [v.tolist() for v in host_ids] == [v.tolist() for v in m_ids] and host_counts.tolist() == m_counts.tolist()
    np.testing.assert_array_equal(a_counts.cpu().numpy(), m_counts)


def test_two_calls_give_the_same_bits():
    rs = np.random.RandomState(3)
    rows = [rs.randint(1, 6, size=int(rs.randint(0, 200))).astype(np.int32) for _ in range(64)]
    groups = [0, 1, 9, 9, 40, 64]
    a = check(rows, groups, A=6)
    b = run_intern(rows, groups, A=6)
    for x, y in zip(a, b):
        np.testing.assert_array_equal(x, y)


def test_python_surface_rejects_bad_rows():
    import ctc_fast
    with pytest.raises(ValueError):
        ctc_fast.intern_words([[2, 3], [2, 9]], [0, 2], SP, A=8)
    with pytest.raises(ValueError):
        ctc_fast.intern_words([[2, 3]], [0, 2], SP, A=8)        # the groups do not end at the rows


def test_word_errors_batch_against_edit_distance():
    """seeded sentence pairs over a vocabulary of 40 random words plus OOV-like words made up on the spot, which a
    lexicon would all map to <UNK>: here they share no id unless they are the same word"""
    import ctc_fast
    import editDistance
    rs = np.random.RandomState(5)
    A = 30

    def word():
        return "".join(chr(ord("a") + int(c)) for c in rs.randint(0, 26, size=int(rs.randint(1, 7))))
    vocab = [word() for _ in range(40)]

    def sentence():
        ws = [vocab[int(rs.randint(40))] if rs.rand() < 0.7 else word() + "zq" for _ in range(int(rs.randint(0, 13)))]
        return " ".join(ws)

    def labels(s):
        return np.array([SP if c == " " else 2 + ord(c) - ord("a") for c in s], dtype=np.int32)
    refs, hyps = [], []
    for p in range(60):
        ref = sentence()
        toks = ref.split()
        for _ in range(int(rs.randint(0, 4))):
            kind, pos = int(rs.randint(3)), int(rs.randint(0, len(toks) + 1))
            if kind == 0:
                toks.insert(pos, word() + "zq")
            elif toks and kind == 1:
                del toks[min(pos, len(toks) - 1)]
            elif toks:
                toks[min(pos, len(toks) - 1)] = word() + "zq"
        refs.append(ref)
        hyps.append("  ".join(toks) + (" " if p % 3 == 0 else ""))      # doubled and trailing spaces are no words
    got = ctc_fast.word_errors_batch([labels(r) for r in refs], [labels(h) for h in hyps], SP, A=A)
    want = np.array([editDistance.edit_distance(r.split(), h.split()) for r, h in zip(refs, hyps)], dtype=np.int32)
    np.testing.assert_array_equal(got, want)
    # and against the restatement of the table, which shares no code with the device
    from tests import edit_model
    for p in range(0, 60, 6):
        table = {}
        a, b = ([table.setdefault(t, len(table)) for t in s.split()] for s in (refs[p], hyps[p]))
        np.testing.assert_array_equal(got[p], edit_model.edit_model(a, b)[0])
    assert want[:, 0].sum() > 30 and want[:, 4].sum() > 100
