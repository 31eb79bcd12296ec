"""CPU checks of the edit-distance work: the restatement of the contract
(tests/edit_model.py) against the reference's own results (tests/golden/edit_ref.npz) and
against itself, the restated editDist.pyx on hand-worked cases, the host-side derivation of
stanford-ctc_amd/editDist.py from a path, and the C boundary (argument errors without a GPU,
struct layout)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from tests import edit_model as em

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


@pytest.fixture(scope="module")
def sctc():
    import __graft_entry__ as ge
    import _sctc
    if not os.path.exists(_sctc.LIB_PATH):
        ge.build()
    return _sctc


@pytest.fixture(scope="module")
def fixture_pairs():
    z = np.load(os.path.join(GOLDEN, "edit_ref.npz"))
    ao = np.concatenate([[0], np.cumsum(z["a_len"])])
    bo = np.concatenate([[0], np.cumsum(z["b_len"])])
    return [(z["a"][ao[p]:ao[p + 1]], z["b"][bo[p]:bo[p + 1]], z["result"][p]) for p in range(len(z["a_len"]))]


def test_model_equals_the_reference_fixture(fixture_pairs):
    assert len(fixture_pairs) >= 300
    assert fixture_pairs[0][2].tolist() == [3, 2, 0, 1, 5] and fixture_pairs[1][2].tolist() == [3, 0, 1, 2, 4]
    assert fixture_pairs[2][2].tolist() == [2, 0, 2, 0, 0] and fixture_pairs[3][2].tolist() == [2, 2, 0, 0, 0]
    assert fixture_pairs[4][2].tolist() == [0, 0, 0, 0, 0]
    assert {0, 40} <= {len(a) for a, _, _ in fixture_pairs}
    for a, b, res in fixture_pairs:
        stats, _ = em.edit_model(a, b)
        assert np.array_equal(stats, res), (a, b)


def test_forward_counts_equal_the_trace_back(fixture_pairs):
    pairs = [(a, b) for a, b, _ in fixture_pairs[:150]] + em.random_pairs(4, 300, 13, [2, 3, 5, 30])
    for a, b in pairs:
        fwd, back, path = em.edit_model_loop(a, b)
        stats, path2 = em.edit_model(a, b)
        assert np.array_equal(fwd, back) and np.array_equal(back, stats) and np.array_equal(path, path2)


def test_paths_rebuild_b_and_count_like_the_stats(fixture_pairs):
    for a, b, _ in fixture_pairs:
        stats, path = em.edit_model(a, b)
        out, used = em.apply_path(a, b, path)
        assert used == len(a) and list(out) == list(b)
        assert [int((path == o).sum()) for o in (em.UP, em.LEFT, em.SUB, em.MATCH)] == stats[1:].tolist()
        assert stats[0] == stats[1] + stats[2] + stats[3] and len(path) == stats[0] + stats[4]


def test_the_vectorised_model_is_quick():
    rs = np.random.RandomState(0)
    stats, path = em.edit_model(rs.randint(0, 2, 1100), rs.randint(0, 2, 1100))
    assert len(path) == stats[0] + stats[4]


HAND = [
    # hyp, ref -> ed, eq, ins, dels, subs, errs_by_pos, hyp_corr, ref_corr   (editDist.pyx:40-108 by hand)
    ("sunday", "saturday", (3, 5, 2, 0, 1, [2, 0, 1, 0, 0, 0],
                            ["s", "<ins>", "<ins>", "u", "n", "d", "a", "y"], list("saturday"))),
    ("sitting", "kitten", (3, 4, 0, 1, 2, [1, 0, 0, 0, 1, 0, 1],
                           list("sitting"), ["k", "i", "t", "t", "e", "n", "<del>"])),
    ("", "ab", (2, 0, 2, 0, 0, [], ["<ins>", "<ins>"], ["a", "b"])),
    ("ab", "", (2, 0, 0, 2, 0, [0, 2], ["a", "b"], ["<del>", "<del>"])),
    ("", "", (0, 0, 0, 0, 0, [], [], [])),
    # the leftover rule: the hypothesis runs out first, the two reference tokens in front are booked at position 0
    ("c", "abc", (2, 1, 2, 0, 0, [2], ["<ins>", "<ins>", "c"], ["a", "b", "c"])),
    ("abc", "c", (2, 1, 0, 2, 0, [0, 2, 0], ["a", "b", "c"], ["<del>", "<del>", "c"])),
]


@pytest.mark.parametrize("hyp,ref,want", HAND)
def test_restated_editdist_on_hand_cases(hyp, ref, want):
    got = em.editdist_restated(hyp, ref)
    assert got[:5] == want[:5]
    assert got[5].tolist() == want[5] and got[6] == want[6] and got[7] == want[7]


def test_editDist_derivation_from_a_path_equals_the_restatement():
    """stanford-ctc_amd/editDist.py reads everything beyond the counts off the forward path: the same here
    with the model's path in place of the device's"""
    import editDist
    rs = np.random.RandomState(2)
    cases = [(list(h), list(r)) for h, r, _ in HAND]
    for a, b in em.random_pairs(6, 400, 12, [2, 3, 6]):
        cases.append((["w%d" % v for v in a], ["w%d" % v for v in b]))
    for hyp, ref in cases:
        table = {}
        ids = [[table.setdefault(t, len(table)) for t in s] for s in (hyp, ref)]
        stats, path = em.edit_model(ids[0], ids[1])
        got = editDist._derive(hyp, ref, stats, path)
        want = em.editdist_restated(hyp, ref)
        assert got[:5] == want[:5], (hyp, ref)
        assert np.array_equal(got[5], want[5]) and got[5].dtype == want[5].dtype, (hyp, ref, got[5], want[5])
        assert got[6] == want[6] and got[7] == want[7], (hyp, ref)
    assert editDist.ref_to_hyp(["s", "<ins>", "<ins>", "u"], ["s", "a", "t", "u"]) == [0, 1, 1, 1]


def edit_cfg(sctc, a_len, b_len, flags=0, a_off=None, b_off=None):
    al, bl = np.array(a_len, dtype=np.int32), np.array(b_len, dtype=np.int32)
    ao = np.array(a_off if a_off is not None else np.concatenate([[0], np.cumsum(al)[:-1]]), dtype=np.int64)
    bo = np.array(b_off if b_off is not None else np.concatenate([[0], np.cumsum(bl)[:-1]]), dtype=np.int64)
    cfg = sctc.EditConfig(len(al), flags, sctc.i32(al), sctc.i64(ao), sctc.i32(bl), sctc.i64(bo))
    return cfg, (al, bl, ao, bo)        # the arrays must outlive the call


def test_argument_errors_need_no_gpu(sctc):
    L = sctc.lib()
    n = ctypes.c_size_t(7)
    fake = ctypes.c_void_p(4096)        # never dereferenced: every call below fails before the device is touched
    assert L.sctc_edit_distance_workspace_bytes(None, ctypes.byref(n)) == -1 and n.value == 0
    assert L.sctc_edit_distance_batch(None, fake, fake, fake, None, None, None, 0, None) == -1
    cfg, keep = edit_cfg(sctc, [3, 8191], [8191, 0])
    assert L.sctc_edit_distance_workspace_bytes(ctypes.byref(cfg), ctypes.byref(n)) == 0 and n.value == 0
    assert L.sctc_edit_distance_workspace_bytes(ctypes.byref(cfg), None) == -1
    cfg, keep = edit_cfg(sctc, [40, 8191], [8191, 0], sctc.EDIT_OPS)
    assert L.sctc_edit_distance_workspace_bytes(ctypes.byref(cfg), ctypes.byref(n)) == 0
    assert 10 * 2048 * 4 <= n.value <= 10 * 2048 * 4 + 256    # 40 x 8191: ten groups of four rows, 2048 words each; n x 0: none
    # the table of a pair that fits a wave's share of on-chip memory needs no workspace
    cfg, keep = edit_cfg(sctc, [200], [200], sctc.EDIT_OPS)
    assert L.sctc_edit_distance_workspace_bytes(ctypes.byref(cfg), ctypes.byref(n)) == 0 and n.value == 0
    cfg, keep = edit_cfg(sctc, [1100], [1100], sctc.EDIT_OPS)
    assert L.sctc_edit_distance_workspace_bytes(ctypes.byref(cfg), ctypes.byref(n)) == 0
    assert 275 * 275 * 4 <= n.value <= 275 * 275 * 4 + 256
    # SCTC_ERR_WORKSPACE before the device is touched
    assert L.sctc_edit_distance_batch(ctypes.byref(cfg), fake, fake, fake, fake, fake, fake, n.value - 1, None) == -3
    assert b"workspace" in L.sctc_last_error()
    assert L.sctc_edit_distance_batch(ctypes.byref(cfg), fake, fake, fake, fake, fake, None, 0, None) == -3
    for bad in ([3, 8192], [-1, 2]):
        for flip in (False, True):
            cfg, keep = edit_cfg(sctc, [1, 1] if flip else bad, bad if flip else [1, 1], a_off=[0, 1], b_off=[0, 1])
            assert L.sctc_edit_distance_workspace_bytes(ctypes.byref(cfg), ctypes.byref(n)) == -1
            assert L.sctc_edit_distance_batch(ctypes.byref(cfg), fake, fake, fake, None, None, None, 0, None) == -1
            assert b"outside 0..8191" in L.sctc_last_error()
    cfg, keep = edit_cfg(sctc, [1, 1], [1, 1], a_off=[0, -1])
    assert L.sctc_edit_distance_batch(ctypes.byref(cfg), fake, fake, fake, None, None, None, 0, None) == -1
    cfg, keep = edit_cfg(sctc, [1, 1], [1, 1], b_off=[-5, 0])
    assert L.sctc_edit_distance_batch(ctypes.byref(cfg), fake, fake, fake, None, None, None, 0, None) == -1
    assert b"negative offset" in L.sctc_last_error()
    cfg, keep = edit_cfg(sctc, [1], [1])
    cfg.P = -1
    assert L.sctc_edit_distance_batch(ctypes.byref(cfg), fake, fake, fake, None, None, None, 0, None) == -1
    cfg, keep = edit_cfg(sctc, [1], [1], flags=2)
    assert L.sctc_edit_distance_batch(ctypes.byref(cfg), fake, fake, fake, None, None, None, 0, None) == -1
    cfg = sctc.EditConfig(1, 0, None, None, None, None)
    assert L.sctc_edit_distance_batch(ctypes.byref(cfg), fake, fake, fake, None, None, None, 0, None) == -1
    # missing output pointers
    cfg, keep = edit_cfg(sctc, [2], [2])
    assert L.sctc_edit_distance_batch(ctypes.byref(cfg), fake, fake, None, None, None, None, 0, None) == -1
    assert L.sctc_edit_distance_batch(ctypes.byref(cfg), None, fake, fake, None, None, None, 0, None) == -1
    cfg, keep = edit_cfg(sctc, [2], [2], sctc.EDIT_OPS)
    assert L.sctc_edit_distance_batch(ctypes.byref(cfg), fake, fake, fake, None, fake, None, 0, None) == -1
    assert L.sctc_edit_distance_batch(ctypes.byref(cfg), fake, fake, fake, fake, None, None, 0, None) == -1
    # P == 0: nothing to do, nothing launched, no pointer looked at
    cfg = sctc.EditConfig(0, 0, None, None, None, None)
    assert L.sctc_edit_distance_batch(ctypes.byref(cfg), None, None, None, None, None, None, 0, None) == 0
    assert L.sctc_edit_distance_workspace_bytes(ctypes.byref(cfg), ctypes.byref(n)) == 0 and n.value == 0
    # the Python surface checks before it needs a device
    import ctc_fast
    assert ctc_fast.edit_distance_batch([], []).shape == (0, 5)
    with pytest.raises(ValueError):
        ctc_fast.edit_distance_batch([[1]], [[1], [2]])
    with pytest.raises(ValueError):
        ctc_fast.edit_distance_batch([np.zeros(8192, np.int32)], [[1]])
    with pytest.raises(ValueError):
        ctc_fast.edit_distance_batch([[1.5]], [[1]])
    with pytest.raises(ValueError):
        ctc_fast.edit_distance_batch([[2 ** 31]], [[1]])
    with pytest.raises(ValueError):
        ctc_fast.edit_distance_batch([[1]], [[1]], a_index=[1])


def test_no_cpu_fallback(sctc):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    import ctc_fast
    import editDistance
    with pytest.raises(sctc.SctcError):
        ctc_fast.edit_distance_batch([[1, 2]], [[1]])
    with pytest.raises(sctc.SctcError):
        editDistance.edit_distance("ab", "a")


def test_struct_mirror_matches_the_header(sctc, tmp_path):
    prog = tmp_path / "sz.c"
    prog.write_text(
        '#include <stdio.h>\n#include <stddef.h>\n#include "sctc.h"\n'
        'int main(void){printf("%zu %zu %zu %zu %zu %zu %zu %d\\n", sizeof(sctc_edit_config),'
        ' offsetof(sctc_edit_config, P), offsetof(sctc_edit_config, flags), offsetof(sctc_edit_config, a_len),'
        ' offsetof(sctc_edit_config, a_off), offsetof(sctc_edit_config, b_len), offsetof(sctc_edit_config, b_off),'
        ' SCTC_EDIT_OPS); return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    E = sctc.EditConfig
    assert got == [ctypes.sizeof(E), E.P.offset, E.flags.offset, E.a_len.offset, E.a_off.offset, E.b_len.offset,
                   E.b_off.offset, sctc.EDIT_OPS]
