"""How sctc_intern_words_batch and sctc_nbest_mbr_batch lay out their workspaces and choose their launches
(csrc/nbest_mbr_plan.h), checked without a GPU.

The header is pure host code: tests/mbr_plan_dump.cpp prints its decisions, compiled here with g++.
  * interning: row n owns the slots from sum ceil(U / 2) of the rows before; a group's table is a power of two of at
    least twice its slots, none for a group without slots, and the tables do not overlap; the slices are the
    documented ones, rounded to 256 bytes, and the 0xff fill covers exactly meta and table;
  * MBR: the bound of a row is U (characters) or ceil(U / 2) (words), 0 beyond K_b; every utterance appears once,
    those whose LDS slot fits 16 KB first; pair numbers run through each launch; an utterance's confidence slots start
    at the sum of the longest bounds before it IN THE CALLER'S ORDER; the LDS slots cover the largest pair of their
    launch; an operation table goes to the workspace exactly when it does not fit behind the panel edge.
"""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "stanford-ctc_amd", "csrc")
DUMP_SRC = os.path.join(ROOT, "tests", "mbr_plan_dump.cpp")
CHARS, WORDS = 0, 1
CONF, DIST = 1, 2
SLOT_MAX, STAT, PANEL = 16384, 32, 256


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("mbr_plan") / "mbr_plan_dump")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", CSRC, DUMP_SRC, "-o", exe])
    return exe


def a256(v):
    return (v + 255) // 256 * 256


def a16(v):
    return (v + 15) // 16 * 16


def run(dump, line):
    out = subprocess.run([dump], input=line + "\n", capture_output=True, text=True, check=True).stdout.splitlines()
    assert out[-1] == "end"
    rec = {}
    for l in out[:-1]:
        k, *v = l.split()
        rec.setdefault(k, []).append([int(x) for x in v])
    return rec


INTERN = {
    "empty": ([], [0]),
    "no_groups_rows": ([], [0, 0, 0]),
    "one": ([7], [0, 1]),
    "zeros": ([0, 0, 0], [0, 2, 3]),
    "ragged": ([int(u) for u in np.random.RandomState(1).randint(0, 60, size=90)], [0, 1, 1, 40, 41, 90]),
    "longest": ([4095, 0, 4095, 1], [0, 2, 4]),
    "pairs": ([5, 6] * 30, list(range(0, 61, 2))),
}


@pytest.mark.parametrize("name", sorted(INTERN))
def test_intern_plan(dump, name):
    U, g = INTERN[name]
    N, G = len(U), len(g) - 1
    r = run(dump, "intern %d %d %s %s" % (N, G, " ".join(map(str, U)), " ".join(map(str, g))))
    per = [(u + 1) // 2 for u in U]
    first = np.concatenate([[0], np.cumsum(per)]).astype(np.int64)
    rows = r.get("row", [])
    assert [x[0] for x in rows] == list(range(N))
    tab_at, spans = 0, []
    for q in range(G):
        s = sum(per[g[q]:g[q + 1]])
        cap = 0
        if s:
            cap = 2
            while cap < 2 * s:
                cap *= 2
            assert cap >= 2 * s and cap < 4 * s + 2
        for n in range(g[q], g[q + 1]):
            assert rows[n][1:] == [U[n], 1000 * n, first[n], tab_at, max(cap - 1, 0)]
        spans.append((tab_at, tab_at + cap))
        tab_at += cap
    assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:]))
    assert r.get("group", []) == [[g[q], g[q + 1]] for q in range(G)]
    assert r["slots"] == [[int(first[-1]), tab_at]]
    want = [0]
    for size in (32 * N, 8 * G):
        want.append(want[-1] + a256(size))
    head = want[-1]
    for size in (4 * N, 24 * int(first[-1]), 4 * tab_at):
        want.append(want[-1] + a256(size))
    off_rows, off_groups, head_b, off_base, off_meta, off_table, fill, total = r["off"][0]
    assert [off_rows, off_groups, off_base, off_meta, off_table, total] == want
    assert head_b == head == off_base and fill == total - off_meta


def _ragged(B, K, hi, seed):
    rs = np.random.RandomState(seed)
    return [int(k) for k in rs.randint(0, K + 1, size=B)], [int(u) for u in rs.randint(0, hi, size=B * K)]


MBR = {
    "one": (1, 1, [1], [5]),
    "no_real": (2, 3, [0, 0], [4] * 6),
    "small": (3, 4, [4, 2, 3], [3, 0, 7, 9, 1, 1, 1, 1, 260, 2, 300, 8]),
    "ragged": (17, 9) + _ragged(17, 9, 50, 3),
    "k256": (2, 256) + _ragged(2, 256, 5, 4),
    "panel": (2, 2, [2, 2], [257, 257, 300, 5]),
    "table_ws": (2, 2, [2, 2], [256, 256, 130, 130]),        # 64 * 64 * 4 + 32 bytes do not fit; 33 * 33 * 4 do
    "alone": (3, 2, [2, 2, 2], [4095, 4095, 10, 12, 2045, 2044]),  # 32 + 8 * 4095 > 16 KB; 32 + 8 * 2045 > 16 KB too
    "alone_edge": (2, 2, [2, 2], [2044, 2044, 2045, 1]),       # 32 + 8 * 2044 = 16384 fits exactly
}


@pytest.mark.parametrize("name", sorted(MBR))
@pytest.mark.parametrize("unit", [CHARS, WORDS])
@pytest.mark.parametrize("flags", [0, CONF, DIST, CONF | DIST])
def test_mbr_plan(dump, name, unit, flags):
    B, K, Kb, U = MBR[name]
    P = B * K
    r = run(dump, "mbr %d %d %d %d %s %s" % (B, K, unit, flags, " ".join(map(str, Kb)), " ".join(map(str, U))))
    eff = [U[o] if o % K < Kb[o // K] else 0 for o in range(P)]
    bound = [(u + 1) // 2 for u in eff] if unit == WORDS else eff
    slot_first = np.concatenate([[0], np.cumsum([(u + 1) // 2 for u in eff])]).astype(np.int64)
    for o, (idx, row_off, bd) in enumerate(r["row"]):
        assert idx == o and bd == bound[o]
        assert row_off == (slot_first[o] if unit == WORDS else 1000 * o)
    longest = [max([bound[b * K + k] for k in range(Kb[b])] + [0]) for b in range(B)]
    conf_first = np.concatenate([[0], np.cumsum(longest)]).astype(np.int64)

    def need(b):
        return STAT + (8 * longest[b] if longest[b] > PANEL else 0)

    def table(b):
        return ((longest[b] + 3) // 4) ** 2 * 4

    utts = r["utt"]
    assert sorted(u[0] for u in utts) == list(range(B))
    n_common, pairs_common, pairs_alone, slot_c, slot_a, cslot_c, cslot_a, tab_stride, conf_slots = r["plan"][0]
    assert [need(u[0]) <= SLOT_MAX for u in utts] == [True] * n_common + [False] * (B - n_common)
    for part, total in ((utts[:n_common], pairs_common), (utts[n_common:], pairs_alone)):
        assert [u[0] for u in part] == sorted(u[0] for u in part)          # the caller's order within a launch
        run_ = 0
        for b, kb, pair_off, conf_off, lg in part:
            assert (kb, pair_off, conf_off, lg) == (Kb[b], run_, conf_first[b], longest[b])
            run_ += kb * (kb - 1) // 2
        assert run_ == total
    assert conf_slots == conf_first[-1]
    common, alone = [u[0] for u in utts[:n_common]], [u[0] for u in utts[n_common:]]
    assert slot_c == a16(max([need(b) for b in common] + [0])) <= SLOT_MAX
    assert slot_a == a16(max([need(b) for b in alone] + [0]))
    assert slot_a == 0 or SLOT_MAX < slot_a <= 64 * 1024
    if flags & CONF:
        on_chip = [need(b) + table(b) <= SLOT_MAX for b in range(B)]
        assert cslot_c == a16(max([need(b) + (table(b) if on_chip[b] else 0) for b in common] + [0])) <= SLOT_MAX
        assert cslot_a == a16(max([need(b) for b in alone] + [0]))
        assert tab_stride == a256(max([table(b) for b in range(B) if not on_chip[b]] + [0]))
    else:
        assert (cslot_c, cslot_a, tab_stride) == (0, 0, 0)
    n_slots = int(slot_first[-1])
    want = [0]
    for size in (8 * P, 32 * B, 4 * B, 4 * P):
        want.append(want[-1] + a256(size))
    off = r["off"][0]
    assert off[:4] == want[:4] and off[4] == want[4] == off[5]          # rows utts kb lens | head = status
    at = want[4]
    if unit == WORDS:
        at += a256(4 * P)
        assert off[6] == at
        at += a256(4 * n_slots)
        assert off[7] == at
        i = run(dump, "intern %d %d %s %s" % (P, B, " ".join(map(str, eff)), " ".join(str(b * K) for b in range(B + 1))))
        at += i["off"][0][-1]
    else:
        assert off[6] == off[7] == at
    assert off[8] == at
    if not flags & DIST:
        at += a256(4 * P * K)
    assert off[9] == at
    if flags & CONF:
        units = K * int(conf_first[-1])
        at += a256(8 * P)
        assert off[10] == at
        at += a256(8 * B)
        assert off[11] == at
        at += a256(units)
        assert off[12] == at
        at += a256(2 * units)
        assert off[13] == at
        at += P * tab_stride
    assert off[14] == at


def test_named_cases_take_the_paths_they_are_named_for(dump):
    def plan(name, unit=CHARS, flags=CONF):
        B, K, Kb, U = MBR[name]
        return run(dump, "mbr %d %d %d %d %s %s" % (B, K, unit, flags, " ".join(map(str, Kb)), " ".join(map(str, U))))["plan"][0]
    assert plan("panel")[3] == a16(32 + 8 * 300)                    # an edge in the common launch
    p = plan("table_ws")
    assert p[7] == a256(64 * 64 * 4) and p[5] == a16(32 + 33 * 33 * 4)
    p = plan("alone")
    assert p[0] == 1 and p[2] == 2 and p[4] == a16(32 + 8 * 4095)
    p = plan("alone_edge")
    assert p[0] == 1 and p[3] == 16384 and p[4] == a16(32 + 8 * 2045)
    assert plan("alone", unit=WORDS)[0] == 2                        # 1023 words fit, 2048 do not (next test)


def test_word_bound_of_the_longest_row(dump):
    # 4095 symbols are at most 2048 words: 32 + 8 * 2048 = 16416 bytes, just beyond the common launch's slot
    r = run(dump, "mbr 1 2 %d 0 2 4095 4095" % WORDS)
    assert r["plan"][0][0] == 0 and r["plan"][0][4] == a16(32 + 8 * 2048)
