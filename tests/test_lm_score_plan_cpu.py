"""How sctc_lm_score_batch walks a batch and lays out its workspace (csrc/lm_score_plan.h), checked without a GPU.

The header is pure host code: tests/lm_score_plan_dump.cpp prints its decisions, compiled here with g++.  For every
length list and LM kind:
  * every sequence has exactly one descriptor, with its own length, label offset and term offset (the sum of the
    lengths of the caller's earlier sequences);
  * recurrent LM: every sequence with labels sits in exactly one tile slot, the lengths run non-increasing through a
    tile (and through the whole order, stably: equal lengths keep the caller's order), a tile has 1..32 sequences and
    takes as many steps as its longest sequence has labels;
  * the other two kinds keep the caller's order, and the window LM has ceil(sum U / 32) tiles of positions;
  * resident = min(tiles, 512) and the bytes are the documented formula: every slice rounded up to 256 bytes --
    24 N | 16 tiles | 4 A | 4 sum U (only without a terms array) | resident * tile_bytes.
"""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "stanford-ctc_amd", "csrc")
DUMP_SRC = os.path.join(ROOT, "tests", "lm_score_plan_dump.cpp")
NGRAM, NN, RNN = 0, 1, 2
TILE, RESIDENT = 32, 512


def _ragged(n, seed):
    return [int(u) for u in np.random.RandomState(seed).randint(0, 41, size=n)]


LISTS = {
    "empty": [],
    "zeros": [0] * 5,
    "one": [7],
    "n31": _ragged(31, 1),
    "n32": _ragged(32, 2),
    "n33": _ragged(33, 3),
    "n65": _ragged(65, 4),
    "equal": [5] * 40,
    "ragged": _ragged(200, 5),
    "beyond_resident": [1 + (i % 3) for i in range(TILE * RESIDENT + 40)],   # 514 tiles of sequences
    "beyond_resident_positions": [40] * 420,                                  # 525 tiles of positions
    "longest": [8191, 0, 8191, 1],
}


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("lm_score_plan") / "lm_score_plan_dump")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", CSRC, DUMP_SRC, "-o", exe])
    return exe


def run(dump, kind, A, tile_bytes, terms_in_ws, U):
    line = "%d %d %d %d %d %s\n" % (kind, A, tile_bytes, int(terms_in_ws), len(U), " ".join(str(u) for u in U))
    out = subprocess.run([dump], input=line, capture_output=True, text=True, check=True).stdout.splitlines()
    assert out[-1] == "end"
    plan = [int(v) for v in out[0].split()[1:]]
    off = [int(v) for v in out[1].split()[1:]]
    seqs = [tuple(int(v) for v in l.split()[1:]) for l in out if l.startswith("seq ")]
    tiles = [tuple(int(v) for v in l.split()[1:]) for l in out if l.startswith("tile ")]
    return plan, off, seqs, tiles


def a256(v):
    return (v + 255) // 256 * 256


@pytest.mark.parametrize("name", sorted(LISTS))
@pytest.mark.parametrize("kind", [NGRAM, NN, RNN])
@pytest.mark.parametrize("terms_in_ws", [False, True])
def test_plan(dump, name, kind, terms_in_ws):
    U = LISTS[name]
    N, A = len(U), 35
    tile_bytes = 0 if kind == NGRAM else 70400
    (n_terms, n_tiles, resident, grid), off, seqs, tiles = run(dump, kind, A, tile_bytes, terms_in_ws, U)
    term_off = np.concatenate([[0], np.cumsum(U)]).astype(np.int64)
    assert n_terms == sum(U)
    # every sequence exactly once, with its own numbers
    assert sorted(s[0] for s in seqs) == list(range(N))
    for n, u, t_off, l_off in seqs:
        assert (u, t_off, l_off) == (U[n], term_off[n], 1000 * n)
    if kind == RNN:
        lens = [s[1] for s in seqs]
        assert lens == sorted(lens, reverse=True)
        for a, b in zip(seqs, seqs[1:]):
            if a[1] == b[1]:
                assert a[0] < b[0]                      # stable
        placed = []
        for first, cnt, steps in tiles:
            assert 1 <= cnt <= TILE
            members = seqs[first:first + cnt]
            assert len(members) == cnt
            ml = [m[1] for m in members]
            assert all(x >= y for x, y in zip(ml, ml[1:])) and min(ml) >= 1
            assert steps == max(ml) == ml[0]
            placed += [m[0] for m in members]
        assert sorted(placed) == [n for n in range(N) if U[n] > 0]      # once each, none without labels
        assert n_tiles == len(tiles) == (sum(1 for u in U if u > 0) + TILE - 1) // TILE
    else:
        assert [s[0] for s in seqs] == list(range(N)) and not tiles
        assert n_tiles == ((sum(U) + TILE - 1) // TILE if kind == NN else 0)
    if kind == NGRAM:
        assert resident == 0 and grid == (sum(U) + 255) // 256
    else:
        assert resident == grid == min(n_tiles, RESIDENT)
    want = [0]
    for size in (24 * N, 16 * len(tiles), 4 * A, 4 * sum(U) if terms_in_ws else 0):
        want.append(want[-1] + a256(size))
    want.append(want[-1] + resident * tile_bytes)
    assert off == want


def test_more_tiles_than_resident_blocks(dump):
    for kind, name in ((RNN, "beyond_resident"), (NN, "beyond_resident_positions")):
        (_, n_tiles, resident, grid), _, _, _ = run(dump, kind, 35, 1024, False, LISTS[name])
        assert n_tiles > RESIDENT and resident == grid == RESIDENT
