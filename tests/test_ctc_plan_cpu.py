"""Which CTC kernel a batch runs and how its workspace is laid out (csrc/ctc_plan.h), checked without a GPU.

The header is pure host code: tests/ctc_plan_dump.cpp prints its decisions, compiled here with g++.
  * tests/data/ctc_plan_parent.txt holds the decisions of the hand-written dispatch this header replaced (commit
    6d568d0: ctc_make_plan / run_ctc in capi_ctc.hip, ctc_lattice_shape, launch_fused_k / launch_fused_one, the NA
    expressions of three launchers), recorded from that code itself on the CPU: its capi_ctc.hip, ctc_fused.hip,
    ctc_fusedw.hip, ctc_kernels.hip and ctc_generic.hip compiled host-only (hipcc --cuda-host-only) and linked against
    a stand-in of the HIP runtime calls they make, which reports success, names every launched kernel by the demangled
    symbol the object registered for it, reads the slice offsets out of the kernel arguments and every utterance's
    lat_off out of the descriptor upload.  A driver called sctc_ctc_workspace_bytes and sctc_ctc_loss_batch under
    setenv for: rows of 2U+1 states on both sides of 128 / 256 / 512 / 1024 / 2048 and U = 1, batches on both sides of
    18 / 24 / 256 / 1025 utterances and 1, alphabets on both sides of 64 / 128 / 256, both dtypes, 33 switch settings
    (every switch alone at the values tests and tools use, and their combinations): 39204 calls at T = 1, stored with
    equal kernel lists written once; and three ragged batches (one with rows beyond 2048 states) under the same
    settings, stored with every lat_off, slice offset and the total bytes.  To repeat it: check that commit out, build
    the five sources as described, and print in the format of `ctc_plan_dump grid`.  The header's decisions must
    equal the table line by line.
  * every name of tests/test_gpu_ctc_paths.py's `path.ENV` reaches the kernel it names on every shape of its SHAPES,
    and the two through-the-network minibatches take the wide kernel by default and the lattice pair with
    SCTC_CTC_FUSED=0 -- what the GPU tests can only infer from numeric differences;
  * moving any one threshold in a copy of the header makes the table test fail;
  * SCTC_CTC_LAZY=1 selects the lattice kernel's lazy instantiation for float32 batches only, and the cases of
    tests/test_gpu_ctc_lazy.py and tests/test_gpu_ctc_entry.py reach the instantiations they claim to.
"""
import os
import subprocess

import numpy as np
import pytest

from tests import test_gpu_ctc_paths as paths

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "stanford-ctc_amd", "csrc")
RECORDED = os.path.join(ROOT, "tests", "data", "ctc_plan_parent.txt")
DUMP_SRC = os.path.join(ROOT, "tests", "ctc_plan_dump.cpp")

GRID_U = [1, 63, 64, 127, 128, 255, 256, 511, 512, 1023, 1024]
GRID_B = [1, 17, 18, 23, 24, 256, 257, 1024, 1025]
GRID_A = [64, 65, 128, 129, 256, 257]
N_SETS = 33


def _compile(exe, include_dir, opt="-O1"):
    subprocess.check_call(["g++", "-std=c++17", opt, "-Wall", "-Wextra", "-Werror", "-I", include_dir, DUMP_SRC, "-o", exe])
    return exe


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    return _compile(str(tmp_path_factory.mktemp("ctc_plan") / "ctc_plan_dump"), CSRC)


def _clean_env(extra=()):
    env = {k: v for k, v in os.environ.items() if not k.startswith("SCTC_CTC_")}
    env.update(extra)
    return env


@pytest.fixture(scope="module")
def recorded():
    """tests/data/ctc_plan_parent.txt expanded to what `ctc_plan_dump grid` prints"""
    bodies, plans, tail, sets = {}, {}, [], None
    for line in open(RECORDED).read().splitlines():
        if line.startswith("sets: "):
            sets = line.split()[1:]
        elif line.startswith("P") and " = " in line and not tail:
            name, body = line.split(" = ")
            bodies[name[1:]] = body.split(" | ")
        elif line.startswith("plan "):
            head, entries = line.split(": ")
            _, L, B, A = head.split()
            plans[int(L), int(B), int(A)] = entries.split()
        else:
            tail.append(line)
    assert len(sets) == N_SETS and sets[0] == "default"
    assert sorted(plans) == sorted((2 * U + 1, B, A) for U in GRID_U for B in GRID_B for A in GRID_A)
    out = []
    for U in GRID_U:
        for B in GRID_B:
            for A in GRID_A:
                refs = plans[2 * U + 1, B, A]
                assert len(refs) == 2 * N_SETS
                for dtype in (0, 1):
                    for i, name in enumerate(sets):
                        out.append("plan %d %d %d %d %s" % (2 * U + 1, B, A, dtype, name))
                        out += [" " + k for k in bodies[refs[dtype * N_SETS + i]]]
    assert sum(l.startswith("layout ") for l in tail) == 3 * 2 * N_SETS
    assert sum(l.startswith(" lat_off ") for l in tail) == sum(l.startswith(" bytes ") for l in tail) == 3 * 2 * N_SETS
    return out + tail


def _first_difference(got, want):
    for i, (g, w) in enumerate(zip(got, want)):
        if g != w:
            head = max(j for j in range(i + 1) if want[j].startswith(("plan ", "layout ")))
            return "line %d: got %r, recorded %r (under %r)" % (i + 1, g, w, want[head])
    return None if len(got) == len(want) else "%d lines, recorded %d" % (len(got), len(want))


def test_decisions_equal_the_recorded_dispatch(dump, recorded):
    got = subprocess.check_output([dump, "grid"], universal_newlines=True, env=_clean_env()).splitlines()
    assert sum(l.startswith("plan ") for l in recorded) == 11 * 9 * 6 * 2 * N_SETS
    assert _first_difference(got, recorded) is None, _first_difference(got, recorded)


def kernels(dump, env, queries):
    """queries: (B, A, dtype, max_L, max_T) -> per query the list of kernel template-ids under the switches `env`"""
    text = "".join("%d %d %d %d %d\n" % q for q in queries)
    out = subprocess.run([dump, "query"], input=text, stdout=subprocess.PIPE, check=True, universal_newlines=True,
                         env=_clean_env(env)).stdout.splitlines()
    res, cur = [], []
    for line in out:
        if line == "end":
            res.append(cur)
            cur = []
        else:
            cur.append(line.strip())
    assert len(res) == len(queries)
    return res


def _args(name):
    return name[name.index("<") + 1:-1].split(", ")


def _na(A):
    return 1 if A <= 64 else (2 if A <= 128 else 4)


def _fused_k(L):
    return 2 if L <= 128 else (4 if L <= 256 else 8)


def _is_lattice_pair(got, ri):
    return (len(got) == 2 and got[0].startswith("ctc_lattice_kernel<%s, " % ri) and _args(got[0])[4] == "false"
            and got[1].startswith("ctc_grad_kernel<%s, " % ri))


@pytest.mark.parametrize("name", sorted(paths.path.ENV))
def test_every_named_path_reaches_the_kernel_it_names(dump, name):
    """single utterances of every shape of test_gpu_ctc_paths.SHAPES, as ctc_loss (float64) and ctc_loss_batch on
    float32 probabilities present them.  One listed shape has 513 states, one more than the narrow fused kernel holds:
    there the "fused*" names run what the default dispatch runs for a single utterance, the lattice pair."""
    env = paths.path.ENV[name]
    assert set(env) <= set(paths.path.VARS)
    queries = [(1, A, dtype, 2 * U + 1, T) for A, T, U in paths.SHAPES for dtype in (0, 1)]
    dieted = 0
    for (B, A, dtype, L, T), got in zip(queries, kernels(dump, env, queries)):
        ri = "double" if dtype else "float"
        rows = "double" if dtype or name in ("fused64", "wide64") else "unsigned int"
        K, NA, tag = _fused_k(L), _na(A), (name, A, L, ri, got)
        if name.startswith("fused") and L > 512:
            assert _is_lattice_pair(got, ri), tag
        elif name.startswith("fused") or (name == "widemin1" and L <= 512):
            helpers_exist = (NA == 1 and rows == "unsigned int") if K == 8 else NA <= 2
            help_ = helpers_exist and name not in ("fused2w", "fused2wd")
            diet = name == "fused2wd" and ri == "float" and rows == "unsigned int" and K <= 4 and NA == 1
            dieted += diet
            assert got == ["ctc_fused_kernel<%s, %s, %d, %d, %s, %s>" % (ri, rows, K, NA, str(help_).lower(), str(diet).lower())], tag
        elif name.startswith("wide"):
            W = 8 if name == "wide8" else 4
            assert got == ["ctc_fusedw_kernel<%s, %s, %d, %d, %d>" % (ri, rows, 2 if L <= 128 * W else 4, NA, W)], tag
        elif name.startswith("lattice"):
            assert _is_lattice_pair(got, ri), tag
            if name != "lattice":        # the forced shapes: that many waves per direction
                assert _args(got[0])[3] == name[len("lattice"):], tag
        elif name.startswith("lazy"):
            # float32: the lattice kernel's lazy instantiation; float64 has none and keeps the reference's schedule -- on the
            # lattice pair as well: the switch turns the fused kernels off for either dtype
            assert len(got) == 2 and got[0].startswith("ctc_lattice_kernel<%s, " % ri), tag
            assert got[1].startswith("ctc_grad_kernel<%s, " % ri) and _args(got[0])[4] == ("false" if dtype else "true"), tag
            if name != "lazy":
                assert _args(got[0])[3] == name[len("lazy"):], tag
        else:
            assert name == "generic"
            assert got == ["ctc_lattice_generic_kernel<%s>" % ri, "ctc_grad_generic_kernel<%s>" % ri], tag
    assert (dieted > 0) == (name == "fused2wd")


def test_the_network_minibatches_take_the_wide_kernel_and_the_lattice_pair(dump):
    """test_wide_rows_through_the_network (25 utterances, label rows of at most 1201 states) and
    test_cfg5_rows_at_18_utterances_through_the_network (18 of 1601 states), float32 probabilities: "fused" = the
    default switches is the wide kernel, "lattice" the lattice + grad pair -- so their two runs differ in kernels"""
    rs = np.random.RandomState(12)
    Us = [int(rs.randint(300, 601)) for _ in range(25)]
    Ts = [int(u + rs.randint(60, 400)) for u in Us]
    assert 1024 < 2 * max(Us) + 1 <= 1201
    queries = [(25, 20, 0, 2 * max(Us) + 1, max(Ts)), (18, 33, 0, 1601, 8000)]
    for got in kernels(dump, paths.path.ENV["fused"], queries):
        assert got == ["ctc_fusedw_kernel<float, unsigned int, 4, 1, 8>"]
    for got in kernels(dump, paths.path.ENV["lattice"], queries):
        assert got == ["ctc_lattice_kernel<float, 4, 1, 8, false>", "ctc_grad_kernel<float, 16>"]
    # one utterance fewer than the 18: the lattice pair by default
    assert _is_lattice_pair(kernels(dump, {}, [(17, 33, 0, 1601, 8000)])[0], "float")


def test_the_bit_pinned_cases_reach_every_instantiation(dump):
    """tests/data/ctc_bits_parent.txt (test_outputs_are_bit_identical_to_the_recorded_parent): its cases run every value
    of every template parameter of the four kernel families but the lattice kernel's lazy schedule (SCTC_CTC_LAZY is
    not a path of path.ENV) -- of the lattice, gradient and generic kernels every instantiation -- with both blank
    positions, a skipping input, an empty band and T = 1 on every path"""
    cases = {c[0]: c for c in paths.bits_cases()}
    recorded = [cases[l.split()[0]] for l in paths.bits_recorded()]
    seen, per_path = set(), {}
    for which in sorted(set(c[1] for c in recorded)):
        mine = [c for c in recorded if c[1] == which]
        queries = [(1, A, int(dt == np.float64), 2 * U + 1, T) for _, _, A, T, U, _, dt, _ in mine]
        for c, got in zip(mine, kernels(dump, paths.path.ENV[which], queries)):
            seen.update(got)
        per_path[which] = mine
    for which, mine in per_path.items():
        assert {c[5] == 0 for c in mine} == {True, False}, which                          # both blank positions
        assert {"skip", "empty"} <= {c[7] for c in mine} and any(c[3] == 1 for c in mine), which
    want = set()
    for ri, st in (("float", "unsigned int"), ("float", "double"), ("double", "double")):
        for NA in (1, 2, 4):
            for K in (2, 4, 8):
                want.add("ctc_fused_kernel<%s, %s, %d, %d, false, false>" % (ri, st, K, NA))
                if (NA == 1 and st == "unsigned int") if K == 8 else NA <= 2:
                    want.add("ctc_fused_kernel<%s, %s, %d, %d, true, false>" % (ri, st, K, NA))
            for K, W in ((2, 4), (4, 4), (2, 8), (4, 8)):
                want.add("ctc_fusedw_kernel<%s, %s, %d, %d, %d>" % (ri, st, K, NA, W))
    want |= {"ctc_fused_kernel<float, unsigned int, %d, 1, false, true>" % K for K in (2, 4)}
    for ri in ("float", "double"):
        for NA in (1, 2, 4):
            for K, W in ((2, 1), (4, 1), (8, 1), (16, 1), (32, 1), (2, 4), (4, 4), (8, 4), (2, 8), (4, 8)):
                want.add("ctc_lattice_kernel<%s, %d, %d, %d, false>" % (ri, K, NA, W))
        want |= {"ctc_grad_kernel<%s, %d>" % (ri, NB) for NB in (4, 8, 16)}
        want |= {"ctc_lattice_generic_kernel<%s>" % ri, "ctc_grad_generic_kernel<%s>" % ri}
    assert seen <= want, sorted(seen - want)
    for family in sorted(set(n[:n.index("<")] for n in want)):
        for i in range(len(_args(next(n for n in want if n.startswith(family + "<"))))):
            values = lambda names: set(_args(n)[i] for n in names if n.startswith(family + "<"))
            assert values(seen) == values(want), (family, i, values(want) - values(seen))
    # the lattice, gradient and generic kernels: every instantiation
    assert not [n for n in want - seen if not n.startswith("ctc_fused")], sorted(want - seen)


def test_the_lazy_switch_selects_the_lazy_lattice_kernel_for_float32_only(dump):
    """SCTC_CTC_LAZY=1 ("switches"): float32 batches of up to 2048 states and 256 symbols get
    ctc_lattice_kernel<float, K, NA, W, true> with the K and W of ctc_lattice_shape and the fused kernels are off, whatever
    the batch size; float64 batches get no lazy kernel (the reference's schedule, on the lattice pair); beyond 2048 states
    or 256 symbols the generic kernels run and the switch does nothing"""
    env = paths.path.ENV["lazy"]
    queries = [(B, A, dtype, L, 50) for B in (1, 17, 24, 300, 1100) for A in (33, 65, 129, 256) for dtype in (0, 1)
               for L in (3, 128, 129, 256, 257, 512, 513, 1024, 1025, 2047)]
    for (B, A, dtype, L, T), got in zip(queries, kernels(dump, env, queries)):
        W = 1 if L <= 256 else (4 if L <= 1024 else 8)
        K = next(k for k in (2, 4, 8) if L <= 64 * W * k)
        ri = "double" if dtype else "float"
        assert got[0] == "ctc_lattice_kernel<%s, %d, %d, %d, %s>" % (ri, K, _na(A), W, "false" if dtype else "true"), (B, A, L, got)
        assert len(got) == 2 and got[1].startswith("ctc_grad_kernel<%s, " % ri)
    beyond = [(1, 33, 0, 2049, 50), (1, 257, 0, 65, 50)]
    assert kernels(dump, env, beyond) == kernels(dump, {}, beyond) == [["ctc_lattice_generic_kernel<float>",
                                                                       "ctc_grad_generic_kernel<float>"]] * 2


def _lazy_missing(dump, shapes):
    """what of the lazy lattice kernel's template parameters (path name, (A, T, U)) cases do NOT reach: (K, W) pairs of
    ctc_lattice_shape and values of NA"""
    seen = set()
    for which in sorted(set(w for w, _ in shapes)):
        queries = [(1, A, 0, 2 * U + 1, T) for w, (A, T, U) in shapes if w == which]
        for got in kernels(dump, paths.path.ENV[which], queries):
            assert got[0].startswith("ctc_lattice_kernel<float, ") and _args(got[0])[4] == "true", (which, got)
            seen.add(tuple(int(v) for v in _args(got[0])[1:4]))
    want_kw = {(2, 1), (4, 1), (8, 1), (16, 1), (32, 1), (2, 4), (4, 4), (8, 4), (2, 8), (4, 8)}
    return (want_kw - {(k, w) for k, _, w in seen}) | ({("NA", n) for n in (1, 2, 4)} - {("NA", n) for _, n, _ in seen})


def test_the_lazy_gpu_cases_reach_every_lazy_instantiation(dump):
    """tests/test_gpu_ctc_lazy.LAZY_SHAPES (its cases against the oracle) run the lazy schedule in every (K, W) of
    ctc_lattice_shape and with 1, 2 and 4 probability registers per frame; a list without its forced shapes, or without its
    wide alphabets, does not"""
    from tests import test_gpu_ctc_lazy as lazy
    assert _lazy_missing(dump, lazy.LAZY_SHAPES) == set()
    assert _lazy_missing(dump, [c for c in lazy.LAZY_SHAPES if c[0] != "lazy8"]) == {(2, 8)}
    assert _lazy_missing(dump, [c for c in lazy.LAZY_SHAPES if c[0] != "lazy1"]) == {(8, 1), (16, 1), (32, 1)}
    assert ("NA", 4) in _lazy_missing(dump, [c for c in lazy.LAZY_SHAPES if c[1][0] <= 128])


def _entry_missing(dump, cases):
    """kernel families, and values of NA per family that has the parameter, that (id, path, row, A, blank, dtype) cases
    of tests/test_gpu_ctc_entry.py do not reach with their seven-utterance batch"""
    seen = set()
    for _, which, row, A, _, dt in cases:
        U, T = paths._ROWS[row]
        seen.update(kernels(dump, paths.path.ENV[which], [(7, A, int(dt == np.float64), 2 * U + 1, T)])[0])
    missing = set()
    for family, na_at in (("ctc_fused_kernel", 3), ("ctc_fusedw_kernel", 3), ("ctc_lattice_kernel", 2), ("ctc_grad_kernel", None),
                          ("ctc_lattice_generic_kernel", None), ("ctc_grad_generic_kernel", None)):
        mine = [n for n in seen if n.startswith(family + "<")]
        if not mine:
            missing.add(family)
        elif na_at is not None:
            missing |= {(family, "NA", n) for n in (1, 2, 4)} - {(family, "NA", int(_args(n)[na_at])) for n in mine}
    if not any(n.startswith("ctc_lattice_kernel<float, ") and _args(n)[4] == "true" for n in seen):
        missing.add("the lazy schedule")
    if not any(n.startswith("ctc_fused_kernel<") and _args(n)[5] == "true" for n in seen):
        missing.add("the dieted fused kernel")
    return missing


def test_the_entry_cases_reach_every_kernel_family_and_register_count(dump):
    """tests/test_gpu_ctc_entry.CASES: every kernel family (fused with and without helper waves and dieted, wide, lattice
    in both schedules, gradient, the generic pair) and, of the three families with the parameter, NA = 1, 2 and 4; taking
    a path's rows away is noticed"""
    from tests import test_gpu_ctc_entry as entry
    assert _entry_missing(dump, entry.CASES) == set()
    assert _entry_missing(dump, [c for c in entry.CASES if not c[1].startswith("wide")]) >= {"ctc_fusedw_kernel"}
    assert _entry_missing(dump, [c for c in entry.CASES if c[1] != "generic"]) == {"ctc_lattice_generic_kernel",
                                                                                    "ctc_grad_generic_kernel"}
    assert ("ctc_fused_kernel", "NA", 4) in _entry_missing(dump, [c for c in entry.CASES if c[3] != 200])


# (text of csrc/ctc_plan.h, its replacement): each moves one threshold by one or two
MUTATIONS = [
    ("(s.max_L > 1024 ? 18 : 24)", "(s.max_L > 1024 ? 19 : 24)"),
    ("(s.max_L > 1024 ? 18 : 24)", "(s.max_L > 1024 ? 18 : 25)"),
    ("(s.max_L > 1024 ? 18 : 24)", "(s.max_L > 1026 ? 18 : 24)"),
    ("int helper_max_b = 256;", "int helper_max_b = 255;"),
    ("int diet_min_b = 1025;", "int diet_min_b = 1026;"),
    ("s.max_L <= 128 ? 2 :", "s.max_L <= 130 ? 2 :"),
    ("(s.max_L <= 256 ? 4 :", "(s.max_L <= 258 ? 4 :"),
    ("(s.max_L <= 512 ? 8 : 0)", "(s.max_L <= 514 ? 8 : 0)"),
    ("s.max_L > 2048 ||", "s.max_L > 2050 ||"),
    ("p.W = (s.max_L > 1024 ||", "p.W = (s.max_L > 1026 ||"),
    ("(force == 0 && max_L <= 256)", "(force == 0 && max_L <= 258)"),
    ("(force == 0 && max_L > 1024)", "(force == 0 && max_L > 1026)"),
    ("return A <= 64 ? 1 : (A <= 128 ? 2 : 4);", "return A <= 65 ? 1 : (A <= 128 ? 2 : 4);"),
    ("return A <= 64 ? 1 : (A <= 128 ? 2 : 4);", "return A <= 64 ? 1 : (A <= 129 ? 2 : 4);"),
    ("|| s.A > 256 ||", "|| s.A > 257 ||"),
    ("p.NB = p.lp <= 256 ? 4 :", "p.NB = p.lp <= 128 ? 4 :"),
    # (the layout half of the table: the pad in front of every utterance's packed rows)
    ("return p.K + (int64_t)T *", "return (int64_t)T *"),
]


@pytest.mark.parametrize("i", range(len(MUTATIONS)))
def test_a_moved_threshold_is_noticed(tmp_path, recorded, i):
    old, new = MUTATIONS[i]
    text = open(os.path.join(CSRC, "ctc_plan.h")).read()
    assert text.count(old) == 1, old
    text = text.replace(old, new).replace('"../../include/sctc.h"', '"%s"' % os.path.join(ROOT, "include", "sctc.h"))
    (tmp_path / "ctc_plan.h").write_text(text)
    exe = _compile(str(tmp_path / "ctc_plan_dump"), str(tmp_path), opt="-O0")
    got = subprocess.check_output([exe, "grid"], universal_newlines=True, env=_clean_env()).splitlines()
    assert _first_difference(got, recorded) is not None, (old, new)
