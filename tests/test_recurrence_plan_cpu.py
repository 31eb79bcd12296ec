"""Which recurrent kernel a shape gets and how a minibatch is cut (csrc/recurrent_plan.h), checked without a GPU.

The header is pure host code: tests/rec_plan_dump.cpp prints its decisions, compiled here with g++.
  * tests/data/rec_plan_parent.txt holds the decisions of the hand-written launcher this header replaced (commit
    1cbab82), recorded from that launcher itself: its recurrent.hip compiled for the host with launch_persistent /
    launch_fallback replaced by printers that report "not launched", so that every candidate is walked, each kernel
    named by its demangled host symbol.  Layer sizes 96..4096, 14 minibatch sizes, all 16 variants x operand type,
    SCTC_REC_TCFG 0..3, BPTT with 16-bit operands, a device of 32 CUs, and the cuts of 16 minibatch sizes: 4018
    launches and 1568 minibatches, stored with equal candidate lists written once.  The header's decisions must
    equal it line by line.
  * values of SCTC_REC_VARIANT that name nothing are rejected;
  * every row of exact_net.GPU_CASES gets, as its first candidate on a device of 256 CUs, the kernel family its id
    names, and the cut rows the launch sizes their comments state.
"""
import os
import subprocess

import pytest

from tests import exact_net

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "stanford-ctc_amd", "csrc")
RECORDED = os.path.join(ROOT, "tests", "data", "rec_plan_parent.txt")


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("rec_plan") / "rec_plan_dump")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", CSRC,
                           os.path.join(ROOT, "tests", "rec_plan_dump.cpp"), "-o", exe])
    return exe


def launches(dump, queries):
    """queries: (Hp, B, prec16, variant, cus) -> per query the list of (nb, family, linear_map, kernel name), or
    "rejected" """
    text = "".join("%d %d %d %d %d\n" % q for q in queries)
    out = subprocess.run([dump, "launches"], input=text, stdout=subprocess.PIPE, check=True,
                         universal_newlines=True).stdout.splitlines()
    res, cur = [], []
    for line in out:
        if line == "end":
            res.append(cur)
            cur = []
        elif line == "rejected":
            cur = "rejected"
        else:
            nb, family, linear_map, name = line.split(" ", 3)
            cur.append((int(nb), family, int(linear_map), name))
    assert len(res) == len(queries)
    return res


HP = [96, 512, 1024, 1824, 1856, 2048, 4096]
BS = [1, 3, 4, 5, 6, 8, 16, 17, 32, 33, 64, 65, 96, 128]
VS = [0, 1, 2, 3, 5, 6, 7, 40, 43, 44, 45, 46, 47, 49, 50, 51]
CB = [32, 33, 40, 48, 49, 64, 65, 72, 80, 81, 96, 97, 128, 129, 150, 300]
CV = [0, 1, 40, 45, 47, 50]
# (prec16, transpose, variant, tcfg, cus) of the entries of a "plan Hp B:" row / (prec16, variant, cus) of a "cut" row
PLAN_COLUMNS = ([(p16, 0, v, 0, 256) for v in VS for p16 in (0, 1)] + [(1, 1, 0, 0, 256)] + [(p16, 0, 0, 0, 32) for p16 in (0, 1)]
                + [(p16, 0, 0, tcfg, 256) for tcfg in (1, 2, 3) for p16 in (0, 1)])
CUT_COLUMNS = [(p16, v, 256) for v in CV for p16 in (0, 1)] + [(p16, 0, 32) for p16 in (0, 1)]


def recorded_lines():
    """tests/data/rec_plan_parent.txt expanded to what `rec_plan_dump grid` prints"""
    bodies, plans, cuts = {}, {}, {}
    for line in open(RECORDED).read().splitlines():
        if line.startswith("P"):
            name, body = line.split(" = ")
            bodies[name[1:]] = body.split(" | ")
        elif line.startswith(("plan ", "cut ")):
            head, entries = line.split(": ")
            kind, Hp, B = head.split()
            (plans if kind == "plan" else cuts)[int(Hp), int(B)] = entries.split()
    assert sorted(plans) == sorted((H, B) for H in HP for B in BS) and sorted(cuts) == sorted((H, B) for H in HP for B in CB)
    out = []
    for tcfg in (0, 1, 2, 3):
        for Hp in HP:
            for B in BS:
                assert len(plans[Hp, B]) == len(PLAN_COLUMNS)
                for (p16, tr, v, tc, cus), ref in zip(PLAN_COLUMNS, plans[Hp, B]):
                    if tc != tcfg:
                        continue
                    out.append("plan %d %d %d %d %d %d %d" % (Hp, B, p16, tr, v, tc, cus))
                    for c in bodies[ref]:
                        out.append(" " + (c[:-1] + str(v) if c.endswith(" v") else c))
        if tcfg == 0:
            for cus in (256, 32):
                for Hp in HP:
                    for B in CB:
                        assert len(cuts[Hp, B]) == len(CUT_COLUMNS)
                        out += ["cut %d %d %d %d %d: %s" % (Hp, B, p16, v, cu, sizes.replace("+", " "))
                                for (p16, v, cu), sizes in zip(CUT_COLUMNS, cuts[Hp, B]) if cu == cus]
    return out


def test_decisions_equal_the_recorded_launcher(dump):
    got = subprocess.check_output([dump, "grid"], universal_newlines=True).splitlines()
    want = recorded_lines()
    assert sum(l.startswith("plan ") for l in want) == 7 * 14 * (16 * 2 + 1 + 2 + 3 * 2)
    assert sum(l.startswith("cut ") for l in want) == 7 * 16 * (6 * 2 + 2)
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        if g != w:
            head = max(j for j in range(i + 1) if want[j].startswith(("plan ", "cut ")))
            raise AssertionError("line %d: got %r, recorded %r (under %r)" % (i + 1, g, w, want[head]))


@pytest.mark.parametrize("variant", [4, 8, 23, 42, 48, -1, 99])
def test_unknown_variants_are_rejected(dump, variant):
    res = launches(dump, [(H, B, 0, variant, 256) for H in (96, 1824) for B in (1, 24, 150)])
    assert all(r == "rejected" for r in res)
    assert launches(dump, [(1824, 24, 0, 0, 256)])[0] != "rejected"


def _args(name):
    return name[name.index("<") + 1:-1].split(", ")


# path of a GPU_CASES id -> what its launches must be: a list of (utterances or None, check of (family, linear_map, name))
def _expected(c):
    Hp = -(-c.H // 32) * 32
    q1 = lambda f, lm, n: f == "Q" and lm == 1
    q2 = lambda f, lm, n: f == "Q" and lm == 0
    s = lambda sb: (lambda f, lm, n: f == "S" and _args(n) == [str(Hp // 32), str(sb)])
    t = lambda nt, ug: (lambda f, lm, n: f == "T" and _args(n)[2] == str(nt) and _args(n)[7] == str(ug))
    slab = lambda ntw, known: (lambda f, lm, n: f == "SLAB" and _args(n)[:2] == [str(ntw), str(Hp // 32 if known else 0)])
    fallback = lambda f, lm, n: f == "FALLBACK" and n == "brnn_recurrent_step_kernel"
    ntw = 1 if c.B <= 32 else (2 if c.B <= 64 else 4)
    return {
        "s4": [(c.B, s(4))], "s8": [(c.B, s(8))], "q1": [(c.B, q1)], "q2": [(c.B, q2)],
        "mh": [(c.B, lambda f, lm, n: f == "MH" and _args(n)[1] == "false")],
        "t-ug1": [(c.B, t(1, 1))], "t-1tile": [(c.B, t(1, 2))], "t-2tile": [(c.B, t(2, 2))],
        "t-cut64": [(64, t(1, 2)), (16, q1)], "t-nocut": [(80, t(2, 2))],
        "t-small": [(c.B, t(1 if c.B <= 64 else 2, 2))],
        "slab": [(c.B, slab(ntw, True))],
        "cut32": [(32, q2), (8, q1)],
        "generic": [(32, slab(1, False)), (8, slab(1, False))] if c.B == 40 else [(c.B, slab(ntw, False))],
        "fallback": [(c.B, fallback)],
        "two-launches": [(128, slab(4, False)), (22, slab(1, False))],
        "below-tl": [(c.B, slab(1, False))],
        "bf16x3": [(c.B, q1)],
    }[c.path]


def test_gpu_cases_get_the_kernel_their_id_names(dump):
    """closes the gap tests/test_gpu_recurrence_exact.py names: which kernel a row of its matrix runs"""
    cases = exact_net.GPU_CASES
    res = launches(dump, [(-(-c.H // 32) * 32, c.B, int(c.mode == "f16"), int(c.variant), 256) for c in cases])
    seen = set()
    for c, got in zip(cases, res):
        want = _expected(c)
        assert [g[0] for g in got] == [w[0] for w in want], (c.id, got)
        for (nb, family, linear_map, name), (_, check) in zip(got, want):
            assert check(family, linear_map, name), (c.id, nb, family, linear_map, name)
        seen.add(c.path)
    sizes = {c.id: [g[0] for g in got] for c, got in zip(cases, res)}
    assert sizes["cut32-H512-B40-v0-f32"] == [32, 8] and sizes["t-cut64-H1824-B80-v0-f32"] == [64, 16]
    assert sizes["t-nocut-H1824-B80-v45-f32"] == [80] and sizes["two-launches-H64-B150-v0-f32"] == [128, 22]
    assert len(seen) == 18
