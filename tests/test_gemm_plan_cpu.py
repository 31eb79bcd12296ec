"""Which GEMM kernel a call runs, on which tile, with how many K slices and how much workspace (csrc/gemm_plan.h),
checked without a GPU.

The header is pure host code: tests/gemm_plan_dump.cpp prints its decisions, compiled here with g++.
  * tests/data/gemm_plan_parent.txt holds the decisions of the dispatch this header replaced (commit d0bf19b:
    gemm_pick_shape / gemm_plan_splits / launch_tiles / launch_gemm_f32 in gemm_f32.hip, h16_pick_big /
    gemm_h16_plan_splits / launch_h16 / launch_gemm_h16_tiles in gemm_h16.hip, gemm_g16_applies / launch_gemm_g16 in
    gemm_g16.hip, gemm_s3_plan_splits / launch_gemm_s3 in gemm_s3.hip), recorded from that code itself on the CPU: its
    four GEMM sources compiled host-only (hipcc --cuda-host-only) and linked against a stand-in of the HIP runtime
    calls they make, which reports success and names every launched kernel by the demangled symbol the object
    registered for it, with block size, dynamic LDS bytes and grid.x.  A driver, one process per setting (that code
    read SCTC_G16 once per process), called launch_gemm_f32 with splits = 1 on never-dereferenced aligned pointers
    and leading dimensions of 8, and gemm_plan_splits(M, N, K, prec, in16 && a_kcontig == b_kcontig && !idx_a) -- the
    approximation of in16 that code's callers passed -- for the queries `gemm_plan_dump queries` lists: every layout,
    gather, A2 and precision (the illegal combinations with their messages) on four shapes under 22 settings of
    SCTC_GEMM_SHAPE / SCTC_H16_TILE / SCTC_G16 and their pairs; M and N on both sides of one and two multiples of
    64 / 96 / 128 / 256; K on both sides of 8 and 64 K tiles and of 4096 on outputs around every tile-count and
    padding threshold; every GEMM of the five BASELINE.json configurations.  Equal launch descriptions are stored
    once.  To repeat it: check that commit out, build the four sources as described, and print in the format of
    `gemm_plan_dump grid`.  The header's decisions must equal the table line by line.
  * moving any one threshold in a copy of the header makes the table test fail;
  * the split-K workspace the engine sizes at create time (brnn_splitk_floats) against every plan its five launch
    sites can make: the five configurations and 125 small networks, both recurrent weight-gradient forms, every frame
    count next to a K-tile edge up to max_frames, three operand types -- 20.5 million plans.  Every weight-gradient
    plan fits (those launches took the planned split unchecked before the engine had one helper).  771108 forward /
    delta plans do not, every one of them above the rule's cap of 2 * 1024 * 128 * 128 floats (the first: cfg-3,
    1327 frames, 1327 x 1824 x 1824, 14 slices, 33904850 floats): they run unsplit, as they did, by that cap's design;
  * tests/gemm_cases.py's hand-kept tile table (case_tile) agrees with the plan for every case of every implementation;
  * the GEMM sources read the environment and raise the dynamic-LDS limit in one place each.
"""
import os
import re
import subprocess

import pytest

from tests import gemm_cases as gc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "stanford-ctc_amd", "csrc")
RECORDED = os.path.join(ROOT, "tests", "data", "gemm_plan_parent.txt")
DUMP_SRC = os.path.join(ROOT, "tests", "gemm_plan_dump.cpp")
SWITCHES = ("SCTC_GEMM_SHAPE", "SCTC_H16_TILE", "SCTC_G16")


def _compile(exe, include_dir, opt="-O1"):
    subprocess.check_call(["g++", "-std=c++17", opt, "-Wall", "-Wextra", "-Werror", "-I", include_dir, DUMP_SRC, "-o", exe])
    return exe


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    return _compile(str(tmp_path_factory.mktemp("gemm_plan") / "gemm_plan_dump"), CSRC)


def _clean_env(extra=()):
    env = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    env.update(extra)
    return env


@pytest.fixture(scope="module")
def recorded():
    """tests/data/gemm_plan_parent.txt expanded to what `gemm_plan_dump grid` prints"""
    sets, bodies, out = {}, {}, []
    for line in open(RECORDED).read().splitlines():
        if line.startswith("#"):
            continue
        if line.startswith("sets "):
            head, names = line.split(": ")
            sets[int(head.split()[1])] = names.split()
        elif line.startswith("B"):
            name, body = line.split(" = ")
            bodies[name[1:]] = body
        else:
            q, entries = line.split(": ")
            M, N = (int(v) for v in q.split()[1:3])
            expanded = []
            for tok in entries.split():
                m = re.fullmatch(r"(\d+)/(\d*)/(\d+)(?:x(\d+))?", tok)
                expanded += [m.group(1, 2, 3)] * int(m.group(4) or 1)
            for name, (ref, grid, s) in zip(sets[len(expanded)], expanded):
                launch = bodies[ref] + (" grid " + grid if grid else "")
                ws = int(s) * M * (N + 1) if int(s) > 1 else 0
                out.append("%s %s | %s | splits %s ws %d" % (q, name, launch, s, ws))
    assert sorted(sets) == [1, 5, 6, 22] and sets[22][0] == "default"
    return out


def _first_difference(got, want):
    for i, (g, w) in enumerate(zip(got, want)):
        if g != w:
            return "line %d: got %r, recorded %r" % (i + 1, g, w)        # a line starts with its query and setting
    return None if len(got) == len(want) else "%d lines, recorded %d" % (len(got), len(want))


def test_decisions_equal_the_recorded_dispatch(dump, recorded):
    got = subprocess.check_output([dump, "grid"], universal_newlines=True, env=_clean_env()).splitlines()
    assert len(recorded) == 26306 and sum(" | rejected: " in l for l in recorded) == 6688
    assert _first_difference(got, recorded) is None, _first_difference(got, recorded)


# (text of csrc/gemm_plan.h, its replacement): each moves one threshold
MUTATIONS = [
    ("GemmShape{128, 96, SCTC_GEMM_OCC1, 0.02}", "GemmShape{128, 96, SCTC_GEMM_OCC1, 0.03}"),
    ("GemmShape{64, 128, 4, 0.10}", "GemmShape{64, 128, 4, 0.12}"),
    ("GemmShape{128, 64, 4, 0.10}", "GemmShape{128, 64, 4, 0.08}"),
    ("big <= 1.06 * small", "big <= 1.02 * small"),
    ("big <= 1.06 * small", "big <= 1.15 * small"),
    ("big <= 1.25 * small", "big <= 1.35 * small"),
    ("big <= 1.25 * small", "big <= 1.10 * small"),
    ("return tiles_big >= 32 &&", "return tiles_big >= 33 &&"),
    ("K >= 4096 && tiles_big >= 8 &&", "K >= 4096 && tiles_big >= 9 &&"),
    ("K >= 4096 && tiles_big >= 8 &&", "K >= 4097 && tiles_big >= 8 &&"),
    ("- 0.002 * c;", "- 0.003 * c;"),
    ("- 0.002 * c;", "- 0.001 * c;"),
    ("min_ktiles = 8;", "min_ktiles = 9;"),
    ("split_bk = GEMM_SPLIT_BK16, min_ktiles = 4;", "split_bk = GEMM_SPLIT_BK16, min_ktiles = 5;"),
    ("GEMM_SPLIT_BK16 = 64;", "GEMM_SPLIT_BK16 = 32;"),
    ("if (tiles < 2 * slots) {", "if (tiles < 1 * slots) {"),
    ("by_k > 64 ? 64 : by_k", "by_k > 63 ? 63 : by_k"),
    ("p.occ = split_big ? 1 : 2;", "p.occ = split_big ? 1 : 3;"),
    # the hint / exact pair of the 16-bit tile choice (GemmPlan::split_tile_differs)
    ("const bool split_big = gemm_h16_pick_big(q.M, q.N, q.K, hint, sw);", "const bool split_big = gemm_h16_pick_big(q.M, q.N, q.K, g16, sw);"),
    ("(q.a_kcontig ? q.K % 8 == 0 : (q.M % 8 == 0 && q.N % 8 == 0))", "(q.a_kcontig ? q.K % 8 == 0 : (q.M % 8 == 0))"),
]


@pytest.mark.parametrize("i", range(len(MUTATIONS)))
def test_a_moved_threshold_is_noticed(tmp_path, recorded, i):
    old, new = MUTATIONS[i]
    text = open(os.path.join(CSRC, "gemm_plan.h")).read()
    assert text.count(old) == 1, old
    (tmp_path / "gemm_plan.h").write_text(text.replace(old, new))
    exe = _compile(str(tmp_path / "gemm_plan_dump"), str(tmp_path), opt="-O0")
    got = subprocess.check_output([exe, "grid"], universal_newlines=True, env=_clean_env()).splitlines()
    assert _first_difference(got, recorded) is not None, (old, new)


def test_the_engine_workspace_covers_every_plan_of_its_launch_sites(dump):
    r = subprocess.run([dump, "sizing"], stdout=subprocess.PIPE, universal_newlines=True, env=_clean_env())
    assert r.returncode == 0, r.stdout[-4000:]
    assert r.stdout.endswith(" 0 uncovered\n") and int(r.stdout.split()[0]) > 20000000, r.stdout[-400:]


@pytest.mark.parametrize("impl", sorted(gc.IMPLS))
def test_case_tiles_agree_with_the_plan(dump, impl):
    """gemm_cases.case_tile (the float64 model needs the K tile without a library) against GemmPlan's (bm, bn, bk)"""
    im = gc.IMPLS[impl]
    cases = gc.cases_for(impl)
    text = "".join("%d %d %d %d %d %d %d %d %d\n" % (c.M, c.N, c.K, c.lay[0] == "N", c.lay[1] == "T", "gather" in c.opts,
                                                    "a2" in c.opts, im["prec"], im["in16"]) for c in cases)
    out = subprocess.run([dump, "plan"], input=text, stdout=subprocess.PIPE, check=True, universal_newlines=True,
                         env=_clean_env(im["env"])).stdout.splitlines()
    assert len(out) == len(cases)
    for c, line in zip(cases, out):
        assert tuple(int(v) for v in line.split()[:3]) == gc.case_tile(c), (c.name, line)


def test_one_environment_reader_and_one_attribute_site():
    text = {f: open(os.path.join(CSRC, f)).read() for f in ("gemm_f32.hip", "gemm_h16.hip", "gemm_g16.hip", "gemm_s3.hip",
                                                            "gemm_f32.h", "gemm_h16_dev.h", "gemm_plan.h")}
    assert [f for f, t in text.items() if "getenv" in t] == ["gemm_plan.h"]
    assert sum(t.count("hipFuncSetAttribute(") for t in text.values()) == 1
    for old in ("gemm_plan_splits", "gemm_pick_shape(int M, int N)", "h16_pick_big", "gemm_g16_enabled", "gemm_g16_applies"):
        assert old not in text["gemm_f32.h"], old
