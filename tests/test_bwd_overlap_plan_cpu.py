"""The overlap order of the backward pass, checked without a GPU: csrc/bwd_overlap_plan.h (when it applies, which delta
buffer every GEMM uses) and the two BPTT forms it needs from csrc/recurrent_plan.h (SCTC_REC_VARIANT 52: the half grid,
53: the default grid with the larger LDS claim).

  * variant 52 gives the tiled family with NT = 1, UG = 2 on 2 * Hp / 32 workgroups at 17 and 32 utterances, fp32,
    Hp = 1824 / 2048; with 16-bit operands, 16 or 33 utterances, or a smaller layer, 52 and 53 plan what variant 0 plans;
  * the half grid's LDS and the claim of variant 53 both leave less of a CU's 160 KiB than any fp32 GEMM tile shape
    needs: GEMM blocks of a concurrent launch cannot land on a CU of the BPTT grid;
  * eligibility over NL in 1..7 x TL in 0..NL: fp32, training, Hp 1824 / 2048, 17..32 utterances, and at least two
    H x H weight gradients above the temporal layer;
  * the buffer route replayed on real arrays in the engine's launch order, in a stand-alone program built with
    -fsanitize=address,undefined: every weight gradient reads the delta the serial order gives it.
"""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "stanford-ctc_amd", "csrc")
GXX = ["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", CSRC]


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("bwd_overlap") / "bwd_overlap_plan_dump")
    subprocess.check_call(GXX + [os.path.join(ROOT, "tests", "bwd_overlap_plan_dump.cpp"), "-o", exe])
    return lambda what: subprocess.check_output([exe, what], universal_newlines=True).splitlines()


@pytest.fixture(scope="module")
def rec(dump):
    """(Hp, B, prec16, variant) -> (kernel name, grid, lds, variant the kernel sees, [template arguments])"""
    out = {}
    for line in dump("rec"):
        head, body = line.split(": ")
        key = tuple(int(v) for v in head.split()[1:])
        name, nums = body.split(" | ")
        nums = [int(v) for v in nums.split()]
        out[key] = (name, nums[0], nums[1], nums[2], nums[4:4 + nums[3]])
    return out


@pytest.mark.parametrize("B", [17, 32])
@pytest.mark.parametrize("Hp", [1824, 2048])
def test_variant_52_is_the_half_grid_tiled_form(rec, Hp, B):
    name, grid, lds, variant, targ = rec[Hp, B, 0, 52]
    assert name.startswith("brnn_recurrent_t_kernel<")
    assert targ[2] == 1 and targ[7] == 2 and targ[8] == 1
    assert grid == 2 * (Hp // 32) == {1824: 114, 2048: 128}[Hp]
    assert variant == 0                       # the kernel sees the default variant
    # the schedule is the 33..64 form's: same template arguments but the flag
    assert rec[Hp, 33, 0, 0][4] == targ[:8]
    # variant 53: the default kernel and grid, only the claim differs
    d, c = rec[Hp, B, 0, 0], rec[Hp, B, 0, 53]
    assert (c[0], c[1], c[3], c[4]) == (d[0], d[1], d[3], d[4]) and c[2] > d[2]
    assert c[1] == Hp // 8


@pytest.mark.parametrize("variant", [52, 53])
def test_overlap_variants_fall_through_to_the_default_plan_elsewhere(rec, variant):
    for (Hp, B, p16, v), got in rec.items():
        if v != variant:
            continue
        applies = Hp in (1824, 2048) and 17 <= B <= 32 and not p16
        if not applies:
            assert got == rec[Hp, B, p16, 0], (Hp, B, p16)
    for Hp in (1824, 2048):
        for B, p16 in ((16, 0), (33, 0), (1, 0), (64, 0), (17, 1), (32, 1)):
            assert rec[Hp, B, p16, variant] == rec[Hp, B, p16, 0]


def test_both_forms_leave_no_room_for_a_gemm_block(dump, rec):
    facts = {}
    gemm = []
    for line in dump("lds"):
        w = line.split()
        if w[0] == "gemm":
            gemm.append(int(w[2]))
        else:
            facts[w[0]] = int(w[1])
    assert len(gemm) == 4 and facts["cu"] == 160 * 1024
    for Hp in (1824, 2048):
        for B in (17, 32):
            for variant in (52, 53):
                left = facts["cu"] - rec[Hp, B, 0, variant][2]
                assert 0 <= left < min(gemm), (Hp, B, variant, left)
    assert facts["cu"] - facts["claim"] < min(gemm)


def test_eligibility_rule(dump):
    n = 0
    for line in dump("elig"):
        head, body = line.split(": ")
        NL, TL, Hp, fp32, train, B = (int(v) for v in head.split()[1:])
        config, eligible, extra = (int(v) for v in body.split())
        hh = NL - TL if 0 < TL < NL else 0            # H x H weight gradients above the temporal layer
        want_config = bool(fp32 and train and Hp in (1824, 2048) and hh >= 2)
        assert config == want_config, line
        assert eligible == (want_config and 17 <= B <= 32), line
        assert extra == (hh - 1 if want_config else 0), line
        n += 1
    assert n == sum(NL + 1 for NL in range(1, 8)) * 3 * 2 * 2 * 5


def test_routes(dump):
    seen = 0
    for line in dump("route"):
        head, body = line.split(": ")
        NL, TL, ov = (int(v) for v in head.split()[1:])
        flags, _, cells = body.partition(" |")
        ok, check = (int(v) for v in flags.split())
        hh = NL - TL if 0 < TL < NL else 0
        if ov and hh < 2:
            assert not ok, line
            continue
        assert ok and check == 0, line
        cells = [tuple(int(v) for v in c.split("/")) for c in cells.split()]      # loop index NL .. 0
        assert len(cells) == NL + 1
        assert cells[0][0] == 0                                                    # the CTC gradient
        assert [c[2] for c in cells] == [int(bool(ov) and i >= TL) for i in range(NL, -1, -1)]
        if not ov:          # dA, dBuf, dA, ...
            assert [c[1] for c in cells[:-1]] == [1 + k % 2 for k in range(NL)]
        else:
            front = [c[1] for c in cells[:NL - TL + 1]]                            # delta GEMMs in front of the join
            assert len(set(front)) == len(front) and 0 not in front
            assert max(front) == 3 + hh - 2                                        # exactly the hh - 1 extra buffers
        seen += 1
    assert seen > 40


def test_route_replay_under_sanitizers(tmp_path):
    exe = str(tmp_path / "bwd_overlap_route_check")
    subprocess.check_call(GXX + ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                                 os.path.join(ROOT, "tests", "bwd_overlap_route_check.cpp"), "-o", exe])
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert out.returncode == 0, out.stdout
    assert out.stdout.startswith("ok ")
