"""CPU restatement (no GPU needed) of the 17..32-utterance form of recurrent.hip's tiled kernel
(brnn_recurrent_t_kernel<NCQ, NREGF, 1, ..., UG = 1>, round 7): its block -> (direction, unit block) map, where a
producer's step flag sits, and the per-wave register / LDS budget that puts one workgroup on every CU."""
import pytest

CUS, XCDS = 256, 8
LDS_BYTES = 160 * 1024
REC_FLAG_STRIDE = 8
REC_COUNTER_WORDS = 32 + 4 * 128 * REC_FLAG_STRIDE
# the dispatcher's instantiations: units -> (chunks per wave, weight fragments in registers)
FORMS = {1824: (29, 29), 2048: (32, 32)}


def block_map(b):
    """block -> (direction, unit block): combo = blockIdx.x & (2 UG - 1), ublk = blockIdx.x / (2 UG), UG = 1"""
    return b & 1, b >> 1


def k_split(nch, wave):
    """first chunk and chunk count of a wave's K quarter (the two-chain kernel's split)"""
    base, rem = nch >> 2, nch & 3
    return wave * base + min(wave, rem), base + (1 if wave < rem else 0)


def tiles(sub):
    """utterance tile of sub-chain `sub` (NT = 1, one half): tile = (i * 2 + sub) * UG + half"""
    return (0 * 2 + sub) * 1 + 0


def flag_word(direction, sub, producer):
    """counters word of a producer's flag: chain slot base + (q % 64) * stride + (q / 64) * NC + wave (wave 0, NC = 1)"""
    return 32 + (direction * 2 + sub) * 64 * REC_FLAG_STRIDE + (producer & 63) * REC_FLAG_STRIDE + (producer >> 6)


@pytest.mark.parametrize("H", sorted(FORMS))
def test_block_map_covers_every_unit_block_of_both_directions_once(H):
    nch = H // 16
    grid = 2 * nch
    assert grid in (228, 256) and grid <= CUS                 # one workgroup per CU
    seen = {}
    for b in range(grid):
        g, ublk = block_map(b)
        assert (g, ublk) not in seen
        seen[(g, ublk)] = b
        assert b % XCDS % 2 == g                               # a direction lives on four XCDs (block b on XCD b % 8)
    assert sorted(seen) == [(g, u) for g in range(2) for u in range(nch)]
    # the two sub-chains of a CU are the two utterance tiles of the minibatch
    assert (tiles(0), tiles(1)) == (0, 1)


@pytest.mark.parametrize("H", sorted(FORMS))
def test_flag_words_are_distinct_and_one_load_per_lane_holds_them(H):
    nprod = H // 16
    words = {}
    for g in range(2):
        for sub in range(2):
            for q in range(nprod):
                w = flag_word(g, sub, q)
                assert 32 <= w < REC_COUNTER_WORDS and w not in words
                words[w] = (g, sub, q)
                # polling lane q % 64 reads the four words of its slot in one 16-byte load: this word is among them
                slot = 32 + (g * 2 + sub) * 64 * REC_FLAG_STRIDE + (q % 64) * REC_FLAG_STRIDE
                assert slot <= w < slot + 4
    for lane in range(64):      # what a lane checks: producer lane, and lane + 64 where it exists
        assert [q for q in range(nprod) if q % 64 == lane] == [lane] + ([lane + 64] if lane + 64 < nprod else [])


@pytest.mark.parametrize("H", sorted(FORMS))
def test_k_split_and_register_budget(H):
    nch = H // 16
    ncq, nregf = FORMS[H]
    covered = []
    for wave in range(4):
        c0, cnt = k_split(nch, wave)
        assert cnt in (ncq, ncq - 1)                           # a shorter quarter multiplies its last chunk by zeros
        covered += list(range(c0, c0 + cnt))
    assert covered == list(range(nch))
    # the wave's whole K quarter of the 16 x H slab in accumulation registers: 4 per fragment, at most 256
    assert nregf == ncq and 4 * nregf <= 128
    assert 64 * 4 * nregf * 4 == ncq * 16 * 16 * 4              # 64 lanes x 4 nregf registers = ncq chunks of 16 x 16
    # LDS: partial sums [2 parities][1 result][3 waves][64 lanes] float4 + stamp words, padded to more than half the
    # CU's LDS so that no second workgroup fits (the co-residency check counts CUs)
    smem = max(16 * 64 * (2 * 3 * 1) + (16 * 8 + 8 * 32) * 4, 81 * 1024)
    assert LDS_BYTES // smem == 1
    # the LDS-resident slab (SCTC_REC_TCFG=3) fits as well, also one per CU
    smem_lds = 16 * 64 * (4 * ncq + 2 * 3) + (16 * 8 + 8 * 32) * 4
    assert smem_lds <= LDS_BYTES and LDS_BYTES // smem_lds == 1
