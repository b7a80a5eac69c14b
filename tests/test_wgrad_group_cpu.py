"""The planner of the grouped weight-gradient launch (devias_policy_wgrad_group_plan, csrc/gemm_wgrad_group.hip): pure host arithmetic, no GPU.

A plan is a list of rounds (tiles x split) over the concatenated 256 x 256 tile list of the jobs, and the unit table the kernel walks: per (round, workgroup) the
job, the tile, the K range in K-tiles of 64 rows and the partial tile the unit writes.  Checked here: every (job, tile) has its K range covered exactly once by
whole-K-tile slabs in order (devias_gemm's slab rule), no round exceeds the workgroups, units sit where the XCD-major order puts them, the plan is a function of its
input, and the K-tiles a CU walks stay at the figures the design counts on for the ViT-B encoder block (36 + 36 + 9 + 27 tiles, 784 K-tiles at B = 32)."""
import pytest

from devias_amd import ops

VITB = [36, 36, 9, 27]        # dW2, dW1, dWp, dWqkv of a ViT-B block in 256 x 256 tiles
CASES = [([1, 2, 3], 8, 8), ([1, 2, 3], 17, 8), ([1, 2, 3], 8, 16), ([1, 2, 3], 17, 16), ([1, 2, 3] * 2, 17, 8), ([2], 8, 8), ([2], 17, 8), ([5], 3, 64), ([1], 1, 8),
         (VITB, 784, 256), (VITB, 784, 248), (VITB, 784, 192), (VITB * 2, 784, 256), (VITB * 3, 784, 256), (VITB * 4, 784, 256), (VITB * 4, 784, 248),
         (VITB * 4, 784, 192), (VITB * 12, 784, 256), (VITB, 196, 256), ([9, 27], 49, 104)]


def cdiv(a, b):
    return -(-a // b)


def k_tiles_per_cu(rounds, kt):
    return sum(cdiv(kt, s) for _, s in rounds)


@pytest.mark.parametrize("jobs,kt,cus", CASES)
def test_plan_covers_every_tile_once_in_whole_slabs(jobs, kt, cus):
    rounds, units = ops.wgrad_group_plan(jobs, kt, cus)
    assert (rounds, units) == ops.wgrad_group_plan(jobs, kt, cus), "the same input must give the same plan"
    assert sum(t for t, _ in rounds) == sum(jobs) and len(units) == len(rounds) * cus
    glob = [(j, t) for j, n in enumerate(jobs) for t in range(n)]          # the concatenated tile list
    first, parts_seen, cover = 0, set(), {}
    for r, (nt, s) in enumerate(rounds):
        assert nt >= 1 and s >= 1 and nt * s <= cus, (r, nt, s, cus)
        per_slab = cdiv(kt, s)
        assert cdiv(kt, per_slab) == s, f"round {r}: split {s} is not what devias_gemm's slab rule makes of it at {kt} K-tiles"
        total, per = nt * s, cdiv(nt * s, 8)
        live = 0
        for b in range(cus):
            job, tile, kbeg, nk, part, rnd = units[r * cus + b]
            j = (b % 8) * per + b // 8
            if b // 8 >= per or j >= total:
                assert job == -1, (r, b)
                continue
            live += 1
            z, t = divmod(j, nt)
            assert (job, tile) == glob[first + t] and rnd == r, (r, b, job, tile)
            assert kbeg == z * per_slab and nk == min(per_slab, kt - kbeg) and nk >= 1, (r, b, kbeg, nk)
            assert (part == -1) == (s == 1)
            if part >= 0:
                assert part not in parts_seen
                parts_seen.add(part)
            cover.setdefault((job, tile), []).append((kbeg, nk, part, r))
        assert live == total
        first += nt
    assert sorted(cover) == glob
    for key, slabs in cover.items():
        slabs.sort()
        assert len({r for *_, r in slabs}) == 1, f"{key}: slabs in more than one round"
        pos = 0
        for kbeg, nk, _, _ in slabs:
            assert kbeg == pos, (key, slabs)
            pos += nk
        assert pos == kt, (key, slabs)
        if len(slabs) > 1:                                               # the combine sums part0, part0 + 1, ...: slab order
            assert [p for _, _, p, _ in slabs] == list(range(slabs[0][2], slabs[0][2] + len(slabs)))
    assert parts_seen == set(range(len(parts_seen)))


def test_vit_b_block_figures():
    one, _ = ops.wgrad_group_plan(VITB, 784, 256)
    four, _ = ops.wgrad_group_plan(VITB * 4, 784, 256)
    print("one block:", one, k_tiles_per_cu(one, 784), " four blocks:", four, k_tiles_per_cu(four, 784))
    assert k_tiles_per_cu(one, 784) <= 336
    assert k_tiles_per_cu(four, 784) <= 1340
    # today's per-product schedule walks 112 + 112 + 28 + 88 = 340 K-tiles per block and writes 1008 partial tiles
    assert sum(t * s for t, s in one if s > 1) < 1008
    assert sum(t * s for t, s in four if s > 1) < 4 * 1008 // 4


def test_bad_arguments_are_refused():
    for jobs, kt, cus in (([], 8, 8), ([0], 8, 8), ([1], 0, 8), ([1], 8, 12), ([1] * 65, 8, 8)):
        with pytest.raises(ValueError):
            ops.wgrad_group_plan(jobs, kt, cus)
