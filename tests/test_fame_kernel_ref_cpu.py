"""tests/fame_kernel_ref.py proven without a GPU: the restated device selection equals the exact reference on every generator x size x k that the GPU tests run, every
seeded mutant differs from the reference on at least one of those cases, the fp32 restatements agree with their float64 forms and with the CPU oracle, and the blur bound
is neither vacuous nor too tight for a plain fp32 implementation."""
import numpy as np
import pytest
import torch

import fame_kernel_ref as fr
from oracle.fame_cpu import FameOracle, gaussian_blur2d

POOL_SHAPES = [(4, 4, 2), (24, 40, 8), (32, 32, 16), (33, 31, 16), (40, 56, 16), (48, 80, 16)]      # the (H, W, pool) of test_fame_kernels_gpu.py
REFINE_HW = (10, 1023, 3840)
MIX_SHAPES = [(3, 6, 3), (3, 6, 1023), (3, 6, 1024), (2, 3, 66560)]
SELECT_SIZES = sorted({H * W for H, W, _ in POOL_SHAPES} | set(REFINE_HW))


def _pool_inputs(kind, H, W, k):
    return torch.stack([fr.gen(kind, H * W, seed=11 * i + 1, k=k) for i in range(3)])


def _pool_cases():
    for H, W, pool in POOL_SHAPES:
        for kind in fr.GENERATORS:
            for _, k in fr.select_cases(kind, H * W, seed=1):
                yield kind, H, W, pool, k


def test_emulated_selection_equals_the_reference():
    n_cases = 0
    for n in SELECT_SIZES:
        for kind in fr.GENERATORS:
            for largest in (True, False):
                for x, k in fr.select_cases(kind, n, seed=3, largest=largest):
                    assert torch.equal(fr.emulate_select(x, k, largest), fr.select_ref(x, k, largest)), (kind, n, k, largest)
                    n_cases += 1
    assert n_cases > 400


@pytest.mark.parametrize("kind", ["smooth", "levels"])
def test_emulated_selection_at_the_cell_limit(kind):
    """512 x 512 (ncell == 1024 at pool 16): chunks of 256 pixels"""
    x = fr.gen(kind, 512 * 512, seed=5)
    order = fr.rank_order(x, True)
    for k in fr.K_OF(x):
        assert torch.equal(fr.emulate_select(x, k, True), torch.sort(order[:k])[0]), (kind, k)


def test_generators_hold_what_they_promise():
    n = 3840
    chunk = (n + fr.SEL_NT - 1) // fr.SEL_NT
    assert torch.unique(fr.gen("smooth", n)).numel() == n
    assert torch.unique(fr.gen("levels", n)).numel() == 5
    key = fr.to_key(fr.gen("low_bits", n))
    assert torch.unique(key >> 10).numel() == 1 and torch.unique(key).numel() == 1024
    key = fr.to_key(fr.gen("mid_bits", n))
    assert torch.unique(key >> 21).numel() == 1 and torch.unique(key >> 10).numel() > 1000 and torch.unique(key).numel() == n
    s = fr.gen("signed", n)
    assert bool((s < 0).any()) and bool((s == 1e-40).any()) and bool((s == -1e-40).any()) and bool((s == 0).any())
    assert not bool(torch.signbit(s[s == 0]).any()) and bool(torch.isfinite(s).all())
    for k in (2, n // 2, n - 1):
        x = fr.gen("one_tie_run", n, seed=2, k=k)
        kth = torch.sort(x, descending=True)[0][k - 1]
        run = torch.nonzero(x == kth).flatten()
        need = k - int((x > kth).sum())
        assert run.numel() > 2 * chunk and int(run[-1] - run[0]) == run.numel() - 1          # one run of consecutive indices, longer than two chunks
        assert int(run[0]) % chunk and int(run[-1] + 1) % chunk                                 # starts and ends inside chunks
        assert 1 <= need < run.numel()
        if k == n // 2:
            assert int(run[0] + need) % chunk and need > chunk                                  # the cut lies inside a later chunk of the run
        assert torch.unique(x).numel() == n - run.numel() + 1
    lv = fr.gen("levels", 3840, seed=1)
    assert {int((lv > v).sum()) + 1 for v in fr.LEVELS} <= set(fr.K_OF(lv)) | {3841}


def _mutant_shows(mutant):
    family = fr.MUTANTS[mutant]
    if family == "select":                                  # on the selections the binarize_pool GPU cases run (largest only)
        for kind, H, W, pool, k in _pool_cases():
            for x in _pool_inputs(kind, H, W, k):
                if not torch.equal(fr.emulate_select(x, k, True, mutant), fr.select_ref(x, k, True)):
                    return (kind, H, W, k)
    elif family == "pool":
        for kind, H, W, pool, k in _pool_cases():
            x = _pool_inputs(kind, H, W, k)
            ref, out = fr.binarize_pool_ref(x, H, W, k, pool), fr.emulate_binarize_pool(x, H, W, k, pool, mutant)
            if not (torch.equal(ref[0], out[0]) and torch.equal(ref[1], out[1])):
                return (kind, H, W, pool, k)
    elif family == "refine":
        for HW in REFINE_HW:
            for ipc in (1, 3):
                blurred = torch.stack([fr.gen("smooth", HW, seed=i) for i in range(2 * ipc)])
                for ck in fr.CMAP_GENERATORS:
                    cmap = fr.gen_cmap(ck, 2, HW, seed=HW)
                    if not torch.equal(fr.emulate_seg_refine(blurred, cmap, ipc, 1e-8, mutant)[0], fr.seg_refine_ref(blurred, cmap, ipc, 1e-8)[0]):
                        return (HW, ipc, ck)
    else:
        for B, CT, HW in MIX_SHAPES:
            I = fr.mix_inputs(B, CT, HW, seed=HW)
            sentinel = torch.full_like(I[0], -7.0)
            if not torch.equal(fr.mix_ref(*I, mutant=mutant, out_init=sentinel), fr.mix_ref(*I)):
                return (B, CT, HW)
    return None


@pytest.mark.parametrize("mutant", sorted(fr.MUTANTS))
def test_every_mutant_differs_from_the_reference(mutant):
    assert _mutant_shows(mutant) is not None, f"no case tells the mutant {mutant} from the kernel: the cases show nothing about it"


def test_unmutated_emulations_equal_the_references():
    for H, W, pool in POOL_SHAPES:
        for kind in ("levels", "one_tie_run", "signed"):
            k = H * W // 2
            x = _pool_inputs(kind, H, W, k)
            ref, out = fr.binarize_pool_ref(x, H, W, k, pool), fr.emulate_binarize_pool(x, H, W, k, pool)
            assert torch.equal(ref[0], out[0]) and torch.equal(ref[1], out[1])
            assert int(ref[0].sum()) == 3 * k
            assert bool((ref[1] * pool * pool == torch.round(ref[1] * pool * pool)).all())       # counts / pool^2, exactly


def test_fp32_refine_is_within_its_budget_of_float64(capsys):
    worst = 0.0
    for HW in REFINE_HW:
        for ipc in (1, 3):
            for kind in ("smooth", "levels", "signed", "one_tie_run"):
                blurred = torch.stack([fr.gen(kind, HW, seed=7 * i + HW, k=fr.refine_ks(HW)[0]) for i in range(2 * ipc)])
                for ck in fr.CMAP_GENERATORS:
                    cmap = fr.gen_cmap(ck, 2, HW, seed=HW)
                    r32, hf, hb = fr.seg_refine_ref(blurred, cmap, ipc, 1e-8)
                    r64, hf64, hb64 = fr.seg_refine_ref64(blurred, cmap, ipc, 1e-8)
                    assert r32.dtype == torch.float32 and r64.dtype == torch.float64
                    assert torch.equal(hf, hf64) and int(hf.sum()) == 2 * ipc * fr.refine_ks(HW)[0] and int(hb.sum()) == 2 * ipc * fr.refine_ks(HW)[1]
                    assert bool(((r64 >= 0) & (r64 <= 1)).all())
                    err = (r32.double() - r64).abs()
                    assert bool((err <= fr.REFINE_RTOL * r64.abs()).all()), (HW, ipc, kind, ck)
                    worst = max(worst, float((err / r64.abs().clamp_min(1e-300)).max()) / fr.U32)
    assert worst > 0.25                                      # the fp32 form does round: the budget is not vacuous
    with capsys.disabled():
        print(f"[bound] fame_seg_refine fp32 restatement vs float64: worst {worst:.2f} u of {fr.REFINE_RTOL / fr.U32:.0f} u")


COLOR_SHAPES = [(2, 2, 5, 7), (1, 4, 16, 17), (2, 6, 16, 16), (1, 8, 16, 16)]


@pytest.mark.parametrize("shape", COLOR_SHAPES)
def test_oracle_colour_map_lies_in_the_candidates(shape):
    video = fr.color_inputs(*shape, seed=shape[1])
    cands = fr.checked_candidates(video)                    # asserts >= 90 % single-candidate pixels
    o = FameOracle()
    got = o.color_map(o.denorm(video)).clamp(0, 999)
    assert bool((cands == got[..., None]).any(-1).all())
    # the planted pixels are what they claim
    c = o.denorm(video)[0].mean(1).reshape(3, -1)
    assert float(c[0, 0]) == float(c[1, 0]) == float(c[2, 0]) == 0.625
    assert 0 < float(c[:, 1].max()) < 0.03
    assert float(c[0, 2]) == float(c[1, 2]) > float(c[2, 2])
    assert float(fr.diffs_ref(video)[0].reshape(-1, shape[2] * shape[3])[:, 3].abs().max()) == 0.0
    assert float(c[0, 4]) > float(c[2, 4]) > float(c[1, 4]) > float(c[2, 4]) - 0.01      # red maximum, green just under blue: the hue is just below its wrap


def test_candidate_sets_on_uniform_colours():
    g = torch.Generator().manual_seed(0)
    video = fr._normalise(torch.rand(1, 3, 2, 128, 128, generator=g))
    frac = fr.single_candidate_fraction(fr.color_candidates(video))
    assert 0.95 <= frac <= 0.985, frac                       # about 3 % of uniform random colours sit within the margin of a bin edge


def test_wide_clip_reaches_both_clamps():
    video = fr.wide_color_inputs(2, 2, 16, 16, seed=3)
    c = fr.bin_coordinates(video)
    raw = torch.round(c[..., 0]) + (torch.round(c[..., 1]) - 1) * 10 + (torch.round(c[..., 2]) - 1) * 100
    assert float(raw.min()) < 0 and float(raw.max()) > 999
    assert int(fr.color_candidates(video).min()) >= 0 and int(fr.color_candidates(video).max()) <= 999


@pytest.mark.parametrize("shape", COLOR_SHAPES)
def test_diffs_restatement_matches_the_oracle(shape):
    video = fr.color_inputs(*shape, seed=shape[1])
    B, T, H, W = shape
    d = fr.diffs_ref(video)
    assert d.dtype == torch.float32 and d.shape == (B, 1 + T // 2, H, W)
    clips = FameOracle().denorm(video).double()
    a = (clips[:, :, :-1] - clips[:, :, 1:]).abs().sum(1)
    assert float((d[:, 0].double() - a.mean(1)).abs().max()) < 1e-6
    for i in range(T // 2):
        assert float((d[:, 1 + i].double() - a[:, 2 * i]).abs().max()) < 1e-6


BLUR_SHAPES = [(6, 6, 11), (16, 16, 1), (33, 70, 11), (16, 40, 31), (70, 97, 31)]


def test_oracle_blur_stays_under_half_of_the_bound(capsys):
    worst = {}
    for H, W, ksize in BLUR_SHAPES:
        x = fr.blur_inputs(3, H, W, seed=ksize)
        ref, bound = fr.blur_ref(x, ksize, ksize / 3)
        out = gaussian_blur2d(x[:, None], ksize, ksize / 3)[:, 0]
        worst[(H, W, ksize)] = fr.excess(out, ref, bound)
        assert worst[(H, W, ksize)] <= 0.5, (H, W, ksize, worst)
        # ... and is not vacuous: one tap dropped from the row pass, or the unnormalised taps, exceed it
        w = fr.gaussian_taps64(ksize, ksize / 3)
        if ksize > 1:
            assert fr.excess(ref * (1 - float(w[0])), ref, bound) > 1
            R = ksize // 2
            shifted = torch.nn.functional.pad(x[:, None].double(), (R, R, R, R), mode="replicate")     # the wrong border
            shifted = torch.nn.functional.conv2d(torch.nn.functional.conv2d(shifted, w.view(1, 1, 1, -1)), w.view(1, 1, -1, 1))[:, 0]
            assert fr.excess(shifted, ref, bound) > 1
    assert fr.blur_roundings(11) == 62 and fr.blur_roundings(31) == 142
    with capsys.disabled():
        for k, v in worst.items():
            print(f"[bound] emulation fame_blur {k} worst ratio {v:.3f}")


def test_num_fg_is_the_references_expression(monkeypatch):
    """int(beta * H * W) (fame.py:80) is not int(beta * (H * W)) everywhere; the two selection sizes of the colour model do agree"""
    differ = [s for s in range(4, 513) if int(0.7 * s * s) != int(0.7 * (s * s))]
    assert {90, 150, 170, 180, 210, 290, 300} <= set(differ)
    hs = np.arange(4, 513, dtype=np.float64)
    for f in (0.5, 0.1):
        assert np.array_equal(np.floor(f * hs[:, None] * hs[None, :]), np.floor(f * (hs[:, None] * hs[None, :])))
    # FAME.masks hands the reference's expression to devias_fame_binarize_pool
    from devias_amd import fame, ops
    calls = []
    monkeypatch.setattr(fame, "_call", lambda name, *args: calls.append((name, args)))
    monkeypatch.setattr(ops, "_chk", lambda t, *a, **k: t)
    monkeypatch.setattr(ops, "_stream", lambda: 0)
    for size in (90, 150, 112):
        calls.clear()
        fame.FAME(beta=0.7, prob_aug=1.0).masks(torch.zeros(1, 3, 2, size, size))
        (args,) = [a for n, a in calls if n == "devias_fame_binarize_pool"]
        assert args[4] == int(0.7 * size * size), (size, args[4])
