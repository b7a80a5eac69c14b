"""The five devias_fame_* entry points, one kernel at a time, against the exact references of tests/fame_kernel_ref.py at the edges of their domains: ties at the k-th
value that cross chunk boundaries, keys that only the second or third radix pass separates, negative keys, HW < 1024 and HW % 1024 != 0, k == 1 and k == HW, images that
are no multiple of the pooling cell, 1024 cells, a NULL binmask, several images per clip, the scalar and the two-sweep path of the mix, T > 2, clip values outside [0, 1], a
blur that fills its whole LDS tile -- and the host-side refusals, which must return before anything is launched.  Every equality is a torch.equal.

No case passes a pointer, stride or colour bin that a kernel would read or index out of range."""
import pytest
import torch

import fame_kernel_ref as fr
from devias_amd import _lib

pytestmark = pytest.mark.gpu

POOL_SHAPES = [(4, 4, 2), (24, 40, 8), (32, 32, 16), (33, 31, 16), (40, 56, 16), (48, 80, 16)]
SENTINEL = -7.0


def _st():
    return torch.cuda.current_stream().cuda_stream


def _ok(name, *args):
    _lib.check(getattr(_lib.load(), name)(*args), name)


def _refused(name, *args):
    rc = getattr(_lib.load(), name)(*args)
    torch.cuda.synchronize()
    assert rc != 0, f"{name} accepted a call outside its domain"
    assert _lib.load().devias_last_error()


# ---- binarize_pool -------------------------------------------------------------------------------------------------------------
def _binarize(x, H, W, k, pool, with_mask=True):
    n_img, ncell = x.shape[0], (H // pool) * (W // pool)
    xd = x.cuda()
    mask = torch.full((n_img, H * W), 77, dtype=torch.uint8, device="cuda") if with_mask else None
    pooled = torch.full((n_img, ncell), SENTINEL, device="cuda")
    _ok("devias_fame_binarize_pool", xd.data_ptr(), n_img, H, W, k, pool, mask.data_ptr() if with_mask else None, pooled.data_ptr(), _st())
    return (mask.cpu() if with_mask else None), pooled.cpu()


def _pool_images(kind, H, W, k):
    return torch.stack([fr.gen(kind, H * W, seed=11 * i + 1, k=k) for i in range(3)])        # a different generator seed per image


@pytest.mark.parametrize("kind", fr.GENERATORS)
@pytest.mark.parametrize("H,W,pool", POOL_SHAPES)
def test_binarize_pool_equals_reference(H, W, pool, kind):
    for _, k in fr.select_cases(kind, H * W, seed=1):
        x = _pool_images(kind, H, W, k)
        want_mask, want_pooled = fr.binarize_pool_ref(x, H, W, k, pool)
        mask, pooled = _binarize(x, H, W, k, pool)
        assert torch.equal(mask, want_mask), (kind, H, W, pool, k, int((mask != want_mask).sum()))
        assert torch.equal(pooled, want_pooled), (kind, H, W, pool, k)


@pytest.mark.parametrize("kind", ["smooth", "levels"])
def test_binarize_pool_at_1024_cells(kind):
    H = W = 512
    x = torch.stack([fr.gen(kind, H * W, seed=5 + i) for i in range(3)])
    orders = [fr.rank_order(img, True) for img in x]
    for k in fr.K_OF(x[0]):
        want = torch.zeros(3, H * W, dtype=torch.uint8)
        for i in range(3):
            want[i, orders[i][:k]] = 1
        want_pooled = torch.stack([fr._pool(m.view(H, W).long(), 16) for m in want])
        mask, pooled = _binarize(x, H, W, k, 16)
        assert pooled.shape[1] == 1024
        assert torch.equal(mask, want), (kind, k, int((mask != want).sum()))
        assert torch.equal(pooled, want_pooled), (kind, k)


@pytest.mark.parametrize("H,W,pool", POOL_SHAPES)
def test_binarize_pool_without_a_binmask(H, W, pool):
    k = H * W // 2
    x = _pool_images("one_tie_run", H, W, k)
    _, pooled = _binarize(x, H, W, k, pool, with_mask=False)
    assert torch.equal(pooled, fr.binarize_pool_ref(x, H, W, k, pool)[1])


# ---- seg_refine ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cmap_kind", fr.CMAP_GENERATORS)
@pytest.mark.parametrize("imgs_per_clip", [1, 3])
@pytest.mark.parametrize("HW", [10, 1023, 3840])
def test_seg_refine_equals_reference(HW, imgs_per_clip, cmap_kind):
    n_img, eps = 2 * imgs_per_clip, 1e-8
    cmap = fr.gen_cmap(cmap_kind, 2, HW, seed=HW)
    for kind in ("smooth", "levels", "signed", "one_tie_run", "low_bits"):
        blurred = torch.stack([fr.gen(kind, HW, seed=7 * i + HW, k=fr.refine_ks(HW)[0]) for i in range(n_img)])
        want, _, _ = fr.seg_refine_ref(blurred, cmap, imgs_per_clip, eps)
        want64, _, _ = fr.seg_refine_ref64(blurred, cmap, imgs_per_clip, eps)
        bd, cd = blurred.cuda(), cmap.cuda()
        out = torch.full((n_img, HW), SENTINEL, device="cuda")
        _ok("devias_fame_seg_refine", bd.data_ptr(), cd.data_ptr(), n_img, imgs_per_clip, HW, eps, out.data_ptr(), _st())
        out = out.cpu()
        assert torch.equal(out, want), (kind, int((out != want).sum()), float((out - want).abs().max()))
        assert bool(((out.double() - want64).abs() <= fr.REFINE_RTOL * want64.abs()).all()), kind      # independent of the fp32 restatement


# ---- mix -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,CT,HW", [(3, 6, 3), (3, 6, 1023), (3, 6, 1024), (2, 3, 66560)])
def test_mix_equals_reference(B, CT, HW):
    """HW = 3 and 1023: the scalar path; 1024: the vector path in one sweep; 66560 = 65 * 1024: the capped grid sweeps twice"""
    video, binmask, stride, src, partner, aug = fr.mix_inputs(B, CT, HW, seed=HW)
    want = fr.mix_ref(video, binmask, stride, src, partner, aug)
    vd, md, sd, pd, ad = video.cuda(), binmask.cuda(), src.cuda(), partner.cuda(), aug.cuda()
    out = torch.full((B, CT, HW), SENTINEL, device="cuda")
    _ok("devias_fame_mix", vd.data_ptr(), md.data_ptr(), stride, sd.data_ptr(), pd.data_ptr(), ad.data_ptr(), out.data_ptr(), B, CT, HW, _st())
    assert torch.equal(out.cpu(), want)
    assert torch.equal(vd.cpu(), video)


# ---- diff_color ----------------------------------------------------------------------------------------------------------------
def _diff_color(video):
    B, _, T, H, W = video.shape
    vd = video.cuda()
    diffs = torch.full((B, 1 + T // 2, H, W), SENTINEL, device="cuda")
    cmap = torch.full((B, H * W), -1, dtype=torch.int16, device="cuda")
    _ok("devias_fame_diff_color", vd.data_ptr(), B, T, H, W, diffs.data_ptr(), cmap.data_ptr(), _st())
    return diffs.cpu(), cmap.cpu().long()


@pytest.mark.parametrize("B,T,H,W", [(2, 2, 5, 7), (1, 4, 16, 17), (2, 6, 16, 16), (1, 8, 16, 16)])
def test_diff_color_equals_reference(B, T, H, W):
    video = fr.color_inputs(B, T, H, W, seed=T)
    cands = fr.checked_candidates(video)
    diffs, cmap = _diff_color(video)
    want = fr.diffs_ref(video)
    assert torch.equal(diffs, want), (int((diffs != want).sum()), float((diffs - want).abs().max()))
    inside = (cands == cmap[..., None]).any(-1)
    assert bool(inside.all()), (torch.nonzero(~inside).tolist()[:8], cmap[~inside].tolist()[:8])


def test_colour_bins_stay_in_range_outside_the_unit_cube():
    video = fr.wide_color_inputs(2, 2, 16, 16, seed=3)
    diffs, cmap = _diff_color(video)
    assert int(cmap.min()) >= 0 and int(cmap.max()) <= 999
    assert torch.equal(diffs, fr.diffs_ref(video))


# ---- blur ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W,ksize", [(6, 6, 11), (16, 16, 1), (33, 70, 11), (16, 40, 31), (70, 97, 31)])
def test_blur_within_bound(H, W, ksize):
    x = fr.blur_inputs(3, H, W, seed=ksize)
    ref, bound = fr.blur_ref(x, ksize, ksize / 3)
    xd = x.cuda()
    out = torch.full((3, H, W), SENTINEL, device="cuda")
    _ok("devias_fame_blur", xd.data_ptr(), out.data_ptr(), 3, H, W, ksize, ksize / 3, _st())
    ratio = fr.excess(out.cpu(), ref, bound)
    print(f"[bound] fame_blur {(H, W)} ksize {ksize} worst ratio {ratio:.3f}")
    assert ratio <= 1.0


# ---- host-side refusals: an error, no launch, destinations untouched -------------------------------------------------------------
def _sentinel(*shape, dtype=torch.float32):
    return torch.full(shape, 77 if dtype != torch.float32 else SENTINEL, dtype=dtype, device="cuda")


def _untouched(*tensors):
    torch.cuda.synchronize()
    for t in tensors:
        assert bool((t == (SENTINEL if t.dtype == torch.float32 else 77)).all())


def test_diff_color_refuses_odd_T():
    video = torch.zeros(1, 3, 3, 4, 4, device="cuda")
    diffs, cmap = _sentinel(1, 2, 4, 4), _sentinel(1, 16, dtype=torch.int16)
    _refused("devias_fame_diff_color", video.data_ptr(), 1, 3, 4, 4, diffs.data_ptr(), cmap.data_ptr(), _st())
    _untouched(diffs, cmap)


@pytest.mark.parametrize("H,W,ksize", [(16, 16, 10), (40, 40, 33), (5, 16, 11), (16, 5, 11)])
def test_blur_refuses_bad_kernel_sizes(H, W, ksize):
    """even, larger than 31, ksize / 2 >= H, ksize / 2 >= W"""
    x, out = torch.zeros(1, H, W, device="cuda"), _sentinel(1, H, W)
    _refused("devias_fame_blur", x.data_ptr(), out.data_ptr(), 1, H, W, ksize, ksize / 3, _st())
    _untouched(out)


def test_blur_refuses_in_place():
    x = _sentinel(1, 16, 16)
    _refused("devias_fame_blur", x.data_ptr(), x.data_ptr(), 1, 16, 16, 11, 11 / 3, _st())
    _untouched(x)


@pytest.mark.parametrize("H,W,pool,num_fg", [(16, 16, 16, 0), (16, 16, 16, 257), (528, 512, 16, 100), (32, 33, 1, 100)])
def test_binarize_pool_refuses(H, W, pool, num_fg):
    """num_fg of 0 or > HW; (H / pool) * (W / pool) > 1024"""
    x = torch.zeros(1, H * W, device="cuda")
    mask, pooled = _sentinel(1, H * W, dtype=torch.uint8), _sentinel(1, (H // pool) * (W // pool))
    _refused("devias_fame_binarize_pool", x.data_ptr(), 1, H, W, num_fg, pool, mask.data_ptr(), pooled.data_ptr(), _st())
    _untouched(mask, pooled)


def test_seg_refine_refuses_fewer_than_ten_pixels():
    x, cmap, out = torch.zeros(1, 9, device="cuda"), torch.zeros(1, 9, dtype=torch.int16, device="cuda"), _sentinel(1, 9)
    _refused("devias_fame_seg_refine", x.data_ptr(), cmap.data_ptr(), 1, 1, 9, 1e-8, out.data_ptr(), _st())
    _untouched(out)


def _mix_buffers(B, CT, HW):
    """video and out with four spare floats, the mask with four spare bytes, so that a view shifted by one element still lies inside its allocation"""
    n = B * CT * HW
    return (torch.zeros(n + 4, device="cuda"), _sentinel(n + 4), torch.ones(B * HW + 4, dtype=torch.uint8, device="cuda"),
            torch.zeros(B, dtype=torch.int32, device="cuda"), torch.zeros(B, dtype=torch.int32, device="cuda"), torch.ones(B, dtype=torch.int32, device="cuda"))


def test_mix_refuses_in_place():
    video, out, mask, src, partner, aug = _mix_buffers(2, 3, 16)
    video.fill_(SENTINEL)
    _refused("devias_fame_mix", video.data_ptr(), mask.data_ptr(), 16, src.data_ptr(), partner.data_ptr(), aug.data_ptr(), video.data_ptr(), 2, 3, 16, _st())
    _untouched(video)


@pytest.mark.parametrize("what", ["video", "out", "binmask", "mask_stride"])
def test_mix_refuses_what_its_vector_path_cannot_load(what):
    """HW % 4 == 0 moves 16-byte vectors of video / out and 4-byte vectors of the mask rows"""
    B, CT, HW = 2, 3, 16
    video, out, mask, src, partner, aug = _mix_buffers(B, CT, HW)
    v = video.data_ptr() + (4 if what == "video" else 0)
    o = out.data_ptr() + (4 if what == "out" else 0)
    m = mask.data_ptr() + (1 if what == "binmask" else 0)
    stride = HW + 2 if what == "mask_stride" else HW
    assert video.data_ptr() % 16 == 0 and out.data_ptr() % 16 == 0 and mask.data_ptr() % 4 == 0
    _refused("devias_fame_mix", v, m, stride, src.data_ptr(), partner.data_ptr(), aug.data_ptr(), o, B, CT, HW, _st())
    _untouched(out)


def test_mix_scalar_path_takes_any_float_alignment():
    """HW % 4 != 0: nothing wider than one element is loaded, so a 4-byte aligned view and an odd mask_stride are in the domain"""
    B, CT, HW = 3, 6, 1023
    video, binmask, _, src, partner, aug = fr.mix_inputs(B, CT, HW, seed=1)
    stride = HW                                                       # odd; the masks of the three clips back to back
    binmask = binmask.view(B, 3, HW)[:, 0].contiguous().view(-1)
    want = fr.mix_ref(video, binmask, stride, src, partner, aug)
    vbuf = torch.zeros(video.numel() + 1, device="cuda")
    vbuf[1:] = video.cuda().view(-1)
    obuf = torch.full((video.numel() + 1,), SENTINEL, device="cuda")
    mbuf = torch.zeros(binmask.numel() + 1, dtype=torch.uint8, device="cuda")
    mbuf[1:] = binmask.cuda()
    sd, pd, ad = src.cuda(), partner.cuda(), aug.cuda()
    _ok("devias_fame_mix", vbuf.data_ptr() + 4, mbuf.data_ptr() + 1, stride, sd.data_ptr(), pd.data_ptr(), ad.data_ptr(), obuf.data_ptr() + 4, B, CT, HW, _st())
    assert torch.equal(obuf[1:].cpu().view(B, CT, HW), want) and float(obuf[0]) == SENTINEL
