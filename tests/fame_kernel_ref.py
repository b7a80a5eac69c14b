"""Exact per-kernel references for the FAME kernels (devias_amd/csrc/fame.hip, driven by devias_amd/fame.py), their edge-case inputs and seeded mutants.

A plain helper module (like kernel_bounds.py and pool_head_bounds.py): no fixtures, no plugin, torch on the CPU only.  tests/test_fame_kernel_ref_cpu.py proves without a
GPU that the cases discriminate (the restated device algorithm equals the reference on every case, every mutant differs on at least one); tests/test_fame_kernels_gpu.py
holds the five devias_fame_* entry points to these references.

Why exact: the pipeline tests of test_fame_gpu.py accept agreement RATES (>= 99.5 % of the mask pixels, mean |pooled diff| < 2e-3) because the device ranks un-normalised
blurred images where the reference ranks them after norm_batch.  That tolerance is right for the pipeline and lets almost any local error of one kernel through.  Kernel by
kernel everything is integer or selection logic, or a short chain of correctly rounded fp32 operations:

    select          the selected index SET of radix_select + for_each_selected: the k best values, ties at the k-th value in index order.  Exact.
    binarize_pool   uint8 mask of the selection; pooled = count / pool^2 over the pool x pool cells that fit (remainder rows / columns dropped).  Exact.
    seg_refine      two integer histograms of the colour bins under the HW/2 largest and HW/10 smallest pixels, then three correctly rounded fp32 divisions
                    (fame.hip: pf = hfg / sfg, pb = (hbg + 1) / sbg, refine = pf / (pb + pf)) -> bitwise on CPU fp32; within 4 * 2^-24 relative of the float64 form.
    mix             a select between two clips by a byte mask.  Exact.
    diff_color      diffs: fl(fl(x std) + mean), |prev - cur| summed over channels 0, 1, 2, summed over t in order, one division by T - 1: every step one correctly
                    rounded fp32 operation (the kernel forbids contraction of the denormalisation) -> bitwise on CPU fp32.
                    cmap: sinf / cosf of an angle up to 4 pi^2 cannot be restated bitwise; instead every device bin must lie in the set of bins reachable when
                    each of the three pre-rounding bin coordinates (float64) moves by +- BIN_MARGIN.
    blur            float64 reference with a per-element bound (blur_ref).

None of the cases passes a pointer, stride or colour bin that a kernel would read or index out of range."""
import math

import torch

U32 = 2.0 ** -24                       # unit roundoff of fp32
SEL_NT = 1024                          # fame.hip: threads of the selection kernels = chunks of for_each_selected
BIN_MARGIN = 5e-3                      # the margin test_fame_gpu.py uses for the kornia vectors (bin_margin > 5e-3)
REFINE_RTOL = 4 * U32                  # fp32 seg_refine against its float64 form: three correctly rounded divisions and the sum pb + pf
MEAN = (0.485, 0.456, 0.406)
STD = (0.229, 0.224, 0.225)


# ---- selection -------------------------------------------------------------------------------------------------------------------
def rank_order(x, largest):
    """All indices of the 1-D tensor x, best first: value order, ties in index order (a stable sort)."""
    v = x.double()
    return torch.sort(-v if largest else v, stable=True)[1]


def select_ref(x, k, largest):
    """The exact index set (sorted int64) that a top-k of the 1-D fp32 tensor x must select: the k best values, ties at the k-th value taken in index order.

    Domain: finite values, no -0.0 and no NaN (to_key orders -0.0 below +0.0 where a float comparison ties them).  The pipeline cannot produce either: the diffs are
    sums of fabsf, the blurs are sums of non-negative products and `refine` is a quotient of non-negatives.  Negative values ARE in the domain (to_key has a branch for
    them that pipeline data never reaches)."""
    assert 1 <= k <= x.numel()
    return torch.sort(rank_order(x, largest)[:k])[0]


def to_key(x, mutant=None):
    """fame.hip to_key on int64: larger float <=> larger 32-bit key"""
    u = x.contiguous().view(torch.int32).long() & 0xFFFFFFFF
    if mutant == "key_sign_branch_dropped":
        return u | 0x80000000
    return torch.where((u & 0x80000000) != 0, ~u & 0xFFFFFFFF, u | 0x80000000)


SELECT_MUTANTS = ("ties_from_end", "need_plus_one", "need_per_chunk", "key_sign_branch_dropped", "shifts_22_11_0", "last_pass_11_bit_digit", "walk_direction_swapped")


def emulate_select(x, k, largest, mutant=None):
    """The device algorithm restated (radix_select + for_each_selected of fame.hip), returning the sorted selected indices.

    to_key; three passes over the key's bits 31..21, 20..10, 9..0 (11 / 11 / 10 bits), each a histogram of the digit among the keys that match the prefix so far and a
    walk from the best digit until the cumulative count reaches `remaining`; after the last pass the prefix is the k-th key and need = remaining is the number of keys
    EQUAL to it that belong to the selection.  Then: every strictly better key, and the ties in 1024 chunks of cdiv(n, 1024) consecutive indices, chunk t starting at
    before = (ties in chunks < t) and taking ties in index order while before < need.

    Mutants (SELECT_MUTANTS):
      ties_from_end            the LAST `need` ties in index order
      need_plus_one            need + 1 ties
      need_per_chunk           `before` starts at 0 in every chunk (the scan of the chunk counts is skipped)
      key_sign_branch_dropped  to_key without the branch for negative floats
      shifts_22_11_0           pass shifts 22 / 11 / 0 (bit 10 is never examined, bit 21 twice)
      last_pass_11_bit_digit   the last pass histograms an 11-bit digit while the walk still covers its 1024 bins: keys whose bit 10 is set are never found and the
                               stale digit of the pass before is kept.  (Widening BOTH to 11 bits changes nothing -- bit 10 is already fixed by the prefix -- so that is
                               no mutant.)
      walk_direction_swapped   the digit walk runs from the worst digit (largest / smallest swapped in the walk only, not in the comparison of the final pass)"""
    assert mutant is None or mutant in SELECT_MUTANTS
    n = x.numel()
    key = to_key(x, mutant)
    shifts = (22, 11, 0) if mutant == "shifts_22_11_0" else (21, 10, 0)
    bits = (11, 11, 10)
    prefix, mask, remaining, sel = 0, 0, k, 0
    walk_largest = (not largest) if mutant == "walk_direction_swapped" else largest
    for p in range(3):
        shift, nb = shifts[p], 1 << bits[p]
        hb = 2048 if (p == 2 and mutant == "last_pass_11_bit_digit") else nb
        cand = key[(key & mask) == prefix]
        hist = torch.bincount((cand >> shift) & (hb - 1), minlength=2048)[:nb]
        order = torch.arange(nb - 1, -1, -1) if walk_largest else torch.arange(nb)
        cum = torch.cumsum(hist[order], 0)
        hit = torch.nonzero(cum >= remaining)
        if hit.numel():                                            # (no digit found: sh.sel and sh.remaining keep their stale values)
            pos = int(hit[0])
            sel = int(order[pos])
            remaining = remaining - int(cum[pos] - hist[sel])
        prefix |= sel << shift
        mask |= (nb - 1) << shift
    prefix &= 0xFFFFFFFF
    need = remaining + 1 if mutant == "need_plus_one" else remaining
    better = key > prefix if largest else key < prefix
    tie = key == prefix
    idx = torch.arange(n)
    if mutant == "ties_from_end":
        t = idx[tie]
        taken = t[max(0, t.numel() - need):]
    else:
        chunk = (n + SEL_NT - 1) // SEL_NT
        chunk_of = idx // chunk
        if mutant == "need_per_chunk":
            before = torch.zeros(SEL_NT, dtype=torch.long)
        else:
            cnt = torch.bincount(chunk_of[tie], minlength=SEL_NT)
            before = torch.cumsum(cnt, 0) - cnt
        t = idx[tie]
        tc = chunk_of[t]
        first = torch.searchsorted(tc, tc, right=False)            # position of the chunk's first tie within t
        rank_in_chunk = torch.arange(t.numel()) - first
        taken = t[before[tc] + rank_in_chunk < need]
    return torch.sort(torch.cat([idx[better], taken]))[0]


# ---- input generators: gen(kind, n, seed, k, largest) -> fp32 [n] ------------------------------------------------------------
GENERATORS = ("smooth", "levels", "low_bits", "mid_bits", "signed", "one_tie_run", "constant")
LEVELS = (0.0, 0.25, 0.5, 0.75, 1.0)


def _rng(seed):
    return torch.Generator().manual_seed(seed)


def gen(kind, n, seed=0, k=None, largest=True):
    """smooth       n distinct non-negative values in random order
    levels       five values: the k-th value's tie group is a fifth of the image and spans every chunk
    low_bits     1 + (j mod 1024) 2^-23: the keys share their top 22 bits, only the last pass separates them (with ties once n > 1024)
    mid_bits     1 + j 2^-23 for distinct j < 2^21: the keys share exactly their top 11 bits, the first pass separates nothing
    signed       mixed sign with exact +0 and +-1e-40 (subnormal) around the median: the negative branch of to_key, keys next to 0x80000000 on both sides
    one_tie_run  all distinct except one run of consecutive indices equal to the k-th value; the run starts and ends inside chunks, and `need` ends inside a chunk
    constant     every pixel ties"""
    g = _rng(seed)
    perm = torch.randperm(n, generator=g)
    if kind == "smooth":
        return (perm.float() + 0.5) * 2.0 ** -10
    if kind == "levels":
        return torch.tensor(LEVELS)[torch.randint(0, 5, (n,), generator=g)]
    if kind == "low_bits":
        return 1.0 + (perm % 1024).float() * 2.0 ** -23
    if kind == "mid_bits":
        assert n <= 2 ** 21
        return 1.0 + ((perm * 2654435761) % 2 ** 21).float() * 2.0 ** -23      # an odd multiplier is a bijection mod 2^21
    if kind == "signed":
        r = perm.float() - (n - 1) / 2.0                                          # distinct, both signs (0.0 itself only for odd n)
        x = torch.where(r.abs() < n / 8.0, torch.zeros(()), r * 2.0 ** -6)       # the middle quarter of the ranks -> +0 ...
        which = torch.randint(0, 4, (n,), generator=g)
        tiny = torch.tensor([0.0, 1e-40, -1e-40, 0.0])[which]                     # ... or +-1e-40
        return torch.where(x == 0, tiny, x) + 0.0                                 # (+ 0.0: no -0.0 can survive)
    if kind == "constant":
        return torch.full((n,), 0.375)
    assert kind == "one_tie_run"
    k = n // 2 if k is None else k
    chunk = (n + SEL_NT - 1) // SEL_NT
    half = chunk // 2
    tail = next((r for r in range(max(1, chunk // 3), 2 * chunk + 1) if (half + r) % chunk), 1)
    L = max(1, min(n // 3, 2 * chunk + tail))                                     # run length: a little over two chunks, ending inside a chunk
    a = min(n - L, (3 + seed % 5) * chunk + half)                                 # starts in the middle of a chunk
    need = next((m for m in range(L // 2 + 1, L) if (half + m) % chunk), L // 2 + 1)
    need = max(1, min(k, need))                                                   # the selection is cut inside the run, in the middle of a chunk (k allowing)
    better = k - need                                                             # values strictly better than the run's
    if better > n - L:
        better, need = n - L, k - (n - L)
    rest = torch.randperm(n - L, generator=g)
    sign = 1.0 if largest else -1.0
    vals = torch.where(rest < better, sign * (rest + 1).float(), -sign * (rest + 1).float()) * 2.0 ** -12 + 1.0
    x = torch.empty(n)
    x[:a], x[a:a + L], x[a + L:] = vals[:a], 1.0, vals[a:]
    return x


def K_OF(x):
    """The k values to run on the 1-D image x: 1, 2, n // 2, n - 1, n; where x has few levels also, at each level v, #(x > v), #(x > v) + 1 and #(x >= v)"""
    n = x.numel()
    ks = {1, 2, n // 2, n - 1, n}
    levels = torch.unique(x)
    if levels.numel() <= 8:
        for v in levels:
            ks |= {int((x > v).sum()), int((x > v).sum()) + 1, int((x >= v).sum())}
    return sorted(k for k in ks if 1 <= k <= n)


def select_cases(kind, n, seed=0, largest=True):
    """(x, k) pairs of one generator at one size"""
    if kind == "one_tie_run":
        for k in K_OF(torch.arange(n)):
            yield gen(kind, n, seed, k, largest), k
    else:
        x = gen(kind, n, seed)
        for k in K_OF(x):
            yield x, k


# ---- binarize + pool ---------------------------------------------------------------------------------------------------------
def _pool(mask2d, pool):
    H, W = mask2d.shape
    ph, pw = H // pool, W // pool
    return mask2d[:ph * pool, :pw * pool].reshape(ph, pool, pw, pool).sum((1, 3)).reshape(-1).float() / float(pool * pool)


def binarize_pool_ref(x, H, W, k, pool):
    """x [n_img, H*W] fp32 -> (uint8 mask [n_img, H*W] of the k largest per image, pooled [n_img, (H/pool)(W/pool)] = count / pool^2 of each whole cell; the counts are
    integers <= pool^2 and pool^2 a power of two in every case run, so the quotient is exact)"""
    masks, pooled = [], []
    for img in x:
        m = torch.zeros(H * W, dtype=torch.uint8)
        m[select_ref(img, k, True)] = 1
        masks.append(m)
        pooled.append(_pool(m.view(H, W).long(), pool))
    return torch.stack(masks), torch.stack(pooled)


POOL_MUTANTS = ("cell_index_transposed", "remainder_not_dropped")


def emulate_binarize_pool(x, H, W, k, pool, mutant=None):
    """fame_binarize_pool_kernel restated: integer cell counters indexed (y / pool) * pw + x / pool under the guard that drops remainder rows and columns.
    Mutants: cell_index_transposed  (x / pool) * ph + y / pool;
             remainder_not_dropped  no guard: a remainder column counts into the NEXT row's first cell (a remainder row's index lies past the last cell, where the
                                    pooled output cannot show it)."""
    assert mutant is None or mutant in POOL_MUTANTS
    ph, pw = H // pool, W // pool
    masks, pooled = [], []
    for img in x:
        sel = emulate_select(img, k, True)
        m = torch.zeros(H * W, dtype=torch.uint8)
        m[sel] = 1
        y, xx = sel // W, sel % W
        inside = (y // pool < ph) & (xx // pool < pw)
        if mutant == "cell_index_transposed":
            cell = (xx // pool) * ph + y // pool
        else:
            cell = (y // pool) * pw + xx // pool
        if mutant == "remainder_not_dropped":
            inside = cell < ph * pw
        masks.append(m)
        pooled.append(torch.bincount(cell[inside], minlength=ph * pw).float() / float(pool * pool))
    return torch.stack(masks), torch.stack(pooled)


# ---- colour histograms -> refined soft mask --------------------------------------------------------------------------------------
REFINE_MUTANTS = ("cmap_of_clip_modulo",)


def refine_ks(HW):
    """devias_fame_seg_refine: k_fg, k_bg"""
    return int(0.5 * HW), int(0.1 * HW)


def _histograms(blurred, cmap, imgs_per_clip, select, mutant=None):
    HW = blurred.shape[1]
    k_fg, k_bg = refine_ks(HW)
    hf, hb, cms = [], [], []
    for i, img in enumerate(blurred):
        cm = cmap[i % imgs_per_clip if mutant == "cmap_of_clip_modulo" else i // imgs_per_clip].long()
        hf.append(torch.bincount(cm[select(img, k_fg, True)], minlength=1000))
        hb.append(torch.bincount(cm[select(img, k_bg, False)], minlength=1000))
        cms.append(cm)
    return torch.stack(hf), torch.stack(hb), torch.stack(cms)


def _refine(hfg, hbg, cm, HW, eps, dtype):
    k_fg, k_bg = refine_ks(HW)
    eps = torch.tensor(eps, dtype=torch.float32).to(dtype)
    sfg = torch.tensor(float(k_fg), dtype=dtype) + eps
    sbg = torch.tensor(float(k_bg + 1000), dtype=dtype) + eps
    pf = hfg.to(dtype).gather(1, cm) / sfg
    pb = (hbg.to(dtype).gather(1, cm) + 1.0) / sbg
    return pf / (pb + pf)


def seg_refine_ref(blurred, cmap, imgs_per_clip, eps, dtype=torch.float32, select=select_ref, mutant=None):
    """blurred [n_img, HW] fp32, cmap [n_clip, HW] integer bins 0..999; image i takes the colour map of clip i // imgs_per_clip.  Returns (refine [n_img, HW] in `dtype`,
    hfg, hbg [n_img, 1000] int64).  The histograms count the bins under the HW/2 largest and the HW/10 smallest pixels (select_ref); then, in the kernel's order and each
    one operation of `dtype`:  sfg = k_fg + eps, sbg = (k_bg + 1000) + eps, pf = hfg[c] / sfg, pb = (hbg[c] + 1) / sbg, refine = pf / (pb + pf)."""
    hfg, hbg, cm = _histograms(blurred, cmap, imgs_per_clip, select, mutant)
    return _refine(hfg, hbg, cm, blurred.shape[1], eps, dtype), hfg, hbg


def seg_refine_ref64(blurred, cmap, imgs_per_clip, eps):
    """the same in float64"""
    return seg_refine_ref(blurred, cmap, imgs_per_clip, eps, torch.float64)


def emulate_seg_refine(blurred, cmap, imgs_per_clip, eps, mutant=None):
    """the fp32 form over the restated device selection; mutant cmap_of_clip_modulo: the colour map of clip img % imgs_per_clip"""
    assert mutant is None or mutant in REFINE_MUTANTS
    return seg_refine_ref(blurred, cmap, imgs_per_clip, eps, torch.float32, emulate_select, mutant)


CMAP_GENERATORS = ("random", "one_bin", "ends")


def gen_cmap(kind, n_clip, HW, seed=0):
    g = _rng(seed)
    if kind == "random":
        return torch.randint(0, 1000, (n_clip, HW), generator=g).to(torch.int16)
    if kind == "one_bin":
        return torch.tensor([[417], [58]] * n_clip)[:n_clip].expand(n_clip, HW).contiguous().to(torch.int16)
    assert kind == "ends"
    return (torch.randint(0, 2, (n_clip, HW), generator=g) * 999).to(torch.int16)


# ---- mix ---------------------------------------------------------------------------------------------------------------------
MIX_MUTANTS = ("mask_row_of_output", "one_grid_sweep")


def mix_ref(video, binmask, mask_stride, src, partner, aug, mutant=None, out_init=None):
    """video [B, CT, HW] fp32; binmask a flat uint8 buffer whose mask of clip c is binmask[c * mask_stride : c * mask_stride + HW]; src, partner, aug integer [B].
    out[j] = aug[j] ? (mask[src[j]] ? video[src[j]] : video[partner[j]]) : video[src[j]].
    Mutants: mask_row_of_output  the mask row of j instead of src[j];
             one_grid_sweep      the grid is capped at 64 blocks of 256 threads; without the grid-stride loop the elements past the first sweep (64 * 1024 on the
                                 vector path HW % 4 == 0, 64 * 256 on the scalar path) keep `out_init`"""
    assert mutant is None or mutant in MIX_MUTANTS
    B, CT, HW = video.shape
    out = torch.empty_like(video)
    for j in range(B):
        s, p = int(src[j]), int(partner[j])
        row = j if mutant == "mask_row_of_output" else s
        m = binmask[row * mask_stride: row * mask_stride + HW] != 0
        out[j] = torch.where(m[None, :], video[s], video[p]) if int(aug[j]) else video[s]
    if mutant == "one_grid_sweep":
        gx = max(1, min(64, (HW // 4 + 255) // 256))
        swept = gx * (1024 if HW % 4 == 0 else 256)
        out[:, :, swept:] = out_init[:, :, swept:]
    return out


def mix_inputs(B, CT, HW, seed=0):
    """video, the flat mask buffer (three slots per clip, mask_stride = 3 HW: slot 0 the mask, the two unused slots its inverse), mask_stride, src (a permutation),
    partner (one augmented row is its own partner), aug = [1, 0, 1][:B]"""
    g = _rng(seed)
    video = torch.randn(B, CT, HW, generator=g)
    m = torch.randint(0, 2, (B, 1, HW), generator=g, dtype=torch.uint8)
    binmask = torch.cat([m, 1 - m, 1 - m], 1).reshape(-1).contiguous()
    src = torch.tensor([2, 0, 1] if B == 3 else [1, 0], dtype=torch.int32)
    partner = torch.tensor([0, 0, 1] if B == 3 else [0, 0], dtype=torch.int32)
    aug = torch.tensor([1, 0, 1][:B], dtype=torch.int32)
    return video, binmask, 3 * HW, src, partner, aug


# ---- frame differences + colour bins -------------------------------------------------------------------------------------------
def _denorm32(video):
    std = torch.tensor(STD, dtype=torch.float32).view(1, 3, 1, 1, 1)
    mean = torch.tensor(MEAN, dtype=torch.float32).view(1, 3, 1, 1, 1)
    return (video * std) + mean                                                   # two fp32 roundings, as __fadd_rn(__fmul_rn(x, std), mean)


def diffs_ref(video):
    """video [B, 3, T, H, W] fp32 -> diffs [B, 1 + T/2, H, W] fp32 in the kernel's operation order: cur = fl(fl(x std) + mean); d_t = (|dc0| + |dc1|) + |dc2| between
    frames t - 1 and t; slot 1 + i = d_(2i+1); slot 0 = (((d_1 + d_2) + ...) + d_(T-1)) / (T - 1), one division."""
    B, C, T, H, W = video.shape
    cur = _denorm32(video)
    a = (cur[:, :, :-1] - cur[:, :, 1:]).abs()                                    # [B, 3, T-1, H, W]
    d = (a[:, 0] + a[:, 1]) + a[:, 2]                                             # [B, T-1, H, W]
    dsum = d[:, 0].clone()
    for t in range(1, T - 1):
        dsum = dsum + d[:, t]
    return torch.cat([(dsum / float(T - 1))[:, None], d[:, 0::2]], 1)


def bin_coordinates(video):
    """float64: the three pre-rounding bin coordinates [B, H*W, 3] of the kernel's formula (kornia rgb_to_hsv of the temporal mean of the denormalised clip, hue in
    [0, 2 pi] multiplied by 2 pi once more as the reference does; coordinates hx 9 + 1, hy 9 + 1, v 9 + 1)"""
    B, C, T, H, W = video.shape
    std = torch.tensor(STD, dtype=torch.float32).double().view(1, 3, 1, 1, 1)
    mean = torch.tensor(MEAN, dtype=torch.float32).double().view(1, 3, 1, 1, 1)
    img = (video.double() * std + mean).mean(2).reshape(B, 3, H * W)
    r, g, b = img[:, 0], img[:, 1], img[:, 2]
    mx, am = img.max(1)                                                           # first maximum, as the kernel's strict >
    mn = img.min(1)[0]
    delta = mx - mn
    s = delta / (mx + 1e-8)
    delta = torch.where(delta == 0, torch.ones_like(delta), delta)
    rc, gc, bc = mx - r, mx - g, mx - b
    h = torch.where(am == 0, bc - gc, torch.where(am == 1, (rc - bc) + 2.0 * delta, (gc - rc) + 4.0 * delta)) / delta
    h = (h / 6.0) % 1.0
    ang = (2.0 * math.pi * h) * (2.0 * math.pi)
    hx, hy = (s * torch.cos(ang) + 1.0) / 2.0, (s * torch.sin(ang) + 1.0) / 2.0
    return torch.stack([hx * 9.0 + 1.0, hy * 9.0 + 1.0, mx * 9.0 + 1.0], -1)


def color_candidates(video):
    """[B, H*W, 8] int64: every bin reachable when each coordinate moves by +- BIN_MARGIN before it is rounded -- at most 8 distinct bins per pixel, each built with the
    kernel's formula h + (s - 1) 10 + (v - 1) 100 and its clamp to 0..999.  No pixel is excluded: a device bin must be one of its pixel's candidates."""
    c = bin_coordinates(video)
    lo, hi = torch.round(c - BIN_MARGIN).long(), torch.round(c + BIN_MARGIN).long()
    out = []
    for ih in (lo, hi):
        for i_s in (lo, hi):
            for iv in (lo, hi):
                out.append((ih[..., 0] + (i_s[..., 1] - 1) * 10 + (iv[..., 2] - 1) * 100).clamp(0, 999))
    return torch.stack(out, -1)


def single_candidate_fraction(cands):
    return float((cands == cands[..., :1]).all(-1).double().mean())


def checked_candidates(video):
    """color_candidates of a test input, asserting that the input pins the kernel down: at least 90 % of its pixels have exactly one candidate"""
    cands = color_candidates(video)
    frac = single_candidate_fraction(cands)
    assert frac >= 0.9, f"only {frac:.3f} of the pixels have a single candidate bin: the input shows too little"
    return cands


def _normalise(rgb):
    """fp32 clip values that denormalise (about) to rgb [..., 3, ...] on dim 1"""
    std = torch.tensor(STD, dtype=torch.float32).view(1, 3, 1, 1, 1)
    mean = torch.tensor(MEAN, dtype=torch.float32).view(1, 3, 1, 1, 1)
    return (rgb - mean) / std


def _exact_grey(v):
    """per channel an fp32 x with fl(fl(x std) + mean) == v exactly: the three channels tie bitwise and the kernel's delta == 0 branch runs"""
    xs = []
    for c in range(3):
        s, m = torch.tensor(STD[c]), torch.tensor(MEAN[c])
        x = (torch.tensor(v) - m) / s
        for _ in range(64):
            got = x * s + m
            if float(got) == float(torch.tensor(v)):
                break
            x = torch.nextafter(x, torch.tensor(math.inf if float(got) < v else -math.inf))
        else:
            raise AssertionError("no exact grey")
        xs.append(x)
    return torch.stack(xs)


PLANTED = ("grey", "near_black", "two_channels_tie_for_max", "static", "hue_below_wrap")


def color_inputs(B, T, H, W, seed=0):
    """A clip whose denormalised values are uniform in [0, 1], with five planted pixels at the start of clip 0 (constant in time unless noted):
    grey (bitwise r == g == b: delta == 0, hx = hy = 0.5 lands on the rounding tie 5.5), near-black (max channel 0.02: hue and saturation from tiny differences),
    two channels tied bitwise for the maximum (the strict > keeps the first), static (random colour, identical frames: its diffs are exactly 0) and a hue just below the
    wrap (red maximum, green a little under blue: (h / 6) mod 1 = 0.999, the angle 4 pi^2 * 0.999)."""
    g = _rng(seed)
    video = _normalise(torch.rand(B, 3, T, H, W, generator=g))
    flat = video[0].reshape(3, T, H * W)
    flat[:, :, 0] = _exact_grey(0.625)[:, None]
    flat[:, :, 1] = _normalise(torch.tensor([0.02, 0.012, 0.005]).view(1, 3, 1, 1, 1)).reshape(3, 1)
    tie = _exact_grey(0.75)
    flat[:, :, 2] = torch.stack([tie[0], tie[1], _normalise(torch.tensor([0.0, 0.0, 0.25]).view(1, 3, 1, 1, 1)).reshape(3)[2]])[:, None]
    flat[:, :, 3] = flat[:, :1, 3].clone()
    flat[:, :, 4] = _normalise(torch.tensor([0.8, 0.297, 0.3]).view(1, 3, 1, 1, 1)).reshape(3, 1)
    return video.contiguous()


def wide_color_inputs(B, T, H, W, seed=0):
    """values that denormalise into [-0.2, 1.3] (what a colour-jittered clip can hold), with one all-negative and one all-above-one pixel planted: bins computed from
    them fall outside 0..999 before the clamp.  Only the clamp is asserted on this clip."""
    g = _rng(seed)
    video = _normalise(torch.rand(B, 3, T, H, W, generator=g) * 1.5 - 0.2)
    flat = video[0].reshape(3, T, H * W)
    flat[:, :, 0] = _normalise(torch.tensor([-0.2, -0.1, -0.15]).view(1, 3, 1, 1, 1)).reshape(3, 1)
    flat[:, :, 1] = _normalise(torch.tensor([1.3, 1.25, 1.1]).view(1, 3, 1, 1, 1)).reshape(3, 1)
    return video.contiguous()


# ---- blur -----------------------------------------------------------------------------------------------------------------------
def gaussian_taps64(ksize, sigma):
    x = torch.arange(ksize, dtype=torch.float64) - ksize // 2
    g = torch.exp(-x * x / (2.0 * float(sigma) ** 2))
    return g / g.sum()


def blur_roundings(ksize):
    """The number of unit roundoffs in blur_ref's bound.
    Each pass is one sequential chain of ksize multiply-adds from a = 0 (fame.hip: a += w[k] * tile), fused or not: ksize + 1 roundings on the sum of absolute terms
    (the standard bound of a length-n chain, n u sum |w||x|, plus one for an unfused product).  Two passes.
    Each pass also carries the error of its taps, computed on the host in fp32 (devias_fame_blur): the argument -(x x) / (2 sigma sigma) takes 3 roundings (x x is an
    exact integer) and |argument| <= 1.2 for sigma >= ksize / 3, so the exponential moves by 1.2 * 3 u, plus 2 u for expf itself; the normalising sum is a chain of
    ksize additions of positive terms (ksize u) and the division adds 1: ksize + 6.6, rounded up to ksize + 8.  Two passes.
    Total 2 (ksize + 1) + 2 (ksize + 8) = 4 ksize + 18."""
    return 2 * (ksize + 1) + 2 * (ksize + 8)


def blur_ref(x, ksize, sigma):
    """x [n, H, W] fp32 -> (float64 blur [n, H, W], per-element bound).

    The ideal result is y = w (*)_y (w (*)_x x) with exact taps w = exp(-j^2 / (2 sigma^2)) / sum, border 'reflect' (sigma is the fp32 value the entry point receives).
    Derivation of the bound, the way kernel_bounds.py bounds its sums: the kernel computes fl-chains with taps w^ = w (1 + e_w), |e_w| <= (ksize + 8) u.  The row pass
    returns p^ = p + dp with |dp| <= ((ksize + 1) + (ksize + 8)) u (|w| (*) |x|); the column pass applied to p^ adds the same factor on |w| (*) |p^| and carries dp
    through |w| (*) |dp|.  With |p^| <= |w| (*) |x| to first order both terms are multiples of A = |w| (*)_y (|w| (*)_x |x|), so
        |y^ - y| <= blur_roundings(ksize) u A        (first order in u; 4 ksize + 18 <= 142 roundings, second-order terms are below 1e-5 of it).
    Valid for sigma >= ksize / 3 (the taps' exponent stays in [-1.2, 0]); FAME uses sigma = ksize / 3."""
    import torch.nn.functional as F
    assert float(sigma) >= ksize / 3 - 1e-6
    sigma = float(torch.tensor(sigma, dtype=torch.float32))
    w = gaussian_taps64(ksize, sigma)
    R = ksize // 2
    n, H, W = x.shape

    def conv(v):
        v = F.pad(v.double()[:, None], (R, R, R, R), mode="reflect") if R else v.double()[:, None]
        v = F.conv2d(v, w.view(1, 1, 1, ksize))
        return F.conv2d(v, w.view(1, 1, ksize, 1))[:, 0]
    return conv(x), blur_roundings(ksize) * U32 * conv(x.abs())


def blur_inputs(n, H, W, seed=0):
    """non-negative like the pipeline's images, graded by row over 2^0 .. 2^-8 so that an error confined to a dim region is not hidden by the image's largest values"""
    g = _rng(seed)
    grade = 2.0 ** -(torch.arange(H) % 9).float()
    return torch.rand(n, H, W, generator=g) * grade.view(1, H, 1)


def excess(out, ref, bound):
    """max |out - ref| / bound; where the bound is 0 the output must equal the reference"""
    err = (out.double() - ref).abs()
    if bool(((bound == 0) & (err > 0)).any()):
        return math.inf
    return float((err / bound.clamp_min(1e-300)).max())


MUTANTS = {m: "select" for m in SELECT_MUTANTS}
MUTANTS.update({m: "pool" for m in POOL_MUTANTS})
MUTANTS.update({m: "refine" for m in REFINE_MUTANTS})
MUTANTS.update({m: "mix" for m in MIX_MUTANTS})
