"""The clip ingest (devias_clip_ingest, devias_amd/ingest.py) stated in float64, the per-element bound its fp32 arithmetic must keep, and an fp32 emulation with
switchable defects.  A plain helper module (like kernel_bounds.py): no fixtures, no plugin, numpy only; importing it needs no GPU.

    table32(mean, std)                      the 768 normalised taps fl(fl(fl(u / 255) - m_c) / s_c) in numpy fp32 (bitwise devias_amd.ingest.tap_table)
    coords(n_in, n_out, flip)               first tap, second tap and lambda of every output index: exact integers, lambda = remainder / (2 n_out) in float64
    statement(frames, box, S_h, S_w, tab)   (ref, M) float64 [3, T, S_h, S_w]: the transform with the fp32 table values as taps and exact rational coordinates, and the
                                            largest tap magnitude among each element's four taps
    bound(ref, M, bf16)                     the per-element bound, derived below
    emulate(frames, box, S_h, S_w, tab, defect, bf16)   the kernel's arithmetic in numpy fp32, one rounding per operation; `defect` switches one seeded mutation on
    load_fixture() / sweep_boxes(...)       the recorded cases of tests/golden/ingest_vectors.npz; a seeded sweep of boxes over one frame size

The bound.  U = 2^-24 (fp32 unit roundoff), every tap of the element has magnitude <= M.
  weights      lam^ = fl(r / (2 n_out)) with exact operands: |lam^ - lam| <= U lam <= U.  w0^ = fl(1 - lam^): |w0^ - (1 - lam)| <= U + U (1 - lam^) <= 2 U.
  horizontal   p^ = fl(fl(w0^ a) + fl(lam^ b)) against p = w0 a + lam b: the weights contribute (2 U + U) M, the two products U (w0^ |a| + lam^ |b|) <= U M (1 + 3 U), the sum
               U M (1 + 3 U)(1 + U):  |p^ - p| <= 5 U M + 8 U^2 M.
  vertical     out^ = fl(fl(wy0^ p^) + fl(ly^ q^)): the horizontal errors pass through with weight wy0^ + ly^ <= 1 + 3 U, the weights contribute 3 U M', the products and
               the sum 2 U M' with M' = M (1 + 5 U + ...):  |out^ - out| <= 10 U M + c U^2 M, c < 100.
  So fp32 output: 10 U M (1 + 2^-16); the factor covers the second-order terms (10 * 2^-16 U M = 655360 U^2 M) with room to spare and is not a tuning knob.
  bf16 output rounds that value once more: half a bf16 ulp at the binade of |ref| + the fp32 bound, 2^(floor(log2 v) - 8)."""
import numpy as np

U = 2.0 ** -24
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
DEFECTS = ("no_half_pixel", "i1_unclamped", "flip_before_crop", "channel_swap", "div256", "bf16_taps")


def to_bf16(x):
    """fp32 -> the nearest bf16 (ties to even), returned as fp32"""
    b = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    r = ((b >> np.uint32(16)) & np.uint32(1)) + np.uint32(0x7FFF)
    return ((b + r) & np.uint32(0xFFFF0000)).view(np.float32)


def table32(mean=MEAN, std=STD, divisor=255.0):
    u = np.arange(256, dtype=np.float32) / np.float32(divisor)
    m, s = np.asarray(mean, dtype=np.float32)[:, None], np.asarray(std, dtype=np.float32)[:, None]
    t = (u[None, :] - m) / s
    assert t.dtype == np.float32
    return t


def coords(n_in, n_out, flip=False, half_pixel=True, clamp=True):
    """src = max((d + 0.5) n_in / n_out - 0.5, 0) = max(((2d + 1) n_in - n_out) / (2 n_out), 0): i0 the quotient, lambda the remainder over 2 n_out (exact integers; one
    float64 division), i1 = min(i0 + 1, n_in - 1).  flip: output index x reads source-side index n_out - 1 - x.  half_pixel / clamp False: the two coordinate defects."""
    d = np.arange(n_out, dtype=np.int64)
    if flip:
        d = n_out - 1 - d
    num = (2 * d + 1) * n_in - n_out if half_pixel else 2 * d * n_in
    den = 2 * n_out
    num = np.maximum(num, 0)
    i0, rem = num // den, num % den
    i1 = np.minimum(i0 + 1, n_in - 1) if clamp else i0 + 1
    return i0, i1, rem, den


def _taps(frames, box, tab, flip_first=False):
    """the box's taps [3, T, h + 1, w + 1] in tab's dtype: one extra row and column of what lies behind the box in the frame (zero past the frame), which only the
    unclamped defect ever reads"""
    i, j, h, w, flip = (int(v) for v in box)
    f = np.asarray(frames)
    if flip_first:
        f = f[:, :, ::-1, :]
    T, H0, W0, _ = f.shape
    x = np.zeros((3, T, h + 1, w + 1), dtype=tab.dtype)
    hh, ww = min(h + 1, H0 - i), min(w + 1, W0 - j)
    for c in range(3):
        x[c, :, :hh, :ww] = tab[c][f[:, i:i + hh, j:j + ww, c].astype(np.int64)]
    return x


def statement(frames, box, S_h, S_w, tab):
    i, j, h, w, flip = (int(v) for v in box)
    x = _taps(frames, box, tab.astype(np.float64))
    r0, r1, ry, dy = coords(h, S_h)
    c0, c1, rx, dx = coords(w, S_w, bool(flip))
    ly, lx = (ry.astype(np.float64) / dy)[:, None], rx.astype(np.float64) / dx
    a, b, c, d = x[:, :, r0][..., c0], x[:, :, r0][..., c1], x[:, :, r1][..., c0], x[:, :, r1][..., c1]
    ref = (1 - ly) * ((1 - lx) * a + lx * b) + ly * ((1 - lx) * c + lx * d)
    M = np.maximum(np.maximum(np.abs(a), np.abs(b)), np.maximum(np.abs(c), np.abs(d)))
    return ref, M


def bound(ref, M, bf16=False):
    b = 10.0 * U * M * (1.0 + 2.0 ** -16)
    if bf16:
        v = np.abs(ref) + b
        _, e = np.frexp(v)                                   # v = m 2^e, m in [0.5, 1): floor(log2 v) = e - 1
        b = b + np.where(v > 0, np.ldexp(1.0, e - 9), 0.0)
    return b


def emulate(frames, box, S_h, S_w, tab=None, defect=None, bf16=False):
    """numpy fp32, one rounding per operation, in the kernel's order: lam = fl(r / den), w0 = fl(1 - lam), fl(fl(wy0 fl(fl(wx0 a) + fl(lx b))) + fl(ly fl(fl(wx0 c) + fl(lx d))))"""
    assert defect is None or defect in DEFECTS
    if tab is None:
        tab = table32()
    if defect == "channel_swap":
        tab = table32(MEAN[::-1], STD[::-1])
    elif defect == "div256":
        tab = table32(divisor=256.0)
    elif defect == "bf16_taps":
        tab = to_bf16(tab)
    i, j, h, w, flip = (int(v) for v in box)
    if defect == "flip_before_crop":                         # the frame is mirrored, then the box cut at the same (i, j); no flip after the resize
        x = _taps(frames, box, tab, flip_first=bool(flip))
        flip = 0
    else:
        x = _taps(frames, box, tab)
    hp, cl = defect != "no_half_pixel", defect != "i1_unclamped"
    r0, r1, ry, dy = coords(h, S_h, False, hp, cl)
    c0, c1, rx, dx = coords(w, S_w, bool(flip), hp, cl)
    one = np.float32(1)
    ly = (ry.astype(np.float32) / np.float32(dy))[:, None]
    lx = rx.astype(np.float32) / np.float32(dx)
    wy0, wx0 = one - ly, one - lx
    a, b, c, d = x[:, :, r0][..., c0], x[:, :, r0][..., c1], x[:, :, r1][..., c0], x[:, :, r1][..., c1]
    out = wy0 * (wx0 * a + lx * b) + ly * (wx0 * c + lx * d)
    assert out.dtype == np.float32
    return to_bf16(out) if bf16 else out


def worst(got, ref, bnd):
    """(largest |got - ref| / bound, its flat index): <= 1 means every element is inside"""
    r = np.abs(np.asarray(got, dtype=np.float64) - ref) / bnd
    k = int(np.argmax(r))
    return float(r.reshape(-1)[k]), k


def load_fixture(path=None):
    """{case name: its entries} of tests/golden/ingest_vectors.npz (make_ingest_goldens.py), `frames` resolved to the case's uint8 [T, H0, W0, 3] array, in file order"""
    import os
    fx = np.load(path or os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ingest_vectors.npz"), allow_pickle=False)
    out = {}
    for name in (str(n) for n in fx["cases"]):
        c = {k: fx[f"{name}.{k}"] for k in ("S", "box", "out", "seeds", "scale", "ratio", "flip_on", "next", "split", "ref_dist")}
        cut = fx[name + ".cut"]
        c["frames"] = np.ascontiguousarray(fx["frames." + str(fx[name + ".src"])][:, :cut[0], :cut[1]])
        c["kind"], c["S"], c["box"], c["ref_dist"] = str(fx[name + ".kind"]), int(c["S"]), tuple(int(v) for v in c["box"]), float(c["ref_dist"])
        out[name] = c
    return out


def sweep_boxes(H0, W0, n, seed):
    """n boxes (i, j, h, w, flip) over an H0 x W0 frame from a seeded generator of its own: every size from one pixel to the whole frame, every position"""
    g = np.random.RandomState(seed)
    boxes = []
    for _ in range(n):
        h, w = int(g.randint(1, H0 + 1)), int(g.randint(1, W0 + 1))
        boxes.append((int(g.randint(0, H0 - h + 1)), int(g.randint(0, W0 - w + 1)), h, w, int(g.randint(0, 2))))
    return boxes
