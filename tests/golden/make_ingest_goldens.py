#!/usr/bin/env python3
"""Generate tests/golden/ingest_vectors.npz by RUNNING THE REAL REFERENCE (build container only) on small uint8 clips:

  train        dataset/kinetics.py's tensor_normalize and spatial_sampling(spatial_idx=-1, ...) -> video_transforms.random_resized_crop, horizontal_flip, after
               random.seed / np.random.seed.  The box is captured by wrapping _get_param_spatial_crop, the flip by wrapping horizontal_flip; the next draw of each
               generator after the call is recorded, so a replay can show that it consumed exactly the reference's random numbers.
  center       video_transforms.CenterCrop, volume_transforms.ClipToTensor, video_transforms.Normalize (the validation transform behind the short-side Resize)
  test         VideoClsDataset.__getitem__ in 'test' mode (kinetics.py:172-235) on an instance made without __init__, its decoder and short-side Resize replaced by the
               frames themselves: the view's window, ClipToTensor, Normalize

Per case: the two seeds, the uint8 frames [T, H0, W0, 3] (stored once per frame set; a case names its set and the top-left sub-frame it uses), S, the scale / ratio ranges, the drawn (i, j, h, w, flip), the reference's output [3, T, S, S] and the reference's
own largest distance from the float64 statement of tests/ingest_bounds.py.  T = 2, S in {16, 20}; frames 20 x 27, 37 x 23, 40 x 40 and one of 8 x 200, on which every attempt
fails (the smallest h the draw can produce is 10) and the fallback box is taken; the test views use sub-frames of those whose short side is S.  Boxes with h = 1 or w = 1
need a wider range than the recipe's (0.08, 1.0) x (0.75, 1.3333): those cases pass their own ranges to spatial_sampling, which takes them as arguments.
The absent imports (torchvision, cv2, decord, pandas) are stubbed in memory.  The script asserts the coverage the set must have.

Usage (in the build container):  python tests/golden/make_ingest_goldens.py
This script never runs on the GPU box and nothing under tests/ imports it."""
from __future__ import annotations

import os
import random
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference"
sys.dont_write_bytecode = True
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ingest_bounds as ib  # noqa: E402

T = 2
MEAN, STD = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]
RECIPE = ((0.08, 1.0), (0.75, 1.3333))
THIN = ((0.002, 0.06), (0.04, 25.0))           # boxes one pixel wide or high
FRAMES = {"f20x27": (20, 27), "f37x23": (37, 23), "f40x40": (40, 40), "f8x200": (8, 200)}


def install_reference():
    def _mod(name, **attrs):
        m = types.ModuleType(name)
        m.__dict__.update(attrs)
        sys.modules[name] = m
        return m

    tvt = _mod("torchvision.transforms", functional=_mod("torchvision.transforms.functional"))
    _mod("torchvision", transforms=tvt)
    _mod("cv2")
    _mod("decord", VideoReader=object, cpu=lambda *a: None)
    _mod("pandas")
    sys.path.insert(0, REF)
    import dataset.kinetics as kin
    import utils.transform.video_transforms as vt
    import utils.transform.volume_transforms as vol
    return kin, vt, vol


def frames_of(name):
    H0, W0 = FRAMES[name]
    g = np.random.RandomState(1000 * H0 + W0)
    return g.randint(0, 256, size=(T, H0, W0, 3)).astype(np.uint8)


def ref_distance(frames, box, S, out):
    ref, _ = ib.statement(frames, box, S, S, ib.table32())
    return float(np.abs(out.astype(np.float64) - ref).max())


def run_train(kin, vt, frames, S, ranges, flip_on, seeds):
    log = {}
    orig_box, orig_flip = vt._get_param_spatial_crop, vt.horizontal_flip

    def box(*a, **k):
        log["box"] = tuple(int(v) for v in orig_box(*a, **k))
        return log["box"]

    def flip(prob, images, boxes=None):
        out = orig_flip(prob, images, boxes)
        log["flip"] = int(out[0] is not images)
        return out

    vt._get_param_spatial_crop, vt.horizontal_flip = box, flip
    try:
        random.seed(seeds[0])
        np.random.seed(seeds[1])
        buf = kin.tensor_normalize(torch.from_numpy(frames), MEAN, STD).permute(3, 0, 1, 2)
        out = kin.spatial_sampling(buf, spatial_idx=-1, min_scale=256, max_scale=320, crop_size=S, random_horizontal_flip=flip_on, inverse_uniform_sampling=False,
                                   aspect_ratio=list(ranges[1]), scale=list(ranges[0]), motion_shift=False)
        nxt = np.array([random.random(), np.random.uniform()])
    finally:
        vt._get_param_spatial_crop, vt.horizontal_flip = orig_box, orig_flip
    b = log["box"] + (log.get("flip", 0),)
    return b, out.contiguous().numpy(), nxt


def run_center(vt, vol, frames, S):
    tf = vt.Compose([vt.CenterCrop(size=(S, S)), vol.ClipToTensor(), vt.Normalize(mean=MEAN, std=STD)])
    return tf([f for f in frames]).contiguous().numpy()


def run_test_view(kin, vt, vol, frames, S, split_nb, num_crop):
    ds = object.__new__(kin.VideoClsDataset)
    ds.mode, ds.args = "test", types.SimpleNamespace(data_set="Kinetics-400")
    ds.test_dataset, ds.test_seg, ds.test_label_array = ["v.mp4"], [(0, split_nb)], [0]
    ds.short_side_size, ds.clip_len, ds.test_num_segment, ds.test_num_crop = S, T, 1, num_crop
    ds.loadvideo_decord = lambda sample: frames
    ds.data_resize = vt.Compose([])
    ds.data_transform = vt.Compose([vol.ClipToTensor(), vt.Normalize(mean=MEAN, std=STD)])
    out = ds[0]
    assert out[4] == split_nb
    return out[0].contiguous().numpy()


def properties(H0, W0, S, b, fallback):
    i, j, h, w, fl = b
    p = {"flip" if fl else "no_flip"}
    p |= {n for n, hit in (("top", i == 0), ("left", j == 0), ("bottom", i + h == H0), ("right", j + w == W0), ("w1", w == 1), ("h1", h == 1)) if hit}
    if h < S or w < S:
        p.add("upscale")
    if h > S or w > S:
        p.add("downscale")
    if h == S and w == S:
        p.add("identity")
    if fallback:
        p.add("fallback")
    return p


def main():
    kin, vt, vol = install_reference()
    fx, names, seen = {}, [], set()

    for fname in FRAMES:                   # every frame set once; a case names its set and the top-left sub-frame it uses
        fx["frames." + fname] = frames_of(fname)

    def put(name, kind, fname, frames, S, b, out, seeds=(0, 0), ranges=RECIPE, flip_on=True, nxt=(0.0, 0.0), split=(0, 1)):
        names.append(name)
        assert np.array_equal(frames, fx["frames." + fname][:, :frames.shape[1], :frames.shape[2]])
        for k, v in (("kind", np.array(kind)), ("src", np.array(fname)), ("cut", np.array(frames.shape[1:3], dtype=np.int32)), ("S", np.array(S)), ("box", np.array(b, dtype=np.int32)), ("out", out.astype(np.float32)),
                     ("seeds", np.array(seeds, dtype=np.int64)), ("scale", np.array(ranges[0])), ("ratio", np.array(ranges[1])), ("flip_on", np.array(int(flip_on))),
                     ("next", np.array(nxt, dtype=np.float64)), ("split", np.array(split, dtype=np.int32)), ("ref_dist", np.array(ref_distance(frames, b, S, out)))):
            fx[f"{name}.{k}"] = v

    # ---- train: the first seeds as they come, then seeds searched for one property each
    plan = [("f20x27", 16, RECIPE, True, None), ("f20x27", 20, RECIPE, True, None), ("f37x23", 16, RECIPE, True, None), ("f37x23", 20, RECIPE, False, None),
            ("f40x40", 16, RECIPE, True, None), ("f40x40", 20, RECIPE, True, None), ("f8x200", 16, RECIPE, True, "fallback"), ("f8x200", 20, RECIPE, False, "fallback"),
            ("f20x27", 16, RECIPE, True, "top"), ("f37x23", 20, RECIPE, True, "left"), ("f40x40", 16, RECIPE, True, "bottom"), ("f20x27", 20, RECIPE, True, "right"),
            ("f37x23", 16, THIN, True, "w1"), ("f40x40", 20, THIN, True, "h1"), ("f20x27", 16, RECIPE, True, "identity"), ("f40x40", 16, RECIPE, True, "flip"),
            ("f37x23", 20, RECIPE, True, "no_flip")]
    for ci, (fname, S, ranges, flip_on, want) in enumerate(plan):
        frames = frames_of(fname)
        H0, W0 = FRAMES[fname]
        for s in range(5000 * ci, 5000 * ci + 5000):
            seeds = (s, 50000 + s)
            calls = {"n": 0}
            orig = random.randint

            def counting(a, b_):
                calls["n"] += 1
                return orig(a, b_)

            random.randint = counting
            try:
                b, out, nxt = run_train(kin, vt, frames, S, ranges, flip_on, seeds)
            finally:
                random.randint = orig
            p = properties(H0, W0, S, b, fallback=calls["n"] == 0)          # a successful attempt draws i and j; the fallback draws neither
            if want is None or want in p:
                break
        else:
            raise AssertionError(f"no seed gives {want} for train case {ci}")
        assert out.shape == (3, T, S, S)
        seen |= p
        put(f"t{ci:02d}", "train", fname, frames, S, b, out, seeds, ranges, flip_on, nxt)
    # ---- validation: the centre crop
    for ci, (fname, S) in enumerate((("f20x27", 16), ("f20x27", 20), ("f37x23", 16), ("f37x23", 20), ("f40x40", 16), ("f40x40", 20))):
        frames = frames_of(fname)
        H0, W0 = FRAMES[fname]
        b = (int(round((H0 - S) / 2.)), int(round((W0 - S) / 2.)), S, S, 0)
        out = run_center(vt, vol, frames, S)
        assert out.shape == (3, T, S, S)
        seen |= properties(H0, W0, S, b, False)
        put(f"c{ci:02d}", "center", fname, frames, S, b, out)
    # ---- test: the views of a frame whose short side is S (sub-frames of the four)
    k = 0
    for fname, S, cut in (("f20x27", 16, (16, 27)), ("f37x23", 20, (37, 20)), ("f40x40", 16, (40, 16))):
        frames = np.ascontiguousarray(frames_of(fname)[:, :cut[0], :cut[1], :])
        for num_crop, split_nb in ((3, 0), (3, 1), (3, 2), (1, 0)):
            out = run_test_view(kin, vt, vol, frames, S, split_nb, num_crop)
            assert out.shape == (3, T, S, S), out.shape
            # the window the reference cut: recovered by search over the long side (its arithmetic is restated by ClipIngest.test_box, which the tests hold to this)
            H0, W0 = cut
            tab = ib.table32()
            hits = [st for st in range(max(H0, W0) - S + 1)
                    if np.array_equal(ib.emulate(frames, (st, 0, S, S, 0) if H0 >= W0 else (0, st, S, S, 0), S, S, tab), out)]
            assert len(hits) == 1, hits
            b = (hits[0], 0, S, S, 0) if H0 >= W0 else (0, hits[0], S, S, 0)
            seen |= properties(H0, W0, S, b, False)
            put(f"v{k:02d}", "test", fname, frames, S, b, out, split=(split_nb, num_crop))
            k += 1
    need = {"fallback", "top", "left", "bottom", "right", "w1", "h1", "upscale", "downscale", "identity", "flip", "no_flip"}
    assert need <= seen, need - seen
    fx["cases"] = np.array(names)
    fx["mean"], fx["std"] = np.array(MEAN), np.array(STD)
    path = os.path.join(HERE, "ingest_vectors.npz")
    np.savez_compressed(path, **fx)
    worst = max(float(fx[n + ".ref_dist"]) for n in names)
    print(f"[ingest_vectors] {len(names)} cases, coverage {sorted(seen)}, the reference's largest distance from the float64 statement {worst:.3e}, "
          f"wrote {path} ({os.path.getsize(path) / 1024:.1f} KiB)")


if __name__ == "__main__":
    main()
