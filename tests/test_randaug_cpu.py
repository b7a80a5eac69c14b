"""RandAugment without a GPU: the config parser, the draws and the two host statements of the arithmetic (devias_amd.randaug.randaug_cpu, tests/randaug_ref.py) against
what the real reference and Pillow produced (tests/golden/randaug_vectors.npz), bitwise; the loader keyword's draw order; the refused options; the ABI."""
import ctypes
import os
import random

import numpy as np
import pytest
import torch

import randaug_ref as rr

HERE = os.path.dirname(os.path.abspath(__file__))
FX = np.load(os.path.join(HERE, "golden", "randaug_vectors.npz"))
SETS = ("f20x27", "f37x23", "f1x9", "f9x1", "f2x2", "const5x4", "ext6x5")
INTEGER_ARG = ("Posterize", "PosterizeIncreasing", "Solarize", "SolarizeIncreasing", "SolarizeAdd")


def op_cases(fset):
    """(name, magnitude, negated, resampling code, level args as the reference passed them, Pillow's output) for every per-op case of a frame set"""
    for name, mag, neg, interp, arg, out in zip(*(FX[f"op.{fset}.{k}"] for k in ("name", "mag", "neg", "interp", "arg", "out"))):
        name = str(name)
        args = () if np.isnan(arg) else ((int(arg),) if name in INTEGER_ARG else (float(arg),))
        yield name, int(mag), int(neg), int(interp), args, out


def chains():
    """(k, config, interpolation, frames, seeds, layers [(name, applied, args)], output, next draws) per recorded chain"""
    for k in range(len(FX["chain.set"])):
        layers = []
        for name, ap, arg in zip(FX["chain.ops"][k], FX["chain.applied"][k], FX["chain.args"][k]):
            name = str(name)
            if name:
                layers.append((name, bool(ap), () if np.isnan(arg) else ((int(arg),) if name in INTEGER_ARG else (float(arg),))))
        yield (k, str(FX["chain.config"][k]), str(FX["chain.interp"][k]), FX["frames." + str(FX["chain.set"][k])], tuple(int(s) for s in FX["chain.seeds"][k]), layers,
               FX[f"chain.out.{k}"], tuple(FX["chain.next"][k]))


def test_the_fixture_covers_what_it_must():
    names = {c[0] for c in op_cases("f20x27")}
    from devias_amd.randaug import RAND_INCREASING_TRANSFORMS, RAND_TRANSFORMS
    assert set(RAND_INCREASING_TRANSFORMS) | set(RAND_TRANSFORMS) <= names
    applied = {n for c in chains() for n, ap, _ in c[5] if ap}
    assert set(RAND_INCREASING_TRANSFORMS) <= applied
    assert any(not ap for c in chains() for _, ap, _ in c[5])
    assert any(len({n for n, ap, _ in c[5] if ap}) < sum(ap for _, ap, _ in c[5]) for c in chains())
    assert {(c[1], c[2]) for c in op_cases("f20x27") if c[0] == "ShearX"} >= {(0, 0), (10, 0), (10, 1), (7, 0), (7, 1)}
    assert {c[3] for c in op_cases("f20x27") if c[0] == "Rotate"} == {rr.BILINEAR, rr.BICUBIC}
    assert os.path.getsize(os.path.join(HERE, "golden", "randaug_vectors.npz")) <= 550 * 1024


def test_config_parser_reads_what_the_reference_reads():
    from devias_amd.randaug import parse_config
    assert len(FX["parse.config"]) >= 8
    for config, (m, n, mstd, inc, weighted) in zip(FX["parse.config"], FX["parse.values"]):
        got = parse_config(str(config))
        assert got[0] == m and got[1] == n and (got[2] is not None) == bool(weighted) and got[4] == bool(inc), (config, got)
        assert (got[3] is None and np.isnan(mstd)) or got[3] == mstd, (config, got)
    with pytest.raises(ValueError, match="rand"):
        parse_config("augmix-m5")


def test_constructor_builds_the_reference_hparams_and_refuses_what_it_does_not_serve():
    from devias_amd import randaug as R
    ra = R.RandAugment(device="cpu")
    assert (ra.magnitude, ra.num_layers, ra.resample, ra.transforms) == (7, 4, R.BICUBIC, R.RAND_INCREASING_TRANSFORMS)
    assert ra.hparams == {"translate_const": 100, "interpolation": R.BICUBIC, "img_mean": (128, 128, 128), "magnitude_std": 0.5}
    assert R.RandAugment("rand-m9-n3", "bilinear", input_size=(160, 224), device="cpu").hparams["translate_const"] == 72
    assert R.RandAugment("rand-m9-n3", device="cpu").transforms == R.RAND_TRANSFORMS
    with pytest.raises(NotImplementedError, match="random.choice"):
        R.RandAugment(interpolation="random")
    with pytest.raises(NotImplementedError, match="without replacement|WITHOUT replacement"):
        R.RandAugment("rand-m7-n4-w0")
    with pytest.raises(ValueError, match="interpolation"):
        R.RandAugment(interpolation="lanczos")


def test_draw_reproduces_every_recorded_chain_and_leaves_both_generators_where_the_reference_does():
    from devias_amd.randaug import RandAugment
    n = 0
    for k, config, interp, frames, seeds, layers, out, nxt in chains():
        ra = RandAugment(config, interp, device="cpu")
        random.seed(seeds[0])
        np.random.seed(seeds[1])
        plan = ra.draw()
        assert (random.random(), np.random.uniform()) == nxt, k
        assert plan == layers, (k, plan, layers)
        n += 1
    assert n >= 10
    ra = RandAugment(device="cpu")                           # a SEQUENCE of draws: two clips after one seeding are two consecutive reference calls
    random.seed(77)
    np.random.seed(78)
    two = [ra.draw(), ra.draw()]
    random.seed(77)
    np.random.seed(78)
    assert [ra.draw(), ra.draw()] == two and two[0] != two[1]


@pytest.mark.parametrize("fset", SETS)
def test_both_host_statements_are_bitwise_pillow_on_every_per_op_case(fset):
    from devias_amd.randaug import randaug_cpu
    frames, n = FX["frames." + fset], 0
    for name, mag, neg, interp, args, out in op_cases(fset):
        got = randaug_cpu(frames, [(name, True, args)], interp)
        assert got.dtype == np.uint8 and np.array_equal(got, out), ("randaug_cpu", fset, name, mag, neg, interp)
        ref = rr.randaug_ref(frames, [(name, True, args[0] if args else None)], interp)
        assert np.array_equal(ref, out), ("randaug_ref", fset, name, mag, neg, interp)
        n += 1
    assert n >= 24


def test_both_host_statements_are_bitwise_pillow_on_every_chain():
    from devias_amd.randaug import BICUBIC, BILINEAR, randaug_cpu
    for k, config, interp, frames, seeds, layers, out, nxt in chains():
        code = BICUBIC if interp == "bicubic" else BILINEAR
        assert np.array_equal(randaug_cpu(frames, layers, code), out), k
        assert np.array_equal(rr.randaug_ref(frames, [(n, ap, a[0] if a else None) for n, ap, a in layers], code), out), k
        t = randaug_cpu(torch.from_numpy(frames), layers, code)
        assert isinstance(t, torch.Tensor) and t.dtype == torch.uint8 and np.array_equal(t.numpy(), out)


def test_identities_are_lowered_to_no_op_and_the_rest_to_what_pil_hands_to_c():
    from devias_amd import randaug as R
    none = (R.OP_NONE, (0.0,) * 6, 0.0, 0, 0)
    assert R.lower("Rotate", (0.0,), 20, 27) == none and R.lower("Rotate", (360.0,), 20, 27) == none
    assert R.lower("ColorIncreasing", (1.0,), 20, 27) == none and R.lower("Sharpness", (1.0,), 20, 27) == none
    assert R.lower("Posterize", (8,), 20, 27) == none and R.lower("PosterizeIncreasing", (4,), 20, 27)[:1] + R.lower("PosterizeIncreasing", (4,), 20, 27)[3:] == (R.OP_POSTERIZE, 0xf0, 0)
    assert R.lower("PosterizeIncreasing", (0,), 20, 27)[3] == 0
    assert R.lower("TranslateXRel", (0.25,), 20, 27)[1] == (1.0, 0.0, 6.75, 0.0, 1.0, 0.0) and R.lower("TranslateYRel", (-0.25,), 20, 27)[1][5] == -5.0
    assert R.lower("ShearX", (0.3,), 20, 27, R.BILINEAR)[3] == R.BILINEAR
    assert R.lower("Brightness", (0.1,), 20, 27)[2] == float(np.float32(0.1))
    assert R.lower("SolarizeAdd", (77,), 20, 27)[3:] == (77, 128)
    assert R.lower("ShearX", (0.0,), 20, 27)[0] == R.OP_AFFINE            # PIL runs the transform; only the three identities above are skipped
    m = R.lower("Rotate", (30.0,), 20, 27)[1]
    assert m[0] == round(np.cos(np.radians(-30.0)), 15) and m[1] == -m[3]


def _loader_inputs():
    g = torch.Generator().manual_seed(4)
    clips = [torch.randint(0, 256, (2, 20, 27, 3), dtype=torch.uint8, generator=g), torch.randint(0, 256, (2, 37, 23, 3), dtype=torch.uint8, generator=g)]
    return clips, torch.tensor([1, 2])


def test_ingest_loader_with_randaug_draws_plan_then_box_per_clip():
    from devias_amd.ingest import ClipIngest, IngestLoader
    from devias_amd.randaug import RandAugment, randaug_cpu
    clips, labels = _loader_inputs()
    m, ra = ClipIngest(16, device="cpu"), RandAugment(device="cpu")
    random.seed(31)
    np.random.seed(32)
    batch, = list(IngestLoader([(clips, labels)], m, mode="train", randaug=ra))
    after = (random.random(), np.random.uniform())
    random.seed(31)
    np.random.seed(32)
    want = []
    for c in clips:                                           # _aug_frame: the clip's RandAugment first, then its crop box and flip
        plan = ra.draw()
        box = m.draw(c.shape[1], c.shape[2])
        want.append(m(randaug_cpu(c, plan)[None], [box])[0])
    assert (random.random(), np.random.uniform()) == after
    assert batch[1] is labels and torch.equal(batch[0], torch.stack(want))
    for mode in ("center", "test"):
        with pytest.raises(ValueError, match="randaug"):
            IngestLoader([(clips, labels)], m, mode=mode, randaug=ra)


def test_ingest_loader_without_randaug_consumes_the_generators_as_before():
    from devias_amd.ingest import ClipIngest, IngestLoader
    clips, labels = _loader_inputs()
    m = ClipIngest(16, device="cpu")
    random.seed(41)
    np.random.seed(42)
    batch, = list(IngestLoader([(clips, labels)], m, mode="train"))
    after = (random.random(), np.random.uniform())
    random.seed(41)
    np.random.seed(42)
    boxes = [m.draw(c.shape[1], c.shape[2]) for c in clips]   # all boxes, in batch order, and nothing else
    assert (random.random(), np.random.uniform()) == after
    assert torch.equal(batch[0], m(clips, boxes))
    assert IngestLoader([(clips, labels)], m).randaug is None


def test_call_on_a_cpu_device_returns_the_form_it_was_given():
    from devias_amd.randaug import RandAugment, randaug_cpu
    import devias_amd
    assert devias_amd.RandAugment is RandAugment
    clips, _ = _loader_inputs()
    ra = RandAugment(device="cpu")
    random.seed(51)
    np.random.seed(52)
    plans = [ra.draw(), ra.draw()]
    out = ra(clips, plans)
    assert isinstance(out, list) and all(torch.equal(o, randaug_cpu(c, p)) for o, c, p in zip(out, clips, plans))
    batch = torch.stack([clips[0], clips[0].flip(1)])
    out = ra(batch, plans)
    assert out.shape == batch.shape and out.dtype == torch.uint8 and torch.equal(out[1], randaug_cpu(batch[1], plans[1]))
    random.seed(51)
    np.random.seed(52)
    assert torch.equal(ra(batch), out)                        # plans drawn per clip, in batch order
    with pytest.raises(ValueError, match="plans"):
        ra(clips, plans[:1])
    with pytest.raises(ValueError, match="uint8"):
        ra(batch.float())


def test_abi_180_entries_resolve_and_validate_before_any_launch():
    from devias_amd import _lib
    from devias_amd import randaug as R
    assert _lib.ABI_VERSION >= 180
    lib = _lib.load()
    assert lib.devias_version() >= 180
    for sym in ("devias_randaug_apply", "devias_randaug_stats", "devias_randaug_launches"):
        assert sym in _lib.PROTOTYPES and hasattr(lib, sym)
    assert ctypes.sizeof(_lib.RandaugRow) == 88 and _lib.RandaugRow.a.offset == 40
    hdr = open(os.path.join(HERE, "..", "include", "devias_amd.h")).read()
    for k, name in enumerate(("NONE", "AUTOCONTRAST", "EQUALIZE", "INVERT", "POSTERIZE", "SOLARIZE", "SOLARIZE_ADD", "COLOR", "CONTRAST", "BRIGHTNESS", "SHARPNESS", "AFFINE")):
        assert f"#define DEVIAS_RA_{name} {k}\n" in hdr and getattr(R, "OP_" + name) == k
    assert f"#define DEVIAS_RANDAUG_STATS_BYTES {_lib.RANDAUG_STATS_BYTES}\n" in hdr and f"#define DEVIAS_RANDAUG_ROWS_PER_LAUNCH {_lib.RANDAUG_ROWS_PER_LAUNCH}\n" in hdr
    lib.devias_counters_reset()
    one = ctypes.c_void_p(16)          # never dereferenced: validation comes first
    H0, W0, T = 20, 27, 2
    n = T * H0 * W0 * 3

    def row(op=R.OP_INVERT, src=0, dst=None, H=H0, W=W0, i0=0, i1=0, f=0.5, a=(1.0, 0.0, 0.0, 0.0, 1.0, 0.0)):
        r = _lib.RandaugRow(src, src if dst is None else dst, H, W, op, i0, i1, f)
        for k in range(6):
            r.a[k] = a[k]
        return r

    def call(fn, rows, buf=one, nbytes=2 * n, B=None, T_=T, stats=one, norows=False):
        arr = (_lib.RandaugRow * len(rows))(*rows)
        rc = getattr(lib, fn)(buf, nbytes, None if norows else arr, len(rows) if B is None else B, T_, stats, None)
        return rc, lib.devias_last_error()

    bad = [(dict(buf=None), b"null"), (dict(norows=True), b"null"), (dict(B=0), b"B="), (dict(T_=0), b"T="), (dict(nbytes=0), b"bytes")]
    bad_rows = [([row(op=12)], b"op"), ([row(op=-1)], b"op"), ([row(H=0)], b"H0"), ([row(W=20000)], b"W0"), ([row(src=n + 1)], b"exceeds"), ([row(src=-1)], b"exceeds"),
                ([row(dst=n)], b"in place"), ([row(op=R.OP_AFFINE, i0=3)], b"apart"), ([row(op=R.OP_SHARPNESS, dst=n - 1)], b"apart"),
                ([row(op=R.OP_AFFINE, i0=3, dst=n + 1)], b"exceeds"), ([row(op=R.OP_AFFINE, i0=1, dst=n)], b"resampling"),
                ([row(op=R.OP_AFFINE, i0=3, dst=n, a=(1.0, float("nan"), 0.0, 0.0, 1.0, 0.0))], b"finite"), ([row(op=R.OP_COLOR, f=float("inf"))], b"finite"),
                ([row(op=R.OP_POSTERIZE, i0=256)], b"i0"), ([row(op=R.OP_SOLARIZE, i0=257)], b"i0"), ([row(op=R.OP_SOLARIZE_ADD, i0=5, i1=-1)], b"i1"),
                ([row(), row(src=n - 1)], b"overlap"), ([row(op=R.OP_SHARPNESS, dst=n), row(src=n)], b"overlap")]
    for fn in ("devias_randaug_apply", "devias_randaug_stats"):
        for kw, word in bad:
            rc, err = call(fn, [row()], **kw)
            assert rc == -1 and fn.encode() in err and word in err, (fn, kw, err)
        for rows, word in bad_rows:
            rc, err = call(fn, rows)
            assert rc == -1 and fn.encode() in err and word in err, (fn, word, err)
        rc, err = call(fn, [row(op=R.OP_CONTRAST)], stats=None)
        assert rc == -1 and b"stats" in err
        # rows that ask for nothing launch nothing: no device is needed to return success
        assert call(fn, [row(op=R.OP_NONE, src=-5, H=0)])[0] == 0
    assert call("devias_randaug_stats", [row()])[0] == 0       # Invert needs no statistics: nothing to launch
    assert lib.devias_randaug_launches() == 0
