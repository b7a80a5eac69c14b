"""Clip ingest without a GPU: ClipIngest's host draw against the boxes and flips the real reference drew for every case of tests/golden/ingest_vectors.npz
(tests/golden/make_ingest_goldens.py) and the generator states it left; center_box / test_box against the recorded validation / test crops; the CPU path within the
float64 bound of tests/ingest_bounds.py; IngestLoader; the C ABI's new entry."""
import ctypes
import random

import numpy as np
import pytest
import torch

import ingest_bounds as ib

FX = ib.load_fixture()
TAB = ib.table32()
TRAIN = [n for n, c in FX.items() if c["kind"] == "train"]
CENTER = [n for n, c in FX.items() if c["kind"] == "center"]
TEST = [n for n, c in FX.items() if c["kind"] == "test"]


def make(c, **kw):
    from devias_amd.ingest import ClipIngest
    return ClipIngest(c["S"], scale=tuple(c["scale"].tolist()), ratio=tuple(c["ratio"].tolist()), flip=bool(c["flip_on"]), **kw)


def test_the_fixture_covers_what_it_must():
    assert len(TRAIN) >= 12 and len(CENTER) >= 4 and len(TEST) >= 8
    assert {c["S"] for c in FX.values()} == {16, 20} and {c["frames"].shape[0] for c in FX.values()} == {2}
    assert {c["frames"].shape[1:3] for c in FX.values() if c["kind"] != "test"} == {(20, 27), (37, 23), (40, 40), (8, 200)}
    seen = set()
    for c in FX.values():
        (i, j, h, w, fl), (H0, W0), S = c["box"], c["frames"].shape[1:3], c["S"]
        seen |= {n for n, hit in (("top", i == 0), ("left", j == 0), ("bottom", i + h == H0), ("right", j + w == W0), ("w1", w == 1), ("h1", h == 1), ("flip", fl == 1),
                                  ("no_flip", fl == 0), ("up", h < S or w < S), ("down", h > S or w > S), ("identity", h == S and w == S),
                                  ("fallback", (H0, W0) == (8, 200) and (h, w) == (8, 11))) if hit}
    assert seen == {"top", "left", "bottom", "right", "w1", "h1", "flip", "no_flip", "up", "down", "identity", "fallback"}
    assert any(not c["flip_on"] for c in FX.values())


@pytest.mark.parametrize("name", TRAIN)
def test_draw_reproduces_the_reference_box_flip_and_generator_states(name):
    c = FX[name]
    m = make(c, device="cpu")
    random.seed(int(c["seeds"][0]))
    np.random.seed(int(c["seeds"][1]))
    assert m.draw(*c["frames"].shape[1:3]) == c["box"]
    assert random.random() == c["next"][0] and np.random.uniform() == c["next"][1]          # both generators are where the reference left them


def test_a_sequence_of_draws_is_the_sequence_of_single_draws():
    """the draw keeps no state of its own: two clips drawn in a row consume what two reference calls consume"""
    a, b = FX[TRAIN[0]], FX[TRAIN[4]]
    m = make(a, device="cpu")
    random.seed(3)
    np.random.seed(4)
    first = m.draw(*a["frames"].shape[1:3])
    state = (random.getstate(), np.random.get_state()[1].copy())
    second = m.draw(*b["frames"].shape[1:3])
    random.seed(3)
    np.random.seed(4)
    assert m.draw(*a["frames"].shape[1:3]) == first
    assert random.getstate() == state[0] and np.array_equal(np.random.get_state()[1], state[1])
    assert m.draw(*b["frames"].shape[1:3]) == second


def test_center_and_test_boxes_are_the_recorded_crops_and_draw_nothing():
    random.seed(1)
    np.random.seed(1)
    before = (random.getstate(), np.random.get_state()[1].copy())
    for name in CENTER:
        c = FX[name]
        assert make(c, device="cpu").center_box(*c["frames"].shape[1:3]) == c["box"], name
    for name in TEST:
        c = FX[name]
        assert make(c, device="cpu").test_box(*c["frames"].shape[1:3], int(c["split"][0]), int(c["split"][1])) == c["box"], name
    assert random.getstate() == before[0] and np.array_equal(np.random.get_state()[1], before[1])
    m = make(FX[CENTER[0]], device="cpu")
    with pytest.raises(ValueError, match="smaller"):
        m.center_box(8, 200)
    with pytest.raises(ValueError, match="short side"):
        m.test_box(20, 27, 0, 3)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_cpu_path_lies_within_the_bound_and_identity_boxes_are_the_reference_bitwise(dtype):
    bf16 = dtype == torch.bfloat16
    for name, c in FX.items():
        m = make(c, out_dtype=dtype, device="cpu")
        out = m(torch.from_numpy(c["frames"])[None], [c["box"]])
        assert out.dtype == dtype and tuple(out.shape) == (1, 3, 2, c["S"], c["S"])
        got = out[0].float().numpy()
        ref, M = ib.statement(c["frames"], c["box"], c["S"], c["S"], TAB)
        r, k = ib.worst(got, ref, ib.bound(ref, M, bf16))
        assert r <= 1.0, (name, r, k)
        assert np.array_equal(got.view(np.uint32), ib.emulate(c["frames"], c["box"], c["S"], c["S"], TAB, bf16=bf16).view(np.uint32)), name
        if c["kind"] != "train" and not bf16:
            assert np.array_equal(got.view(np.uint32), c["out"].view(np.uint32)), name
        if not bf16:          # the golden: the triangle inequality through the float64 statement, no margin
            assert bool((np.abs(got.astype(np.float64) - c["out"]) <= ib.bound(ref, M) + c["ref_dist"]).all()), name


def test_call_draws_in_batch_order_and_accepts_a_ragged_list():
    a, b = FX[TRAIN[0]], FX[TRAIN[2]]
    m = make(a, device="cpu")
    fa, fb = torch.from_numpy(a["frames"]), torch.from_numpy(b["frames"])
    random.seed(5)
    np.random.seed(6)
    out = m([fa, fb])
    random.seed(5)
    np.random.seed(6)
    boxes = [m.draw(*fa.shape[1:3]), m.draw(*fb.shape[1:3])]
    assert torch.equal(out, m([fa, fb], boxes)) and torch.equal(out[1], m(fb[None], boxes[1:])[0])
    with pytest.raises(ValueError, match="leaves"):
        m(fa[None], [(0, 0, 21, 5, 0)])
    with pytest.raises(ValueError, match="uint8"):
        m(fa[None].float(), [(0, 0, 5, 5, 0)])
    with pytest.raises(ValueError, match="boxes"):
        m([fa, fb], boxes[:1])


def test_ingest_loader_replaces_field_zero_and_nothing_else():
    import devias_amd
    from devias_amd.ingest import ClipIngest, IngestLoader
    assert devias_amd.ClipIngest is ClipIngest and devias_amd.IngestLoader is IngestLoader
    c = FX[CENTER[0]]
    m = make(c, device="cpu")
    frames = torch.from_numpy(np.stack([c["frames"], c["frames"][::-1].copy()]))
    labels, names, idx = torch.tensor([3, 4]), ["a", "b"], torch.tensor([7, 8])
    src = [(frames, labels, names, idx), [frames, labels, names, idx]]
    got = list(IngestLoader(src, m, mode="center"))
    assert len(IngestLoader(src, m)) == 2 and type(got[0]) is tuple and type(got[1]) is list
    for batch in got:
        assert len(batch) == 4 and batch[1] is labels and batch[2] is names and batch[3] is idx
        assert torch.equal(batch[0], m(frames, [c["box"]] * 2))
    # "test": split_nb from field 4, where the reference's test dataset puts it
    v = [FX[n] for n in TEST[:3]]
    assert all(np.array_equal(x["frames"], v[0]["frames"]) for x in v)
    fr = torch.from_numpy(np.stack([x["frames"] for x in v]))
    batch, = list(IngestLoader([(fr, torch.zeros(3), ["n"] * 3, torch.zeros(3, dtype=torch.int64), torch.tensor([int(x["split"][0]) for x in v]))], make(v[0], device="cpu"), mode="test", num_crop=3))
    assert np.array_equal(batch[0].numpy().view(np.uint32), np.stack([x["out"] for x in v]).view(np.uint32))
    # "train": the draws of the wrapped call, in batch order
    t = FX[TRAIN[0]]
    mt = make(t, device="cpu")
    ft = torch.from_numpy(np.stack([t["frames"]] * 2))
    random.seed(9)
    np.random.seed(9)
    batch, = list(IngestLoader([(ft, labels)], mt, mode="train"))
    random.seed(9)
    np.random.seed(9)
    assert torch.equal(batch[0], mt(ft)) and batch[1] is labels
    with pytest.raises(ValueError, match="mode"):
        IngestLoader(src, m, mode="val")


def test_abi_179_entry_resolves_and_validates_before_any_launch():
    from devias_amd import _lib
    assert _lib.ABI_VERSION >= 179
    lib = _lib.load()
    assert lib.devias_version() >= 179 and "devias_clip_ingest" in _lib.PROTOTYPES and hasattr(lib, "devias_clip_ingest")
    assert ctypes.sizeof(_lib.IngestRow) == 40
    one = ctypes.c_void_p(16)          # never dereferenced: validation comes first
    H0, W0, T = 20, 27, 2
    nbytes = T * H0 * W0 * 3

    def call(row=None, src=one, table=one, out=one, B=1, T_=T, S_h=16, S_w=16, dtype=_lib.F32, n=nbytes, rows=True):
        r = (_lib.IngestRow * 2)()
        for k in range(2):
            r[k] = _lib.IngestRow(0, H0, W0, 1, 2, 5, 6, 0, 0)
        if row is not None:
            r[B - 1] = _lib.IngestRow(*row)
        rc = lib.devias_clip_ingest(src, n, table, r if rows else None, B, T_, S_h, S_w, dtype, out, None)
        return rc, lib.devias_last_error()

    for kw in (dict(src=None), dict(table=None), dict(out=None), dict(rows=False)):
        rc, err = call(**kw)
        assert rc == -1 and b"devias_clip_ingest" in err and b"null" in err, kw
    for kw, word in ((dict(B=0), b"B="), (dict(T_=0), b"T="), (dict(S_h=0), b"S_h"), (dict(S_w=0), b"S_w"), (dict(dtype=7), b"out_dtype"),
                     (dict(row=(0, H0, W0, 1, 2, 0, 6, 0, 0)), b"empty box"), (dict(row=(0, H0, W0, 1, 2, 5, 0, 0, 0)), b"empty box"),
                     (dict(row=(0, H0, W0, 16, 2, 5, 6, 0, 0)), b"leaves"), (dict(row=(0, H0, W0, 1, 22, 5, 6, 0, 0)), b"leaves"),
                     (dict(row=(0, H0, W0, -1, 2, 5, 6, 0, 0)), b"leaves"), (dict(row=(0, H0, W0, 1, 2, 5, 6, 2, 0)), b"flip"),
                     (dict(row=(0, 0, W0, 0, 0, 1, 1, 0, 0)), b"H0"),
                     (dict(row=(1, H0, W0, 1, 2, 5, 6, 0, 0)), b"exceeds"), (dict(row=(-1, H0, W0, 1, 2, 5, 6, 0, 0)), b"exceeds"),
                     (dict(n=nbytes - 1), b"exceeds"), (dict(B=2, row=(nbytes, H0, W0, 1, 2, 5, 6, 0, 0)), b"rows[1]")):
        rc, err = call(**kw)
        assert rc == -1 and b"devias_clip_ingest" in err and word in err, (kw, err)
