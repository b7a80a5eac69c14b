"""tests/ingest_bounds.py proved on the CPU, the way test_kernel_bounds_cpu.py proves kernel_bounds.py: an fp32 emulation of the ingest kernel's arithmetic lies inside the
per-element float64 bound on every recorded case and on the seeded sweep the GPU test runs, fp32 and bf16; each seeded defect lands outside it on at least one case."""
import numpy as np
import pytest

import ingest_bounds as ib

FX = ib.load_fixture()
TAB = ib.table32()
SWEEP = [(name, b) for name in ("t00", "t03", "t05", "t06") for b in ib.sweep_boxes(*FX[name]["frames"].shape[1:3], 12, seed=int(name[1:]))]
SWEEP += [(name, (0, 0) + FX[name]["frames"].shape[1:3] + (fl,)) for name, fl in (("t00", 0), ("t03", 1), ("t05", 0), ("t06", 1))]          # the whole frame: the buffer's first and last byte are taps


def _all_cases():
    for name, c in FX.items():
        yield name, c["frames"], c["box"], c["S"], c["S"]
    for name, b in SWEEP:
        yield name + str(b), FX[name]["frames"], b, 16, 20          # a sweep box is resized to 16 x 20: two output sizes in one call


def test_table_is_the_host_class_table_bitwise():
    from devias_amd.ingest import tap_table
    assert np.array_equal(tap_table().numpy().view(np.uint32), TAB.view(np.uint32))
    assert TAB.shape == (3, 256) and TAB.dtype == np.float32


def test_coordinates_are_the_half_pixel_rule():
    """against the rule evaluated in exact fractions"""
    from fractions import Fraction
    for n_in, n_out in ((1, 16), (11, 20), (16, 16), (27, 16), (200, 20), (340, 224)):
        i0, i1, rem, den = ib.coords(n_in, n_out)
        for d in range(n_out):
            src = max((Fraction(2 * d + 1, 2)) * Fraction(n_in, n_out) - Fraction(1, 2), Fraction(0))
            assert int(i0[d]) == src.numerator // src.denominator and Fraction(int(rem[d]), den) == src - int(i0[d])
            assert int(i1[d]) == min(int(i0[d]) + 1, n_in - 1)
        f0, _, frem, _ = ib.coords(n_in, n_out, flip=True)
        assert np.array_equal(f0, i0[::-1]) and np.array_equal(frem, rem[::-1])


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
def test_emulation_lies_inside_the_bound_on_every_case(bf16):
    worst = 0.0
    for name, frames, box, S_h, S_w in _all_cases():
        ref, M = ib.statement(frames, box, S_h, S_w, TAB)
        r, k = ib.worst(ib.emulate(frames, box, S_h, S_w, TAB, bf16=bf16), ref, ib.bound(ref, M, bf16))
        assert r <= 1.0, (name, r, k)
        worst = max(worst, r)
    print(f"[ingest bound, {'bf16' if bf16 else 'fp32'}] emulation at most {worst:.3f} of the bound")
    assert worst > 0.01          # the bound is of the size of the error, not orders above it


def test_identity_boxes_return_the_taps_bitwise():
    for name, c in FX.items():
        i, j, h, w, fl = c["box"]
        if h == c["S"] and w == c["S"] and not fl:
            want = np.stack([TAB[ch][c["frames"][:, i:i + h, j:j + w, ch].astype(np.int64)] for ch in range(3)])
            assert np.array_equal(ib.emulate(c["frames"], c["box"], h, w, TAB).view(np.uint32), want.view(np.uint32)), name
            assert np.array_equal(want.view(np.uint32), c["out"].view(np.uint32)), name          # and they are what the reference computed


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("defect", ib.DEFECTS)
def test_every_seeded_defect_lands_outside_the_bound(defect, bf16):
    caught = []
    for name, frames, box, S_h, S_w in _all_cases():
        ref, M = ib.statement(frames, box, S_h, S_w, TAB)
        r, _ = ib.worst(ib.emulate(frames, box, S_h, S_w, TAB, defect=defect, bf16=bf16), ref, ib.bound(ref, M, bf16))
        if r > 1.0:
            caught.append(name)
    assert caught, defect


def test_the_recorded_reference_distance_is_what_the_statement_gives():
    for name, c in FX.items():
        ref, _ = ib.statement(c["frames"], c["box"], c["S"], c["S"], TAB)
        assert float(np.abs(c["out"].astype(np.float64) - ref).max()) == c["ref_dist"], name
