"""CPU: the fp64 reference of the camera transform (tests/camera_refs.py) against torch's own operators in fp64 - the resize against
F.interpolate (antialiased bilinear, align_corners=False), the shift against DrQ-v2's RandomShiftsAug."""
import pytest
import torch
import torch.nn.functional as F

import camera_refs as R

LIMIT = 1e-9          # of a level; the gaps measured here are ~1e-13


def _img(h, w, seed, n=2):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 256, (n, h, w, 3), generator=g, dtype=torch.uint8)


@pytest.mark.parametrize("src,dst,modes", [((37, 29), (16, 12), (True,)), ((25, 25), (28, 28), (True, False)), ((9, 7), (16, 12), (True, False)),
                                           ((21, 84), (28, 28), (True,)), ((16, 13), (16, 13), (True, False)), ((136, 16), (17, 16), (True,))])
def test_resize_equals_interpolate_fp64(src, dst, modes):
    u = _img(*src, seed=src[0] * 100 + src[1])
    got = R.resize(u, dst)
    x = u.permute(0, 3, 1, 2).to(torch.float64)
    for aa in modes:
        ref = F.interpolate(x, size=dst, mode="bilinear", align_corners=False, antialias=aa)
        gap = float((got - ref).abs().max())
        print(f"{src} -> {dst} antialias={aa}: max gap {gap:.2e} levels")
        assert gap <= LIMIT


def test_identity_weights_are_exact():
    Wm = R.axis_weights(13, 13)
    assert torch.equal(Wm, torch.eye(13, dtype=torch.float64))
    u = _img(16, 13, 3)
    assert torch.equal(R.resize(u, (16, 13)), u.permute(0, 3, 1, 2).to(torch.float64))


def test_weight_rows_sum_to_one_and_stay_inside():
    for n_in, n_out in ((37, 16), (9, 16), (200, 224), (84, 224), (640, 224), (136, 17)):
        Wm = R.axis_weights(n_in, n_out)
        assert float((Wm.sum(1) - 1).abs().max()) < 1e-14 and float(Wm.min()) >= 0
        assert int((Wm > 0).sum(1).max()) <= 2 * max(n_in / n_out, 1) + 1


@pytest.mark.parametrize("pad,h", [(3, 16), (10, 28), (4, 9)])
def test_shift_equals_random_shifts_aug_fp64(pad, h):
    g = torch.Generator().manual_seed(pad * 10 + h)
    n = 6
    img = torch.rand(n, 3, h, h, generator=g, dtype=torch.float64) * 255
    shifts = torch.randint(0, 2 * pad + 1, (n, 2), generator=g)
    shifts[0], shifts[1], shifts[2] = torch.tensor([0, 0]), torch.tensor([2 * pad, 2 * pad]), torch.tensor([0, 2 * pad])
    ref = R.random_shifts_aug(img, pad, shifts.view(n, 1, 1, 2))
    got = R.shift(img, shifts.tolist(), pad)
    gap = float((got - ref).abs().max())
    print(f"pad {pad}, {h} x {h}: max gap {gap:.2e} levels")
    assert gap <= LIMIT
    centre = torch.full((n, 2), pad)
    assert torch.equal(R.shift(img, centre.tolist(), pad), img)                          # shift = pad is the unshifted image
    assert torch.equal(R.shift(img, [[-4, 99]] * n, pad), R.shift(img, [[0, 2 * pad]] * n, pad))   # out-of-range shifts clamp into [0, 2 pad]


def test_levels_round_half_to_even_and_clamp():
    v = torch.tensor([0.5, 1.5, 2.5, 254.5, 255.4, -0.2, 255.0], dtype=torch.float64)
    assert R.levels(v).tolist() == [0.0, 2.0, 2.0, 254.0, 255.0, 0.0, 255.0]


def test_check_output_accepts_the_reference_and_refuses_a_wrong_level():
    u = _img(37, 29, 9)
    mean, std = (0.4, 0.5, 0.6), (0.25, 0.3, 0.2)
    Rv, out = R.transform(u, (16, 12), mean, std)
    assert R.check_output(out.float(), Rv, mean, std)[0] <= 0
    assert R.check_output(out.to(torch.bfloat16), Rv, mean, std)[0] <= 0
    bad = out.clone()
    bad[1, 2, 3, 4] += 1.0 / 255.0 / std[2]                                              # one level off
    assert R.check_output(bad.float(), Rv, mean, std)[0] > 1e-3
