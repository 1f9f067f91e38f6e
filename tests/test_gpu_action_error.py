"""GPU: mode_action_error against the order-mirroring fp64 reference of tests/val_refs.py, bit for bit: the batch sizes around the lane stride of
64, every combination of absent / present mask, weight and unit, factors that count as zero (0, negatives, NaN), accumulation over calls, and the
refusals."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import hip_helpers as H  # noqa: E402
import val_refs as V  # noqa: E402
from mode_diffusion_policy_amd import _lib as L  # noqa: E402
from mode_diffusion_policy_amd import validation  # noqa: E402

BAD_ARG, UNSUPPORTED = -1, -2
CANARY = -1536.0
SHAPES = [(1, 1, 1), (3, 4, 3), (64, 10, 7), (65, 10, 7), (130, 2, 5)]            # the lane-stride edges: one lane, < 64, = 64, 64 + 1, 2 * 64 + 2


class Acc:
    """sq, ab [W * A] and cnt [W] fp64, each between canary elements."""

    def __init__(self, W, A, fill=CANARY):
        self.n = (W * A, W * A, W)
        self.bufs = [torch.full((n + 8,), CANARY, dtype=torch.float64, device="cuda") for n in self.n]
        for b in self.bufs:
            b[4:-4] = fill

    def views(self):
        return [b[4:-4] for b in self.bufs]

    def host(self):
        return [v.cpu().numpy() for v in self.views()]

    def intact(self):
        return all(bool((b[:4] == CANARY).all()) and bool((b[-4:] == CANARY).all()) for b in self.bufs)


def launch(acc, pred, target, mask=None, weight=None, unit=None, accumulate=0, over=None):
    B, W, A = pred.shape
    sq, ab, cnt = acc.views()
    d = L.ModeActionErrorDesc(pred=H.p(pred), target=H.p(target), mask=H.p(mask), weight=H.p(weight), unit=H.p(unit), sq=sq.data_ptr(), ab=ab.data_ptr(),
                              cnt=cnt.data_ptr(), B=B, W=W, A=A, accumulate=accumulate)
    for k, v in (over or {}).items():
        setattr(d, k, v)
    return L.load().mode_action_error(C.byref(d), H.stream())


def factors(B, W, A, kind, rng):
    """mask [B, W], weight [B] fp32 (or None) by kind."""
    if kind == "absent":
        return None, None
    if kind == "zero":
        return np.zeros((B, W), np.float32), np.zeros(B, np.float32)
    mask = ((rng.random((B, W)) < 0.7) * (0.25 + rng.random((B, W)))).astype(np.float32)
    weight = (0.5 + rng.random(B)).astype(np.float32)
    if kind == "dirty":                                                          # what counts as zero: 0, negatives, NaN
        mask.reshape(-1)[::3] = np.resize(np.array([-1.0, np.nan, 0.0, -np.inf], np.float32), mask.reshape(-1)[::3].shape)
        weight[::4] = np.resize(np.array([np.nan, -0.5], np.float32), weight[::4].shape)
        mask.reshape(-1)[-1], weight[-1] = 1.0, 1.0                              # one live term at least
    return mask, weight


@pytest.mark.parametrize("unit_kind", ["absent", "present"])
@pytest.mark.parametrize("B,W,A", SHAPES)
def test_sums_match_the_ordered_reference_bit_for_bit(B, W, A, unit_kind):
    rng = np.random.default_rng(100 * B + W)
    pred, target = (rng.standard_normal((B, W, A)).astype(np.float32) for _ in range(2))
    unit = None
    if unit_kind == "present":
        unit = 0.1 + 3 * rng.random(A)
        unit[A // 2] = 0.0                                                       # a constant dimension: no error from it
    dev = lambda x, dt=torch.float32: None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to("cuda", dt)
    dp, dtg, du = dev(pred), dev(target), dev(unit, torch.float64)
    for mk in ("absent", "present", "zero", "dirty"):
        for wk in ("absent", "present", "zero", "dirty"):
            mask, weight = factors(B, W, A, mk, rng)[0], factors(B, W, A, wk, rng)[1]
            acc = Acc(W, A)                                                      # accumulate = 0 overwrites the canary fill
            assert launch(acc, dp, dtg, dev(mask), dev(weight), du) == 0
            torch.cuda.synchronize()
            ref = V.action_error(pred, target, mask, weight, unit)
            assert acc.intact()
            V.same_sums(acc.host(), ref, (mk, wk))
            live = bool((V._terms(pred, target, mask, weight, None)[0] > 0).any())
            assert live == (ref[2].sum() > 0) and (live or all((r == 0).all() for r in ref)) and not (live and "zero" in (mk, wk))
            if live and (unit is None or A > 1):
                assert ref[0].sum() > 0 and ref[1].sum() > 0
            if unit is not None:
                assert (ref[0].reshape(W, A)[:, A // 2] == 0).all()


@pytest.mark.parametrize("B,W,A", [(65, 10, 7), (130, 2, 5)])
def test_accumulation_over_calls_and_dirt_under_the_mask(B, W, A):
    rng = np.random.default_rng(B)
    p1, t1, p2, t2 = (rng.standard_normal((B, W, A)).astype(np.float32) for _ in range(4))
    mask, weight = factors(B, W, A, "dirty", rng)
    unit = 0.1 + rng.random(A)
    c = V._terms(p1, t1, mask, weight, None)[0]
    assert (c == 0).sum() > B // 4
    p1d = p1.copy()
    p1d[c == 0] = np.resize(np.array([np.nan, np.inf, -np.inf, 3e38], np.float32), int((c == 0).sum()))[:, None]     # non-finite pred where c == 0
    dev = lambda x, dt=torch.float32: torch.from_numpy(np.ascontiguousarray(x)).to("cuda", dt)
    acc = Acc(W, A)
    assert launch(acc, dev(p1d), dev(t1), dev(mask), dev(weight), dev(unit, torch.float64), accumulate=0) == 0
    torch.cuda.synchronize()
    first = V.action_error(p1, t1, mask, weight, unit)
    assert all(np.isfinite(h).all() for h in acc.host())
    V.same_sums(acc.host(), first, "first call, dirty pred")
    assert launch(acc, dev(p2), dev(t2), None, dev(weight), None, accumulate=1) == 0
    torch.cuda.synchronize()
    both = V.action_error(p2, t2, None, weight, None, into=first)
    V.same_sums(acc.host(), both, "two calls")
    assert acc.intact() and (both[0] > first[0]).all()
    # the Python entry: the same launch, accumulate by default
    sq, ab, cnt = (torch.zeros(n, dtype=torch.float64, device="cuda") for n in (W * A, W * A, W))
    validation.action_error(dev(p1d), dev(t1), sq, ab, cnt, mask=dev(mask), weight=dev(weight), unit=dev(unit, torch.float64))
    validation.action_error(dev(p2), dev(t2), sq, ab, cnt, weight=dev(weight))
    V.same_sums([v.cpu().numpy() for v in (sq, ab, cnt)], both, "validation.action_error")
    res = validation.ValidationResult.from_sums(sq, ab, cnt)
    assert abs(float(res["mse"]) - both[0].sum() / (A * both[2].sum())) < 1e-12 * float(res["mse"]) and float(res["count"]) == both[2].sum()
    assert res["mse_per_step"].shape == (W,) and res["mse_per_dim"].shape == (A,) and float(res.mse_executed(1)) == float(res["mse_per_step"][0])
    for bad in (dict(mask=dev(mask)[:, :1]), dict(unit=dev(unit)), dict(weight=dev(weight).double())):
        with pytest.raises(ValueError):
            validation.action_error(dev(p2), dev(t2), sq, ab, cnt, **bad)


def test_refusals_launch_nothing():
    B, W, A = 5, 4, 3
    x = torch.randn(B, W, A, device="cuda")
    acc = Acc(W, A)
    lib = L.load()
    assert lib.mode_action_error(None, H.stream()) == BAD_ARG
    for k in ("pred", "target", "sq", "ab", "cnt"):
        assert launch(acc, x, x + 1, over={k: None}) == BAD_ARG, k
    for k in ("B", "W", "A"):
        for v in (0, -1):
            assert launch(acc, x, x + 1, over={k: v}) == BAD_ARG, (k, v)
    assert launch(acc, x, x + 1, over=dict(B=65536)) == UNSUPPORTED
    assert launch(acc, x, x + 1, over=dict(W=1366)) == UNSUPPORTED                          # 1366 * 3 = 4098 > 4096
    assert launch(acc, x, x + 1, over=dict(W=65536, A=65536)) == UNSUPPORTED                # the product, not its low 32 bits
    torch.cuda.synchronize()
    assert acc.intact() and all(bool((v == CANARY).all()) for v in acc.views())
    assert launch(acc, x, x + 1) == 0
    torch.cuda.synchronize()
    assert acc.intact() and acc.host()[2].tolist() == [float(B)] * W and np.allclose(acc.host()[0], B)
