"""GPU: mode_level_error and mode_val_noise_levels through the C ABI, into guarded outputs, bit for bit against the numpy replay of
tests/level_refs.py; every level's slice against mode_action_error run on the same device with the level folded into the weight; the batch sizes
around the lane stride of 64; empty levels, masked rows, non-finite predictions where nothing counts, levels out of range, accumulation over calls,
and the refusals.

Levels are dealt round-robin (a permutation of b mod K), and the first row of every level is made live, so each of the min(B, K) levels a batch of B
rows can reach has a live row; with B < K the remaining levels are empty by necessity.  That is asserted on the host before every launch."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import hip_helpers as H  # noqa: E402
import level_refs as LR  # noqa: E402
import val_refs as V  # noqa: E402
from mode_diffusion_policy_amd import _lib as L  # noqa: E402
from mode_diffusion_policy_amd import validation  # noqa: E402

BAD_ARG, UNSUPPORTED = -1, -2
BATCHES = [1, 3, 64, 65, 130]                                                    # one lane, < 64, = 64, 64 + 1 (the lane wrap), three terms per lane
GEOMS = [(4, 3), (10, 7)]
LEVELS = [1, 3, 16]


def dev(x, dt=torch.float32):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to("cuda", dt)


class Out:
    """sq [K, W * A] and cnt [K, W] fp64, NaN-prefilled between canary rows."""

    def __init__(self, K, W, A):
        self.sq, self.cnt = H.Guarded(K, W * A, torch.float64), H.Guarded(K, W, torch.float64)

    def host(self):
        return self.sq.t.cpu().numpy(), self.cnt.t.cpu().numpy()

    def intact(self):
        return self.sq.intact() and self.cnt.intact()

    def untouched(self):
        return self.intact() and bool(torch.isnan(self.sq.t).all()) and bool(torch.isnan(self.cnt.t).all())


def launch(out, pred, target, level, K, mask=None, weight=None, accumulate=0, over=None):
    B, W, A = pred.shape
    d = L.ModeLevelErrorDesc(pred=H.p(pred), target=H.p(target), mask=H.p(mask), weight=H.p(weight), level=H.p(level), sq=out.sq.t.data_ptr(),
                             cnt=out.cnt.t.data_ptr(), B=B, W=W, A=A, K=K, accumulate=accumulate)
    for k, v in (over or {}).items():
        setattr(d, k, v)
    return L.load().mode_level_error(C.byref(d), H.stream())


def action_error_slices(pred, target, level, K, mask, weight):
    """mode_action_error on the device, once per level, with weight'[b] = level[b] == k ? weight[b] : 0 and unit = NULL -> (sq [K, W * A], cnt [K, W])."""
    B, W, A = pred.shape
    sq, ab = (torch.full((K, W * A), float("nan"), dtype=torch.float64, device="cuda") for _ in range(2))
    cnt = torch.full((K, W), float("nan"), dtype=torch.float64, device="cuda")
    lv, wt = level.cpu().numpy(), None if weight is None else weight.cpu().numpy()
    for k in range(K):
        validation.action_error(pred, target, sq[k], ab[k], cnt[k], mask=mask, weight=dev(LR.folded_weight(lv, k, wt)), accumulate=False)
    return sq.cpu().numpy(), cnt.cpu().numpy()


def inputs(B, W, A, K, seed):
    """pred, target, mask, weight, level with every reachable level live: round-robin levels, the first row of each level fully unmasked."""
    rng = np.random.default_rng(seed)
    pred, target = (rng.standard_normal((B, W, A)).astype(np.float32) for _ in range(2))
    mask = ((rng.random((B, W)) < 0.7) * (0.25 + rng.random((B, W)))).astype(np.float32)
    weight = (0.5 + rng.random(B)).astype(np.float32)
    weight[3::5] = 0.0                                                           # some whole rows count nothing
    level = (rng.permutation(B) % K).astype(np.int32)
    for k in range(K):
        rows = np.nonzero(level == k)[0]
        if len(rows):
            mask[rows[0]], weight[rows[0]] = 0.5 + rng.random(W).astype(np.float32), 1.25
    return pred, target, mask, weight, level


def live_levels(level, K, mask, weight, B, W):
    c = V._terms(np.zeros((B, W, 1), np.float32), np.zeros((B, W, 1), np.float32), mask, weight, None)[0]
    return {int(k) for k, row in zip(level, c) if 0 <= k < K and (row > 0).any()}


@pytest.mark.parametrize("K", LEVELS)
@pytest.mark.parametrize("W,A", GEOMS)
@pytest.mark.parametrize("B", BATCHES)
def test_sums_match_the_replay_and_the_action_error_bit_for_bit(B, W, A, K):
    pred, target, mask, weight, level = inputs(B, W, A, K, 1000 * B + 10 * W + K)
    dp, dtg, dl = dev(pred), dev(target), dev(level, torch.int32)
    for kind, m, wt in (("mask only", mask, None), ("weight only", None, weight), ("both", mask, weight)):
        assert live_levels(level, K, m, wt, B, W) == set(range(min(B, K)))
        out = Out(K, W, A)
        assert launch(out, dp, dtg, dl, K, dev(m), dev(wt)) == 0
        torch.cuda.synchronize()
        ref = LR.level_error(pred, target, level, K, m, wt)
        assert out.intact()
        V.same_sums(out.host(), ref, kind)
        V.same_sums(out.host(), action_error_slices(dp, dtg, dl, K, dev(m), dev(wt)), kind + ": mode_action_error per level")
        for k in range(K):
            if k < min(B, K):
                assert ref[1][k].sum() > 0 and ref[0][k].sum() > 0
            else:                                                                # B < K: a level no row can reach is exactly +0.0
                assert not out.host()[0][k].view(np.uint64).any() and not out.host()[1][k].view(np.uint64).any()


@pytest.mark.parametrize("K", LEVELS)
@pytest.mark.parametrize("B,W,A", [(3, 4, 3), (65, 10, 7), (130, 4, 3), (130, 10, 7)])
def test_empty_levels_masked_rows_and_levels_out_of_range(B, W, A, K):
    pred, target, mask, weight, level = inputs(B, W, A, K, 77 * B + K)
    dtg = dev(target)
    # one level without any row: its rows go to the next level (K = 1: out of range, nothing counts anywhere)
    gone = K // 2
    lv = np.where(level == gone, (gone + 1) % K if K > 1 else K, level).astype(np.int32)
    assert live_levels(lv, K, mask, weight, B, W) == set(range(min(B, K))) - {gone}
    out = Out(K, W, A)
    assert launch(out, dev(pred), dtg, dev(lv, torch.int32), K, dev(mask), dev(weight)) == 0
    torch.cuda.synchronize()
    got = out.host()
    V.same_sums(got, LR.level_error(pred, target, lv, K, mask, weight), "a level without rows")
    assert out.intact() and not got[0][gone].view(np.uint64).any() and not got[1][gone].view(np.uint64).any()       # +0.0, not -0.0 or NaN
    # every row masked: every sum is +0.0
    out = Out(K, W, A)
    assert launch(out, dev(pred), dtg, dev(level, torch.int32), K, dev(np.zeros((B, W), np.float32)), dev(weight)) == 0
    torch.cuda.synchronize()
    assert out.intact() and all(not h.view(np.uint64).any() for h in out.host())
    # levels -1 and K (and the int32 extremes) count nowhere; NaN / Inf in pred under a zero c and in the rows out of range change nothing
    lv = level.copy()
    lv[::4] = np.resize(np.array([-1, K, -2 ** 31, 2 ** 31 - 1], np.int32), lv[::4].shape)
    inside = (lv >= 0) & (lv < K)
    c = V._terms(pred, target, mask, weight, None)[0]
    dead = (c == 0) | ~inside[:, None]
    dirty = pred.copy()
    dirty[dead] = np.resize(np.array([np.nan, np.inf, -np.inf, 3e38], np.float32), int(dead.sum()))[:, None]
    assert (~inside).any() and ((c == 0).any() or B == 3) and not np.isfinite(dirty).all()      # (B = 3: every row is some level's live row)
    out = Out(K, W, A)
    assert launch(out, dev(dirty), dtg, dev(lv, torch.int32), K, dev(mask), dev(weight)) == 0
    torch.cuda.synchronize()
    got = out.host()
    clean = LR.level_error(pred, target, np.where(inside, lv, 0), K, mask, weight * inside)      # the rows out of range weighted 0 instead
    assert out.intact() and all(np.isfinite(h).all() for h in got)
    V.same_sums(got, LR.level_error(dirty, target, lv, K, mask, weight), "dirty pred, levels out of range")
    V.same_sums(got, clean, "out of range = weight 0")
    V.same_sums(got, action_error_slices(dev(dirty), dtg, dev(lv, torch.int32), K, dev(mask), dev(weight)), "mode_action_error per level")


@pytest.mark.parametrize("K", LEVELS)
@pytest.mark.parametrize("B,W,A", [(65, 10, 7), (130, 4, 3)])
def test_two_calls_accumulate(B, W, A, K):
    p1, t1, mask, weight, l1 = inputs(B, W, A, K, B + K)
    p2, t2, _, _, l2 = inputs(B, W, A, K, B + K + 1)
    out = Out(K, W, A)
    assert launch(out, dev(p1), dev(t1), dev(l1, torch.int32), K, dev(mask), dev(weight), accumulate=0) == 0      # overwrites the NaN fill
    assert launch(out, dev(p2), dev(t2), dev(l2, torch.int32), K, None, dev(weight), accumulate=1) == 0
    torch.cuda.synchronize()
    first = LR.level_error(p1, t1, l1, K, mask, weight)
    both = LR.level_error(p2, t2, l2, K, None, weight, into=first)
    V.same_sums(out.host(), both, "two calls")
    assert out.intact() and (both[1] >= first[1]).all() and (both[1] > first[1]).any()
    # the Python entry: the same launches, accumulate by default
    sq, cnt = torch.zeros(K, W * A, dtype=torch.float64, device="cuda"), torch.zeros(K, W, dtype=torch.float64, device="cuda")
    validation.level_error(dev(p1), dev(t1), dev(l1, torch.int32), sq, cnt, mask=dev(mask), weight=dev(weight))
    validation.level_error(dev(p2), dev(t2), dev(l2, torch.int32), sq, cnt, weight=dev(weight))
    V.same_sums((sq.cpu().numpy(), cnt.cpu().numpy()), both, "validation.level_error")
    for bad in (dict(mask=dev(mask)[:, :1]), dict(weight=dev(weight).double()), dict(level=dev(l2, torch.int64))):
        kw = {**dict(level=dev(l2, torch.int32)), **bad}
        with pytest.raises(ValueError):
            validation.level_error(dev(p2), dev(t2), kw.pop("level"), sq, cnt, **kw)
    with pytest.raises(ValueError):
        validation.level_error(dev(p2), dev(t2), dev(l2, torch.int32), sq.reshape(-1), cnt)


def test_level_error_refusals_launch_nothing():
    B, W, A, K = 5, 4, 3, 3
    x = torch.randn(B, W, A, device="cuda")
    lv = torch.arange(B, dtype=torch.int32, device="cuda") % K
    out = Out(K, W, A)
    assert L.load().mode_level_error(None, H.stream()) == BAD_ARG
    for k in ("pred", "target", "level", "sq", "cnt"):
        assert launch(out, x, x + 1, lv, K, over={k: None}) == BAD_ARG, k
    for k in ("B", "W", "A", "K"):
        for v in (0, -1):
            assert launch(out, x, x + 1, lv, K, over={k: v}) == BAD_ARG, (k, v)
    assert launch(out, x, x + 1, lv, K, over=dict(K=257)) == UNSUPPORTED
    assert launch(out, x, x + 1, lv, K, over=dict(B=65536)) == UNSUPPORTED
    assert launch(out, x, x + 1, lv, K, over=dict(W=1366)) == UNSUPPORTED                   # 1366 * 3 = 4098 > 4096
    assert launch(out, x, x + 1, lv, K, over=dict(W=65536, A=65536)) == UNSUPPORTED         # the product, not its low 32 bits
    torch.cuda.synchronize()
    assert out.untouched()
    assert launch(out, x, x + 1, lv, K) == 0
    torch.cuda.synchronize()
    sq, cnt = out.host()
    assert out.intact() and cnt.tolist() == [[2.0] * W, [2.0] * W, [1.0] * W] and np.allclose(sq, cnt[:, :1])


# ------------------------------------------------------------------------------------------------------------ mode_val_noise_levels
class Prep:
    """level [B] int32, sigma [B] fp32, x [B, W * A] fp32 in guarded buffers."""

    def __init__(self, B, WA):
        self.level, self.sigma, self.x = H.Guarded(1, B, torch.int32, fill=-7), H.Guarded(1, B), H.Guarded(B, WA)

    def host(self):
        return self.level.t.cpu().numpy().reshape(-1), self.sigma.t.cpu().numpy().reshape(-1), self.x.t.cpu().numpy()

    def intact(self):
        return self.level.intact() and self.sigma.intact() and self.x.intact()

    def untouched(self):
        return self.intact() and bool((self.level.t == -7).all()) and bool(torch.isnan(self.sigma.t).all()) and bool(torch.isnan(self.x.t).all())


def prep(out, actions, noise, window, sigmas, draw, over=None):
    B, W, A = actions.shape
    d = L.ModeValLevelsDesc(actions=H.p(actions), noise=H.p(noise), window=H.p(window), sigmas=H.p(sigmas), B=B, W=W, A=A, K=sigmas.shape[0], draw=draw,
                            level=out.level.t.data_ptr(), sigma=out.sigma.t.data_ptr(), x=out.x.t.data_ptr())
    for k, v in (over or {}).items():
        setattr(d, k, v)
    return L.load().mode_val_noise_levels(C.byref(d), H.stream())


def prep_inputs(B, W, A, K, seed):
    rng = np.random.default_rng(seed)
    actions, noise = (rng.standard_normal((B, W, A)).astype(np.float32) for _ in range(2))
    window = rng.integers(0, 700, B).astype(np.int32)
    if B > 2:
        window[-2:] = window[-3]                                                 # padding rows repeat the last window, data and all
        actions[-2:], noise[-2:] = actions[-3], noise[-3]
    sigmas = np.exp(rng.uniform(np.log(1e-3), np.log(80.0), K)).astype(np.float32)
    return actions, noise, window, sigmas


@pytest.mark.parametrize("K", LEVELS)
@pytest.mark.parametrize("W,A", GEOMS)
@pytest.mark.parametrize("B", [1, 3, 130])
def test_noise_levels_match_the_fp32_replay_bit_for_bit(B, W, A, K):
    actions, noise, window, sigmas = prep_inputs(B, W, A, K, 31 * B + K + W)
    for draw in (0, 5, 2 ** 32 - 3):                                             # the last: window + draw wraps past 2^32 for every window >= 3
        out = Prep(B, W * A)
        assert prep(out, dev(actions), dev(noise), dev(window, torch.int32), dev(sigmas), draw) == 0
        torch.cuda.synchronize()
        level, sigma, x = out.host()
        rl, rs, rx = LR.noise_levels(actions, noise, window, sigmas, draw)
        assert out.intact() and np.array_equal(level, rl) and np.array_equal(sigma.view(np.uint32), rs.view(np.uint32))
        assert np.array_equal(x.view(np.uint32), rx.reshape(B, W * A).view(np.uint32)), draw
        assert (window.astype(np.int64) + draw >= 2 ** 32).any() == (draw > 2 ** 31) or B == 1
        if B > 2:                                                                # padding rows: a level like any other row's, the repeated window's
            assert level[-1] == level[-2] == level[-3] and np.array_equal(x[-1], x[-3])
    # the Python entry
    lv, sg, xn = validation.noise_levels(dev(actions), dev(noise), dev(window, torch.int32), dev(sigmas), 5)
    rl, rs, rx = LR.noise_levels(actions, noise, window, sigmas, 5)
    assert lv.dtype == torch.int32 and np.array_equal(lv.cpu().numpy(), rl) and np.array_equal(sg.cpu().numpy(), rs) and np.array_equal(xn.cpu().numpy(), rx)


def test_a_rows_outputs_do_not_depend_on_its_place_or_the_batch_size():
    B, W, A, K = 130, 10, 7, 16
    actions, noise, window, sigmas = prep_inputs(B, W, A, K, 9)
    full = Prep(B, W * A)
    assert prep(full, dev(actions), dev(noise), dev(window, torch.int32), dev(sigmas), 11) == 0
    level, sigma, x = full.host()
    for rows in ([129], [64, 0, 77], list(range(40, 105))):                      # other places, other batch sizes
        sub = Prep(len(rows), W * A)
        assert prep(sub, dev(actions[rows]), dev(noise[rows]), dev(window[rows], torch.int32), dev(sigmas), 11) == 0
        torch.cuda.synchronize()
        l2, s2, x2 = sub.host()
        assert sub.intact() and np.array_equal(l2, level[rows]) and np.array_equal(s2.view(np.uint32), sigma[rows].view(np.uint32))
        assert np.array_equal(x2.view(np.uint32), x[rows].view(np.uint32))


def test_noise_levels_refusals_launch_nothing():
    B, W, A, K = 5, 4, 3, 3
    a, z = torch.randn(B, W, A, device="cuda"), torch.randn(B, W, A, device="cuda")
    win = torch.arange(B, dtype=torch.int32, device="cuda")
    sig = torch.tensor([0.1, 1.0, 10.0], device="cuda")
    out = Prep(B, W * A)
    assert L.load().mode_val_noise_levels(None, H.stream()) == BAD_ARG
    for k in ("actions", "noise", "window", "sigmas", "level", "sigma", "x"):
        assert prep(out, a, z, win, sig, 0, over={k: None}) == BAD_ARG, k
    for k in ("B", "W", "A", "K"):
        for v in (0, -1):
            assert prep(out, a, z, win, sig, 0, over={k: v}) == BAD_ARG, (k, v)
    assert prep(out, a, z, win, sig, 0, over=dict(K=257)) == UNSUPPORTED
    assert prep(out, a, z, win, sig, 0, over=dict(B=65536)) == UNSUPPORTED
    assert prep(out, a, z, win, sig, 0, over=dict(W=1366)) == UNSUPPORTED
    assert prep(out, a, z, win, sig, 0, over=dict(W=65536, A=65536)) == UNSUPPORTED
    torch.cuda.synchronize()
    assert out.untouched()
    assert prep(out, a, z, win, sig, 1) == 0
    torch.cuda.synchronize()
    level, sigma, x = out.host()
    assert out.intact() and level.tolist() == [1, 2, 0, 1, 2] and sigma.tolist() == [1.0, 10.0, pytest.approx(0.1), 1.0, 10.0]
    for bad in (dict(draw=-1), dict(draw=2 ** 32), dict(draw=1.0)):
        with pytest.raises(ValueError):
            validation.noise_levels(a, z, win, sig, **bad)
    with pytest.raises(ValueError):
        validation.noise_levels(a, z, win, torch.ones(257, device="cuda"))
    with pytest.raises(ValueError):
        validation.noise_levels(a, z, win.long(), sig)
