"""Numpy restatement of the training batch stream and the masked EDM loss as include/mode_hip.h states them (mode_data_sample_windows,
mode_edm_loss_masked): the hashes, the draw, the binary search, the padding, the normalisation in unfused fp32, and the loss in fp64 with the
error bound that follows from the kernel's stated summation order.  Validated without a GPU by tests/test_data_references.py; the GPU tests
compare the kernels against it (integers and copies bit for bit)."""
from __future__ import annotations

import math

import numpy as np

U32 = np.uint32
GOLDEN = 0x9E3779B9


def lowbias32(x):
    """hash_u32 of csrc/mode_common.h on uint32 arrays (arithmetic modulo 2^32)."""
    x = np.asarray(x, dtype=np.uint64) & 0xFFFFFFFF
    x ^= x >> 16; x = (x * 0x7FEB352D) & 0xFFFFFFFF
    x ^= x >> 15; x = (x * 0x846CA68B) & 0xFFFFFFFF
    x ^= x >> 16
    return x.astype(np.uint64)


def stream_seed(seed: int, stream: int) -> int:
    """mode_stream_seed of csrc/mode_common.h."""
    x = (seed ^ ((GOLDEN * ((stream + 1) & 0xFFFFFFFF)) & 0xFFFFFFFF)) & 0xFFFFFFFF
    return int(lowbias32(np.array([x]))[0])


def episode_lengths(W: int):
    """The test store: episodes of length 1, W - 1, W and W + 3."""
    return [1, W - 1, W, W + 3]


def make_store(W: int, A: int, G: int, seed: int = 0, cams=None):
    """Host episodes [(actions [L, A] fp32, goal [G] fp32, static u8 | None, gripper u8 | None)] of the test store; cams = ((H, W), (Hg, Wg))."""
    rng = np.random.default_rng(seed)
    eps = []
    for L in episode_lengths(W):
        a = rng.standard_normal((L, A)).astype(np.float32) * np.float32(1.7) + np.float32(0.3)
        g = rng.standard_normal(G).astype(np.float32)
        fr = [None, None] if cams is None else [rng.integers(0, 256, (L, h, w, 3), dtype=np.uint8) for h, w in cams]
        eps.append((a, g, fr[0], fr[1]))
    return eps


def minmax(eps):
    """lo, hi, scale [A] fp32: scale = 2 / (hi - lo) in fp64 rounded to fp32, 0 where hi == lo."""
    alla = np.concatenate([e[0] for e in eps])
    lo, hi = alla.min(axis=0), alla.max(axis=0)
    span = hi.astype(np.float64) - lo.astype(np.float64)
    scale = np.where(span > 0, 2.0 / np.where(span > 0, span, 1.0), 0.0).astype(np.float32)
    return lo, hi, scale


def start_table(lengths, W: int, pad: str):
    lengths = np.asarray(lengths, dtype=np.int64)
    n_e = lengths if pad == "hold" else np.maximum(0, lengths - W + 1)
    return np.concatenate([[0], np.cumsum(n_e)]).astype(np.int64)


def draw_starts(seed: int, step: int, B: int, n_total: int):
    k = stream_seed(seed, step)
    j = np.arange(B, dtype=np.uint64)
    return ((lowbias32(k ^ j) * np.uint64(n_total)) >> np.uint64(32)).astype(np.int64)


def locate(g: int, starts) -> int:
    """The header's binary search: the largest e with starts[e] <= g."""
    lo, hi = 0, len(starts) - 1
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if starts[mid] <= g:
            lo = mid
        else:
            hi = mid
    return lo


def sample_windows(eps, W: int, B: int, seed: int, step: int, pad: str, norm=None, shift_pads=(0, 0)):
    """The batch of `step`: index, episode [B] int32; action_mask [B, W], actions [B, W, A], latent_goal [B, G] fp32; u [B] fp64;
    shifts [2][B, 2] int32 (None where shift_pads[q] == 0).  norm = (lo, scale) fp32 or None."""
    lengths = [e[0].shape[0] for e in eps]
    begin = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    acts, goals = np.concatenate([e[0] for e in eps]), np.stack([e[1] for e in eps])
    starts = start_table(lengths, W, pad)
    n_total = int(starts[-1])
    g = draw_starts(seed, step, B, n_total)
    A = acts.shape[1]
    out = dict(index=np.zeros(B, np.int32), episode=np.zeros(B, np.int32), action_mask=np.zeros((B, W), np.float32),
               actions=np.zeros((B, W, A), np.float32), latent_goal=np.zeros((B, goals.shape[1]), np.float32))
    for j in range(B):
        e = locate(int(g[j]), starts)
        idx = int(begin[e] + g[j] - starts[e])
        last = int(begin[e + 1] - 1)
        assert begin[e] <= idx <= last
        out["index"][j], out["episode"][j] = idx, e
        for w in range(W):
            x = acts[min(idx + w, last)]
            out["action_mask"][j, w] = 1.0 if idx + w <= last else 0.0
            out["actions"][j, w] = x if norm is None else (x - norm[0]) * norm[1] - np.float32(1.0)      # fp32 numpy: each operation rounded, none fused
        out["latent_goal"][j] = goals[e]
    ju = np.arange(B, dtype=np.uint64)
    k2 = stream_seed((seed + 2) & 0xFFFFFFFF, step)
    out["u"] = ((lowbias32(k2 ^ ju) >> np.uint64(8)).astype(np.float64) + 0.5) * 2.0 ** -24
    k3 = stream_seed((seed + 3) & 0xFFFFFFFF, step)
    out["shifts"] = []
    for q in range(2):
        if shift_pads[q] == 0:
            out["shifts"].append(None)
            continue
        s = np.zeros((B, 2), np.int32)
        for c in range(2):
            h = lowbias32(k3 ^ ((4 * ju + 2 * q + c) & np.uint64(0xFFFFFFFF)))
            s[:, c] = ((h * np.uint64(2 * shift_pads[q] + 1)) >> np.uint64(32)).astype(np.int32)
        out["shifts"].append(s)
    return out


def noise_seeds(seed: int, B: int):
    """s_j = (seed + 1 + j * 0x9E3779B9) mod 2^32: row j of the batch's noise is rollout.env_noise([s_j], [step], W, A, 1.0)."""
    return [(seed + 1 + j * GOLDEN) & 0xFFFFFFFF for j in range(B)]


# ---------------------------------------------------------------------------------------------------------------- masked EDM loss, fp64
U24 = 2.0 ** -24          # unit roundoff of fp32


def masked_loss(F, action, noise, sigma, sigma_data, mask=None, weight=None):
    """fp64 from the fp32 inputs -> dict(loss, dF [B, W, A], per_sample [B]) and the kernel's error bounds b_loss, b_dF, b_per_sample.

    Values: m = mask > 0 ? mask : 0, wt likewise, c = wt m, den = A sum c; loss = sum c d^2 / den (0 when den == 0), dF = 2 c d / den (+0 where
    c == 0, whatever d), per_sample[b] = sum_w m sum_a d^2 / (A sum_w m) (0 without a real step).  An element with m == 0 is skipped, so d there may
    be non-finite.

    Bounds (u = 2^-24; first order, times 1.01 for the second-order terms), from the operations include/mode_hip.h states:
    * the residual d = F - (a - c_skip (a + n s)) / c_out in fp32, divisions and the square root taken as 2 ulp: s2 = s s + sd sd carries 2u,
      c_skip = sd sd / s2 5u, c_out = s sd / sqrt(s2) 5u, noised = a + n s an absolute 2u M with M = |a| + |n s|, so c_skip noised an absolute
      8u c_skip M, the numerator u |a| + 9u c_skip M, the quotient (u |a| + 9u c_skip M) / c_out + 7u |target|, and the difference adds u |d|:
          E = u ((|a| + 9 c_skip M) / c_out + 7 |target| + |d|)                       (a contracted multiply-add only removes a rounding)
    * den: M_b is a lane's ceil(W / 64) - 1 additions and the 6 of the butterfly, one product with wt, ceil(B / 16) additions in the wave, 16
      across the waves, one product with A: every term is >= 0, so the relative error is n_c u, n_c = ceil(W / 64) + ceil(B / 16) + 24
    * dF = ((2 c) / den) d: the coefficient carries n_c u + 1 (c) + 2 (division), the product one more: |coef| E + (n_c + 4) u |dF|
    * S_b = sum m d^2 (terms >= 0): d d rounded, one fma per element in the lane (ceil(W A / 64) of them), 6 in the butterfly:
          e_S = sum m (2 |d| E + E^2) + (ceil(W A / 64) + 7) u S_b
    * per_sample = S_b / (A M_b): e_S / (A M_b) + (ceil(W / 64) + 6 + 1 + 2) u per_sample
    * loss = (sum wt S_b) / den: one fma per sample in the wave (ceil(B / 16)), 16 across the waves, the division 2:
          (sum wt e_S) / den + (ceil(B / 16) + 16 + n_c + 2) u loss"""
    F, a, n = (np.asarray(t, dtype=np.float64) for t in (F, action, noise))
    B, W, A = a.shape
    s = np.asarray(sigma, dtype=np.float64).reshape(B, 1, 1)
    sd = float(sigma_data)
    m = np.ones((B, W)) if mask is None else np.where(np.asarray(mask, np.float64) > 0, np.asarray(mask, np.float64), 0.0)
    wt = np.ones(B) if weight is None else np.where(np.asarray(weight, np.float64) > 0, np.asarray(weight, np.float64), 0.0)
    c = wt[:, None] * m
    s2 = s * s + sd * sd
    c_skip, c_out = sd * sd / s2, s * sd / np.sqrt(s2)
    noised = a + n * s
    target = (a - c_skip * noised) / c_out
    live = np.broadcast_to((m > 0)[:, :, None], a.shape)
    with np.errstate(invalid="ignore"):
        d = np.where(live, F - target, 0.0)
    E = np.where(live, U24 * ((np.abs(a) + 9 * c_skip * (np.abs(a) + np.abs(n * s))) / c_out + 7 * np.abs(target) + np.abs(d)), 0.0)
    Mb = m.sum(axis=1)
    den = A * c.sum()
    Sb = (m[:, :, None] * d * d).sum(axis=(1, 2))
    per = np.where(Mb > 0, Sb / np.where(Mb > 0, A * Mb, 1.0), 0.0)
    loss = float((wt * Sb).sum() / den) if den > 0 else 0.0
    coef = 2 * c / den if den > 0 else np.zeros_like(c)
    dF = coef[:, :, None] * d
    n_c = math.ceil(W / 64) + math.ceil(B / 16) + 24
    k = 1.01
    b_dF = k * (coef[:, :, None] * E + (n_c + 4) * U24 * np.abs(dF))
    e_S = (m[:, :, None] * (2 * np.abs(d) * E + E * E)).sum(axis=(1, 2)) + (math.ceil(W * A / 64) + 7) * U24 * Sb
    b_per = k * np.where(Mb > 0, e_S / np.where(Mb > 0, A * Mb, 1.0) + (math.ceil(W / 64) + 9) * U24 * per, 0.0)
    b_loss = k * ((wt * e_S).sum() / den + (math.ceil(B / 16) + 18 + n_c) * U24 * loss) if den > 0 else 0.0
    return dict(loss=loss, dF=dF, per_sample=per, b_loss=float(b_loss), b_dF=b_dF, b_per_sample=b_per)


def same_bits(a, b) -> bool:
    """Two arrays of one shape and dtype with the same bytes: NaN payloads and the sign of zero count."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()
