"""Numpy restatement of the two kernels behind validation.LevelValidator as include/mode_hip.h states them (mode_val_noise_levels,
mode_level_error): a window's level and noised input in unfused fp32, and the masked squared error per level in fp64 in the kernel's stated order -
lane by lane over the rows of one level, then the xor butterfly - built on the terms and the butterfly of tests/val_refs.py, so that the GPU tests can
compare bit for bit.  Validated without a GPU by tests/test_level_references.py.

The bound on an ordered sum.  Every term t = c * (e * e) (or c) is >= 0 and is the same fp64 number in any order of summation, so only the additions
differ.  Lane l adds at most ceil(B / 64) terms, the first of them to 0.0 (exact), and its sum then passes through the 6 additions of the butterfly:
no term goes through more than R(B) = ceil(B / 64) + 6 rounded additions (one of them spare), each with a relative error of at most u = 2^-53 of a
partial sum that is no larger than the total.  Hence |ordered - exact| <= gamma(R) * exact with gamma(n) = n u / (1 - n u).  An accumulator that was
added to over `calls` launches passes through calls - 1 further additions (the first lands on 0.0), each rounding a running total <= the total:
R(B, calls) = ceil(B / 64) + 6 + calls - 1.  `sum_bound` returns gamma(R); two ordered sums of the same terms differ by at most the sum of their
bounds."""
from __future__ import annotations

import numpy as np

import val_refs as V

U = 2.0 ** -53


def roundings(B: int, calls: int = 1) -> int:
    return -(-B // 64) + 6 + (calls - 1)


def sum_bound(B: int, calls: int = 1) -> float:
    """gamma(R(B, calls)): the relative error of an ordered (and accumulated) sum of non-negative terms against their exact sum."""
    n = roundings(B, calls)
    return n * U / (1 - n * U)


def levels_of(window, draw: int, K: int):
    """level [B] int32 = ((uint32) window + draw) mod 2^32 mod K."""
    g = np.asarray(window).astype(np.int64) & 0xFFFFFFFF
    return (((g + int(draw)) & 0xFFFFFFFF) % K).astype(np.int32)


def noise_levels(actions, noise, window, sigmas, draw: int):
    """(level [B] int32, sigma [B] fp32, x [B, W, A] fp32): x = actions + noise * sigma in numpy fp32 - the product rounded, then the sum."""
    actions, noise, sigmas = np.asarray(actions, np.float32), np.asarray(noise, np.float32), np.asarray(sigmas, np.float32)
    level = levels_of(window, draw, sigmas.shape[0])
    sigma = sigmas[level]
    with np.errstate(all="ignore"):
        t = (noise * sigma[:, None, None]).astype(np.float32)
        x = (actions + t).astype(np.float32)
    return level, sigma, x


def level_error(pred, target, level, K: int, mask=None, weight=None, into=None):
    """(sq [K, W * A], cnt [K, W]) fp64 in the kernel's order: the wave of (k, i) has lane l add the terms of the rows b = l, l + 64, ... ascending with
    level[b] == k and c > 0, and the 64 lane sums go through the butterfly.  A level outside [0, K) counts nowhere.  `into` = (sq, cnt) of earlier
    calls, to which the sums are added (accumulate = 1)."""
    c, e = V._terms(pred, target, mask, weight, None)
    B, W, A = e.shape
    level = np.asarray(level, np.int32)
    sq, cn = np.zeros((64, K, W, A)), np.zeros((64, K, W))
    with np.errstate(all="ignore"):
        for b in range(B):
            k = int(level[b])
            if not 0 <= k < K:
                continue
            l, cb = b % 64, c[b]
            live = cb > 0
            t2 = cb[:, None] * (e[b] * e[b])
            sq[l, k] = np.where(live[:, None], sq[l, k] + t2, sq[l, k])
            cn[l, k] = np.where(live, cn[l, k] + cb, cn[l, k])
        out = (V._butterfly(sq).reshape(K, W * A), V._butterfly(cn))
        if into is not None:
            out = tuple(o + s for o, s in zip(into, out))
    return out


def level_error_plain(pred, target, level, K: int, mask=None, weight=None):
    """The same sums by numpy's own summation, terms with c == 0 and rows of other levels dropped.  The fp64 terms are summed in np.longdouble
    (64 mantissa bits on x86: the B additions cost < B * 2^-64 relative, inside the spare rounding of `sum_bound`) and returned unrounded, so the
    reference's own error does not eat the bound."""
    c, e = V._terms(pred, target, mask, weight, None)
    B, W, A = e.shape
    level = np.asarray(level, np.int32)
    sq, cn = np.zeros((K, W, A), np.longdouble), np.zeros((K, W), np.longdouble)
    with np.errstate(all="ignore"):
        for k in range(K):
            rows = (level == k)[:, None] & (c > 0)
            t2 = np.where(rows[:, :, None], c[:, :, None] * (e * e), 0.0)
            sq[k] = t2.astype(np.longdouble).sum(axis=0)
            cn[k] = np.where(rows, c, 0.0).astype(np.longdouble).sum(axis=0)
    return sq.reshape(K, W * A), cn


def folded_weight(level, k: int, weight=None):
    """weight'[b] = level[b] == k ? weight[b] : 0 (an absent weight is 1): what turns mode_action_error into level k's slice."""
    level = np.asarray(level, np.int32)
    w = np.ones(level.shape[0], np.float32) if weight is None else np.asarray(weight, np.float32)
    return np.where(level == k, w, np.float32(0.0)).astype(np.float32)
