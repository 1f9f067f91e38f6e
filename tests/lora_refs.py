"""fp64 restatements of the LoRA kernels (csrc/lora.hip, include/mode_hip.h "LoRA adapters") with DERIVED per-element bounds, in the style of
tests/gemm_refs.py (U = 2^-23 = two unit roundoffs of fp32, half_ulp_bf16 = the final rounding of a bf16 output).

Merge.  out = W + s acc, acc <- acc + B A over the r products from 0, every product and sum rounded on its own: r products and r sums on
quantities bounded by sum_k |B||A|, the product with s, and the last sum on |W| + |s| sum_k |B||A|:
    |got - ref| <= u (|W| + (2 r + 2) |s| sum_k |B||A|) + O(u^2)  <=  U (|W| + (r + 1) |s| sum_k |B||A|)      (+ half_ulp_bf16(ref) for a bf16 output)

Projection.  A sum of K terms (dA: K = rows, terms s B[i][k] dW[i][j]; dB: K = cols, terms s dW[i][j] A[k][j]) formed as fma chains of at most K
roundings, the adds of ceil(rows / 64) - 1 further row-block partials (dA only), one multiply by s and, with `accumulate`, one add of the previous
value - which then counts as one more term of the sum.  That is at most K + ceil(rows / 64) + 1 <= 2 K roundings of relative size u on quantities
bounded by the sum of the terms' magnitudes:
    |got - ref| <= K U sum |terms|                                        (K = number of terms, the previous value included when accumulating)
(K = 1: one fma from zero and the multiply by s are two roundings = 1 * U.)

The deliberately WRONG references (scale dropped, neighbouring experts' adapters swapped, dW transposed, last row block dropped) are what the
tests must be able to tell from the right one: tests/test_lora_references.py shows each of them outside the bound on the inputs used here."""
from __future__ import annotations

import functools

import torch

from gemm_refs import U, half_ulp_bf16

ROW_BLOCK = 64                                                                     # LG_ROWS of csrc/lora.hip
SCALE = 1.7                                                                        # not a power of two: a dropped scale changes every bit
MERGE_SHAPES = [(1, 64), (7, 64), (65, 192), (384, 128), (128, 512)]
GRAD_SHAPES = MERGE_SHAPES + [(63, 64), (64, 64), (65, 64), (129, 64)]             # + the row-block edges
RANKS = [1, 3, 16, 64]
GROUPS = [1, 3]
STRIDE_PAD = 64                                                                    # element stride between matrices = rows * cols + STRIDE_PAD


@functools.lru_cache(maxsize=None)
def inputs(G, rows, cols, r):
    """fp32 operands of one case (CPU), the same for every test: W, dW [G, rows, cols], A [G, r, cols], B [G, rows, r], previous dA / dB, a 0/1 mask."""
    g = torch.Generator().manual_seed(1000003 * G + 7919 * rows + 31 * cols + r)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float32)
    d = dict(W=rn(G, rows, cols) * 0.05, dW=rn(G, rows, cols), A=rn(G, r, cols) * r ** -0.5, B=rn(G, rows, r) * 0.1,
             dA0=rn(G, r, cols), dB0=rn(G, rows, r), mask=(torch.rand(G, rows, cols, generator=g) < 0.5).float())
    return d


def f64(t):
    return t.detach().double().cpu()


def merge_ref(W, A, B, s):
    """(ref, S): ref = W + s B A in fp64 and S = |W| + (r + 1) |s| sum_k |B||A|, both [G, rows, cols]."""
    W, A, B = f64(W), f64(A), f64(B)
    r = A.shape[1]
    return W + s * (B @ A), W.abs() + (r + 1) * abs(s) * (B.abs() @ A.abs())


def merge_bound(ref, S, out_bf16):
    return (half_ulp_bf16(ref) if out_bf16 else 0.0) + U * S


def grad_ref(dW, A, B, s, dA0=None, dB0=None):
    """((dA, dB), (bound_dA, bound_dB)) in fp64: dA = s B^T dW [G, r, cols], dB = s dW A^T [G, rows, r], added to dA0 / dB0 when given."""
    dW, A, B = f64(dW), f64(A), f64(B)
    rows, cols = dW.shape[1], dW.shape[2]
    dA, SA, KA = s * (B.transpose(1, 2) @ dW), abs(s) * (B.abs().transpose(1, 2) @ dW.abs()), rows
    dB, SB, KB = s * (dW @ A.transpose(1, 2)), abs(s) * (dW.abs() @ A.abs().transpose(1, 2)), cols
    if dA0 is not None:
        dA, SA, KA = dA + f64(dA0), SA + f64(dA0).abs(), KA + 1
        dB, SB, KB = dB + f64(dB0), SB + f64(dB0).abs(), KB + 1
    return (dA, dB), (KA * U * SA, KB * U * SB)


# ---- deliberately wrong references ----------------------------------------------------------------------------------------------------------
def swap_experts(A, B):
    """Expert g reads the adapter of expert g + 1 (cyclically)."""
    return torch.roll(A, -1, 0), torch.roll(B, -1, 0)


def transposed(dW):
    """The buffer of dW read as [cols, rows] and transposed (for rows = 1 that is the same matrix: no sensitivity case there)."""
    G, rows, cols = dW.shape
    return dW.reshape(G, cols, rows).transpose(1, 2).contiguous()


def drop_last_block(dW):
    out = dW.clone()
    rows = dW.shape[1]
    out[:, (rows - 1) // ROW_BLOCK * ROW_BLOCK:] = 0
    return out


def wrong_merges(W, A, B, s):
    out = {"scale dropped": merge_ref(W, A, B, 1.0)[0]}
    if W.shape[0] > 1:
        out["experts swapped"] = merge_ref(W, *swap_experts(A, B), s)[0]
    return out


def wrong_grads(dW, A, B, s):
    out = {"scale dropped": grad_ref(dW, A, B, 1.0)[0], "last row block dropped": grad_ref(drop_last_block(dW), A, B, s)[0]}
    if dW.shape[0] > 1:
        out["experts swapped"] = grad_ref(dW, *swap_experts(A, B), s)[0]
    if dW.shape[1] > 1:
        out["dW transposed"] = grad_ref(transposed(dW), A, B, s)[0]
    return out


def worst(got, ref, bound):
    """max over elements of |got - ref| / bound (an exactly right element counts 0 whatever its bound)."""
    err = (f64(got) - ref).abs()
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bound.clamp_min(1e-300))
    return float(ratio.max())
