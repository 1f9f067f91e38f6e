"""fp64 reference and DERIVED error bound for the device-side gradient norms (csrc/grad_norm.hip, optim.GradClip).

Reference: per-tensor sums of squares, their total, and torch.nn.utils.clip_grad_norm_'s norm / coefficient / scale, all in fp64 from the same
gradient bits the device reads.

Bound - from the kernel's accumulation structure, not from what the kernel returns.  u = 2^-24 (fp32 round-to-nearest unit).
  stage 1 (grad_sumsq_kernel), one chunk of CH = 16384 elements, 256 threads:
    every square is rounded to fp32 once                                              -> 1 rounding
    a thread adds its CH / (4 * 256) = 16 squares of one 16-byte lane into one accumulator  -> 16 additions (the first, to 0.0, is exact)
    (a0 + a1) + (a2 + a3)                                                             -> 2 additions
    64-lane butterfly                                                                 -> 6 additions
    ((w0 + w1) + w2) + w3 through LDS                                                 -> 3 additions
  A = 16 + 2 + 6 + 3 = 27 additions on the longest path from an element to its partial.  All addends are non-negative, so every rounding moves
  the running sum by a relative <= u and the partial's relative error is at most (1 + u)^(1 + A - 1) - 1 < (1 + A) u   (one of the 1 + A
  roundings is the exact 0 + x; the second-order terms are below u^2 * 28^2 / 2 and fit in that slack).
  stage 2: the partials are summed in fp64 (n_chunks * 2^-53, kept as an explicit term) and a tensor's sum is rounded to fp32 once:
    tensor_sq:  (1 + A) u + u + n_chunks 2^-53
    total (fp64, never rounded by itself):  (1 + A) u + n_chunks 2^-53
    total_norm = |grad_scale| * sqrt(total): half of the total's relative error, + u for sqrt -> fp32 and + u for the multiply / store
    coef = max_norm / (total_norm + 1e-6): the norm's error + u (add) + u (divide);  scale = grad_scale * coef: + u
  The relative bounds hold while every square is a NORMAL fp32 number (|g| in [1e-12, 1e3] in the synthetic tests - `assert_normal_squares`).
  Real model gradients may hold smaller elements: a square that lands in the subnormal range is off by at most 2^-150 absolutely (subnormal
  sums are exact), hence the absolute term n_elements * 2^-149 every bound below carries."""
import math

import torch

U = 2.0 ** -24
CH = 16384
THREADS = 256
A = CH // (4 * THREADS) + 2 + 6 + 3                      # 27
REL_PARTIAL = (1 + A) * U
assert A == 27


def n_chunks(numel, ch=CH):
    return -(-int(numel) // ch)


def bound_tensor_sq(value, numel):
    """|device tensor_sq - fp64| allowed for a tensor of `numel` elements whose fp64 sum of squares is `value`."""
    return value * (REL_PARTIAL + U + n_chunks(numel) * 2.0 ** -53) + numel * 2.0 ** -149


def rel_total(chunks):
    return REL_PARTIAL + chunks * 2.0 ** -53


def rel_norm(chunks):
    return 0.5 * rel_total(chunks) + 2 * U


def bound_norm(value, chunks, numel):
    """|device total_norm - fp64|; value = the fp64 norm (grad_scale included)."""
    return value * rel_norm(chunks) + math.sqrt(numel * 2.0 ** -149)


def bound_total(value, chunks, numel):
    """|device total_norm^2 - fp64 total| (the total itself stays in fp64 on the device; it is observable as the square of the fp32 norm)."""
    r = rel_norm(chunks)
    return value * (2 * r + r * r) + numel * 2.0 ** -149 + 2 * math.sqrt(value * numel * 2.0 ** -149)


def rel_coef(chunks):
    return rel_norm(chunks) + 2 * U


def rel_scale(chunks):
    return rel_coef(chunks) + U


def assert_normal_squares(tensors):
    """Synthetic inputs: every non-zero magnitude in [1e-12, 1e3], so that every g^2 is a normal fp32 number (exact zeros are allowed: 0 + 0)."""
    for t in tensors:
        a = t.detach().double().abs()
        nz = a[a != 0]
        if nz.numel():
            assert float(nz.min()) >= 1e-12 and float(nz.max()) <= 1e3, (float(nz.min()), float(nz.max()))
            sq = (nz.float() * nz.float())
            assert float(sq.min()) >= 2.0 ** -126 and bool(torch.isfinite(sq).all())


def ref_tensor_sq(tensors):
    """fp64 sum of squares of each tensor (python floats), from the tensors' own bits."""
    return [float((t.detach().double().cpu() ** 2).sum()) for t in tensors]


def ref_clip(tensor_sq, max_norm=None, grad_scale=1.0):
    """(total, total_norm, coef, scale) as torch.nn.utils.clip_grad_norm_ defines them for the gradient grad_scale * g, in fp64."""
    total = math.fsum(tensor_sq)
    total_norm = abs(grad_scale) * math.sqrt(total)
    coef = 1.0 if max_norm is None else min(1.0, float(max_norm) / (total_norm + 1e-6))
    return total, total_norm, coef, grad_scale * coef


def make_values(n, seed, lo_exp=-11.99, hi_exp=2.99):
    """n fp32 values with random signs and magnitudes log-uniform inside [1e-12, 1e3] (CPU)."""
    g = torch.Generator().manual_seed(seed)
    mag = 10.0 ** (torch.rand(n, generator=g, dtype=torch.float64) * (hi_exp - lo_exp) + lo_exp)
    sign = torch.where(torch.rand(n, generator=g) < 0.5, -1.0, 1.0).double()
    return (mag * sign).float()
