"""References for the candidate selection of rollout.VectorEnvPolicy(candidates=N) (tests/test_vector_env_candidates.py,
tests/test_gpu_vector_env_candidates.py): the coherence score and the selection rule of include/mode_hip.h restated in numpy fp64, and the
bound the fp32 kernel is held to."""
import numpy as np


# (W, A, shift, N) of the kernel test: the smallest; a plain one; L = 1; W no multiple of anything; W * A = 4096 and N = 64, both limits
SHAPES = [(2, 1, 1, 2), (10, 7, 4, 4), (10, 7, 9, 8), (37, 7, 5, 3), (64, 64, 1, 64)]
CASE_ENVS = 6                                                                        # environments (previous plans) per shape
RHO = 0.5


def case_rng(W, A, shift):
    return np.random.default_rng(W * 1000 + A * 10 + shift)


def weights64(rho, L):
    """rho ** w for the w-th coming step, fp64 (rollout.coherence_weights is this table rounded to fp32)."""
    return float(rho) ** np.arange(L, dtype=np.float64)


def scores64(cands, prev, shift, rho):
    """score_c = sum_{w < L} rho^w sum_a (X_c[w, a] - P[w + shift, a])^2 in fp64: cands [N, W, A], prev [W, A] -> [N]."""
    x, p = np.asarray(cands, dtype=np.float64), np.asarray(prev, dtype=np.float64)
    W = p.shape[0]
    L = W - shift
    d = x[:, :L] - p[None, shift:]
    return (weights64(rho, L)[None, :, None] * d * d).sum(axis=(1, 2))


def select(scores):
    """The rule: the smallest score, the lowest index on ties; a NaN never beats a non-NaN; all NaN -> candidate 0."""
    best = 0
    for c in range(1, len(scores)):
        if scores[c] < scores[best] or (np.isnan(scores[best]) and not np.isnan(scores[c])):
            best = c
    return best


def score_bound(L, A):
    """Relative bound on an fp32 score against scores64: every term is non-negative, so the sum's relative error is at most the add-chain
    length (at most the n = L * A terms) plus the four roundings of a term (fp32 weight, difference, square, product), each 2^-24."""
    return (L * A + 4) * 2.0 ** -24


def decisive(scores, bound):
    """True where the fp64 gap between the best and the second-best score exceeds 2 * bound relative: there an fp32 argmin must agree."""
    s = np.sort(np.asarray(scores, dtype=np.float64))
    return len(s) < 2 or s[1] - s[0] > 2.0 * bound * s[1]


def make_case(rng, n, N, W, A, shift):
    """Previous plans with entries spanning 1e-3 .. 1e3 (both signs) and, per row, N candidates = previous tail (last row held) + noise of a
    per-candidate scale 10^U(-1, 1) relative to the plan's entries.  Returns fp32 (cands [n, N, W, A], prev [n, W, A])."""
    prev = rng.uniform(-1.0, 1.0, (n, W, A)) * 10.0 ** rng.uniform(-3.0, 3.0, (n, W, A))
    idx = np.minimum(np.arange(W) + shift, W - 1)
    scale = 10.0 ** rng.uniform(-1.0, 1.0, (n, N, 1, 1))
    cands = prev[:, None, idx] + scale * rng.standard_normal((n, N, W, A))
    return cands.astype(np.float32), prev.astype(np.float32)
