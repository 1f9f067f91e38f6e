"""References for the forward contrast of rollout.VectorEnvPolicy(candidates=N, contrast=M) (tests/test_vector_env_contrast.py,
tests/test_gpu_vector_env_contrast.py): the selection rule of include/mode_hip.h restated in numpy fp64 on top of tests/cand_refs.py, the bounds
the fp32 kernel is held to, and the seeded case table both test files share (built once per shape, never modified)."""
import functools

import numpy as np

import cand_refs as R

# (W, A, shift, N, M, K): the smallest; a plain one with K < N, M; L = 1 and K = N = M ("all"); W no multiple of anything, N != M; W * A = 4096
# with N + M = 64, both limits
CASES = [(2, 1, 1, 2, 1, 1), (10, 7, 4, 4, 4, 2), (10, 7, 9, 8, 8, 8), (37, 7, 5, 3, 5, 2), (64, 64, 1, 32, 32, 4)]
CASE_ENVS = 6                                                                        # environments (previous plans) per shape
LAMBDAS = (1.0, 0.25)                                                                # (both exact in fp32)
RHO = R.RHO
WEAK_SCALE = 3.0                                                                     # weak candidates: three times the strong ones' noise scale
DECISIVE_SHARE = 0.90                                                                # of the table's rows; a condition on the table, not a measurement
U = 2.0 ** -24


def ranked(bc, k):
    """The indices of the k smallest entries in rank order: the lower index wins ties, a NaN ranks after every non-NaN (NaNs by index)."""
    return np.argsort(np.asarray(bc, dtype=np.float64), kind="stable")[:k]           # (a stable sort puts NaN last and keeps index order)


def dist64(x, y):
    """d(x, y) = sum_w sum_a (x[w, a] - y[w, a])^2 over the whole chunk, fp64."""
    d = np.asarray(x, dtype=np.float64) - np.asarray(y, dtype=np.float64)
    return float((d * d).sum())


def reference(cands, prev, has_prev, shift, rho, N, K, lam):
    """The rule in fp64 for one row: cands [N + M, W, A] (strong first), prev [W, A].  Returns a dict: bc [N + M], sp / sn (S+ / S- in rank
    order, indices into cands), pos / neg [N] (the sums of distances to S+ / S-), fc [N], total [N], selected."""
    x = np.asarray(cands, dtype=np.float64)
    NT = x.shape[0]
    M = NT - N
    Ks, Kw = min(K, N), min(K, M)
    bc = R.scores64(x, prev, shift, rho) if has_prev else np.zeros(NT)
    sp, sn = ranked(bc[:N], Ks), N + ranked(bc[N:], Kw)
    pos = np.array([sum(dist64(x[c], x[p]) for p in sp) for c in range(N)])
    neg = np.array([sum(dist64(x[c], x[q]) for q in sn) for c in range(N)])
    fc = pos / Ks - neg / Kw
    total = bc[:N] + lam * fc
    return dict(bc=bc, sp=sp, sn=sn, pos=pos, neg=neg, fc=fc, total=total, selected=R.select(total), Ks=Ks, Kw=Kw)


def _gamma(n):
    return n * U / (1.0 - n * U)


def fc_bound(ref, W, A):
    """Absolute bound on the fp32 fc against the fp64 one, per strong candidate, given the same sets.  fc is a difference, so the bound is
    relative to pos / Ks + neg / Kw.  A distance's element passes through at most ceil(W A / 64) fused multiply-adds of its lane and 6 shuffle
    adds, and carries the rounding of the difference twice (it is squared; the square itself is not rounded inside the fma); the sum over the
    set adds max(Ks, Kw) additions, the division one rounding, the subtraction one more: each 2^-24."""
    n = -(-W * A // 64) + 6 + 2 + max(ref["Ks"], ref["Kw"]) + 2
    return _gamma(n) * (ref["pos"] / ref["Ks"] + ref["neg"] / ref["Kw"])


def total_bound(ref, W, A, shift, lam):
    """Absolute bound on the fp32 total = fma(lambda, fc, bc), per strong candidate: total can be negative, so the bound is relative to the sum
    of magnitudes bc + lambda (pos / Ks + neg / Kw).  The longest chain is fc's (above; bc's own, ceil(L A / 64) + 6 adds + the 4 roundings of
    a term, is never longer) plus the one rounding of the final fma; lambda is exact in fp32 in every case of the table."""
    n = -(-W * A // 64) + 6 + 2 + max(ref["Ks"], ref["Kw"]) + 3
    assert n >= -(-(W - shift) * A // 64) + 6 + 4 + 1
    N = len(ref["total"])
    return _gamma(n) * (ref["bc"][:N] + lam * (ref["pos"] / ref["Ks"] + ref["neg"] / ref["Kw"]))


def decisive(ref, bound_total, bc_rel, N, K, has_prev):
    """True when the fp32 kernel must select the fp64 argmin: (1) where a top-K set is a proper subset (K < N, K < M) and a previous plan
    exists, the fp64 gap in bc across the set's boundary exceeds twice the bc bound, so fp32 forms the same set (with no previous plan the
    sets go by index); (2) the gap between the best total and every other one - the second best in particular - exceeds the sum of the two
    bounds."""
    bc = ref["bc"]
    if has_prev:
        for part, k in ((bc[:N], ref["Ks"]), (bc[N:], ref["Kw"])):
            if k < len(part):
                s = np.sort(part)
                if not s[k] - s[k - 1] > 2.0 * bc_rel * s[k]:
                    return False
    t, b = ref["total"], bound_total
    i = ref["selected"]
    return all(t[c] - t[i] > b[c] + b[i] for c in range(len(t)) if c != i)


def case_rng(W, A, shift, N, M):
    return np.random.default_rng(W * 100000 + A * 1000 + shift * 100 + N + M)


def make_case(rng, n, N, M, W, A, shift):
    """cand_refs.make_case with N strong + M weak candidates per row: previous plans with entries spanning 1e-3 .. 1e3 (both signs), candidates =
    previous tail (last row held) + noise of a per-candidate scale 10^U(-1, 1), the weak ones' scale three times that.  Returns fp32
    (cands [n, N + M, W, A], prev [n, W, A])."""
    prev = rng.uniform(-1.0, 1.0, (n, W, A)) * 10.0 ** rng.uniform(-3.0, 3.0, (n, W, A))
    idx = np.minimum(np.arange(W) + shift, W - 1)
    scale = 10.0 ** rng.uniform(-1.0, 1.0, (n, N + M, 1, 1))
    scale[:, N:] *= WEAK_SCALE
    cands = prev[:, None, idx] + scale * rng.standard_normal((n, N + M, W, A))
    return cands.astype(np.float32), prev.astype(np.float32)


@functools.lru_cache(maxsize=None)
def table(W, A, shift, N, M, K):
    """One shape of the table: (cands, prev) of CASE_ENVS environments, read-only, and refs[(lam, has_prev)][env] = (reference, total bound,
    fc bound, decisive)."""
    cands, prev = make_case(case_rng(W, A, shift, N, M), CASE_ENVS, N, M, W, A, shift)
    cands.setflags(write=False)
    prev.setflags(write=False)
    refs = {}
    for lam in LAMBDAS:
        for has in (True, False):
            rows = []
            for i in range(CASE_ENVS):
                ref = reference(cands[i], prev[i], has, shift, RHO, N, K, lam)
                bt = total_bound(ref, W, A, shift, lam)
                rows.append((ref, bt, fc_bound(ref, W, A), decisive(ref, bt, R.score_bound(W - shift, A), N, K, has)))
            refs[(lam, has)] = rows
    return cands, prev, refs
