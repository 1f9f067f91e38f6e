"""CPU: forward contrast in rollout.VectorEnvPolicy(candidates=N, contrast=M) - the fp64 restatement the GPU tests hold the kernel to
(tests/bid_refs.py) against a brute-force loop, its limits (lambda = 0, K >= N and M), the share of the seeded table in which the fp32 choice
must equal the fp64 one, the constructor's and select_bidirectional's refusals, the new struct's size and the bad-argument paths of the new
exports (they return before any launch)."""
import ctypes as C

import numpy as np
import pytest
import torch

from mode_diffusion_policy_amd import _lib as L
from mode_diffusion_policy_amd import rollout

import bid_refs as B
import cand_refs as R
from test_vector_env_candidates import _den, _kw


# ------------------------------------------------------------------------------------------------------------------ the restatement
def _brute(cands, prev, has_prev, shift, rho, N, K, lam):
    """The rule of include/mode_hip.h with explicit loops and a selection sort, sharing nothing with bid_refs.reference."""
    NT, W, A = cands.shape
    M, Lh = NT - N, W - shift
    x, p = cands.astype(np.float64), prev.astype(np.float64)
    bc = [sum(rho ** w * sum((x[c, w, a] - p[w + shift, a]) ** 2 for a in range(A)) for w in range(Lh)) if has_prev else 0.0 for c in range(NT)]

    def smallest(idx, k):
        left, out = list(idx), []
        while len(out) < k:
            best = left[0]
            for c in left[1:]:
                if bc[c] < bc[best] or (np.isnan(bc[best]) and not np.isnan(bc[c])):
                    best = c
            out.append(best)
            left.remove(best)
        return out
    sp, sn = smallest(range(N), min(K, N)), smallest(range(N, NT), min(K, M))
    d = lambda a, b: sum((x[a, w, i] - x[b, w, i]) ** 2 for w in range(W) for i in range(A))
    fc = [sum(d(c, q) for q in sp) / len(sp) - sum(d(c, q) for q in sn) / len(sn) for c in range(N)]
    total = [bc[c] + lam * fc[c] for c in range(N)]
    best = 0
    for c in range(1, N):
        if total[c] < total[best] or (np.isnan(total[best]) and not np.isnan(total[c])):
            best = c
    return bc, sp, sn, fc, total, best


@pytest.mark.parametrize("W,A,shift,N,M,K", B.CASES[:4])
def test_reference_equals_a_brute_force_loop(W, A, shift, N, M, K):
    cands, prev, _ = B.table(W, A, shift, N, M, K)
    for i in (0, B.CASE_ENVS - 1):
        for has in (True, False):
            ref = B.reference(cands[i], prev[i], has, shift, B.RHO, N, K, 0.25)
            bc, sp, sn, fc, total, best = _brute(cands[i], prev[i], has, shift, B.RHO, N, K, 0.25)
            assert list(ref["sp"]) == sp and list(ref["sn"]) == sn and ref["selected"] == best
            assert np.allclose(ref["bc"], bc, rtol=1e-12, atol=0) and np.allclose(ref["total"], total, rtol=1e-9, atol=1e-9 * np.abs(bc[:N]).max())
            assert np.allclose(ref["fc"], fc, rtol=1e-9, atol=1e-9 * (ref["pos"] + ref["neg"]).max())
            if not has:
                assert sp == list(range(min(K, N))) and sn == list(range(N, N + min(K, M))) and not ref["bc"].any()


def test_ranking_ties_and_nans():
    nan = float("nan")
    assert list(B.ranked([3.0, 1.0, 2.0, 1.0], 3)) == [1, 3, 2]                            # the lower index wins ties
    assert list(B.ranked([nan, 2.0, nan, 1.0], 4)) == [3, 1, 0, 2]                          # a NaN ranks after every non-NaN, NaNs by index
    assert list(B.ranked([0.0, 0.0, 0.0], 2)) == [0, 1] and list(B.ranked([np.inf, nan, 5.0], 2)) == [2, 0]


def test_lambda_zero_is_the_coherence_selection():
    for W, A, shift, N, M, K in B.CASES[:4]:
        cands, prev, _ = B.table(W, A, shift, N, M, K)
        for i in range(B.CASE_ENVS):
            ref = B.reference(cands[i], prev[i], True, shift, B.RHO, N, K, 0.0)
            sc = R.scores64(cands[i, :N], prev[i], shift, B.RHO)
            assert np.array_equal(ref["total"], sc) and ref["selected"] == R.select(sc)


def test_topk_beyond_both_counts_means_all():
    W, A, shift, N, M, _ = B.CASES[3]
    cands, prev, _ = B.table(*B.CASES[3])
    for i in range(B.CASE_ENVS):
        a, b = (B.reference(cands[i], prev[i], True, shift, B.RHO, N, K, 1.0) for K in (max(N, M), 64))
        assert sorted(a["sp"]) == list(range(N)) and sorted(a["sn"]) == list(range(N, N + M))
        assert all(np.array_equal(a[k], b[k]) for k in ("sp", "sn", "fc", "total")) and a["selected"] == b["selected"]
        # with every candidate in both sets fc_c is the mean distance to the strong ones minus the mean distance to the weak ones
        want = [np.mean([B.dist64(cands[i, c], cands[i, p]) for p in range(N)]) - np.mean([B.dist64(cands[i, c], cands[i, q]) for q in range(N, N + M)])
                for c in range(N)]
        assert np.allclose(a["fc"], want, rtol=1e-12)


def test_the_exact_comparison_covers_the_committed_table():
    """The GPU test compares the kernel's choice with the fp64 argmin only on decisive rows (bid_refs.decisive).  Over the committed table -
    5 shapes x 6 environments x 2 lambdas x with / without a previous plan - these must be at least 90 %: a condition on the table."""
    total = covered = 0
    for case in B.CASES:
        _, _, refs = B.table(*case)
        assert sorted(refs) == sorted((lam, has) for lam in B.LAMBDAS for has in (True, False))
        for rows in refs.values():
            total += len(rows)
            covered += sum(bool(dec) for _, _, _, dec in rows)
    print(f"decisive: {covered} of {total}")
    assert total == len(B.CASES) * B.CASE_ENVS * 4 == 120 and covered >= B.DECISIVE_SHARE * total, (covered, total)


def test_bounds_are_positive_and_scale_with_the_magnitudes():
    W, A, shift, N, M, K = B.CASES[1]
    _, _, refs = B.table(*B.CASES[1])
    for (lam, has), rows in refs.items():
        for ref, bt, bf, _ in rows:
            mag = ref["bc"][:N] + lam * (ref["pos"] / ref["Ks"] + ref["neg"] / ref["Kw"])
            n = -(-W * A // 64) + 6 + 2 + K + 3                                          # the chain of bid_refs.total_bound, counted here again
            assert np.all(bt > 0) and np.all(bf > 0) and np.allclose(bt, n * 2.0 ** -24 * mag, rtol=1e-4)
            assert np.all(np.abs(ref["total"]) <= mag * (1 + 1e-12))


# ------------------------------------------------------------------------------------------------------------------ the constructor
@pytest.mark.parametrize("bad", [0, -1, 2.0, 0.5, True, "4"])
def test_contrast_not_a_positive_int_is_refused(bad):
    den, cfg = _den()
    with pytest.raises(ValueError, match=r"contrast must be None or an int >= 1"):
        rollout.VectorEnvPolicy(den, 4, candidates=4, contrast=bad, **_kw(cfg))


@pytest.mark.parametrize("cand", [None, 1])
def test_contrast_needs_two_candidates(cand):
    den, cfg = _den()
    with pytest.raises(ValueError, match="needs candidates >= 2"):
        rollout.VectorEnvPolicy(den, 4, candidates=cand, contrast=4, **_kw(cfg))


def test_contrast_batch_limits():
    den, cfg = _den()
    for N, M in ((60, 5), (2, 63), (33, 32)):
        with pytest.raises(ValueError, match=r"candidates \+ contrast must be at most 64"):
            rollout.VectorEnvPolicy(den, 1, candidates=N, contrast=M, **_kw(cfg))
    for n, N, M in ((129, 4, 4), (17, 32, 32), (342, 2, 1)):
        with pytest.raises(ValueError, match=rf"num_envs \* \(candidates \+ contrast\) must be at most {L.MODE_ENV_MAX}"):
            rollout.VectorEnvPolicy(den, n, candidates=N, contrast=M, **_kw(cfg))


@pytest.mark.parametrize("bad", [0, -2, 1.5, True, "2"])
def test_contrast_topk_not_a_positive_int_is_refused(bad):
    den, cfg = _den()
    with pytest.raises(ValueError, match=r"contrast_topk must be None or an int >= 1"):
        rollout.VectorEnvPolicy(den, 4, candidates=4, contrast=4, contrast_topk=bad, **_kw(cfg))


@pytest.mark.parametrize("bad", [-0.5, -1e-30, float("nan"), float("inf"), "x", True])
def test_contrast_weight_not_finite_or_negative_is_refused(bad):
    den, cfg = _den()
    with pytest.raises(ValueError, match=r"contrast_weight must be a finite float >= 0"):
        rollout.VectorEnvPolicy(den, 4, candidates=4, contrast=4, contrast_weight=bad, **_kw(cfg))


@pytest.mark.parametrize("kw", [dict(contrast_weight=1.0), dict(contrast_topk=2), dict(candidates=4, contrast_weight=0.5),
                                dict(candidates=4, contrast_topk=1)], ids=lambda k: ",".join(k))
def test_contrast_weight_and_topk_are_only_legal_with_contrast(kw):
    den, cfg = _den()
    with pytest.raises(ValueError, match="only legal with contrast"):
        rollout.VectorEnvPolicy(den, 4, **_kw(cfg, **kw))


def test_valid_contrast_options_reach_the_older_checks():
    """Valid values pass the new checks - which all come before any allocation -; the refusals that were there before still speak (here: the
    parameters are on the host)."""
    den, cfg = _den()
    for kw in (dict(candidates=2, contrast=1), dict(candidates=4, contrast=4, contrast_weight=0.0), dict(candidates=32, contrast=32, contrast_topk=100),
               dict(candidates=np.int64(4), contrast=np.int64(2), contrast_topk=np.int64(1), contrast_weight=2),
               dict(candidates=4, contrast=4, warm_start=5, temporal_ensemble=0.5)):
        with pytest.raises(ValueError, match="ROCm device"):
            rollout.VectorEnvPolicy(den, 4, **_kw(cfg, **kw))
    with pytest.raises(ValueError, match="ROCm device"):
        rollout.VectorEnvPolicy(den, 128, candidates=4, contrast=4, **_kw(cfg))                # 128 * 8 = MODE_ENV_MAX: allowed
    with pytest.raises(ValueError, match="multistep < act_window_size"):
        rollout.VectorEnvPolicy(den, 4, candidates=4, contrast=4, **_kw(cfg, multistep=cfg.action_seq_len))


# ------------------------------------------------------------------------------------------------------------------ select_bidirectional's arguments
def _good(n=3, NT=6, W=6, A=2):
    return dict(chunk=torch.zeros(n, NT, W, A), prev=torch.zeros(n, W, A), has_prev=[True] * n, shift=2, weights=np.ones(W - 2, dtype=np.float32),
                n_weak=2, topk=2, contrast_weight=1.0)


@pytest.mark.parametrize("over,msg", [
    (dict(chunk=torch.zeros(3, 6, 2)), r"chunk must be a non-empty \(n, N \+ M, W, A\) tensor"),
    (dict(chunk=torch.zeros(0, 6, 6, 2)), r"chunk must be a non-empty \(n, N \+ M, W, A\) tensor"),
    (dict(chunk=torch.zeros(3, 65, 6, 2)), r"N \+ M must be at most 64, got 65"),
    (dict(n_weak=0), r"n_weak must be an int in \[1, 5\]"),
    (dict(n_weak=6), r"n_weak must be an int in \[1, 5\]"),
    (dict(n_weak=2.0), r"n_weak must be an int in \[1, 5\]"),
    (dict(topk=0), "topk must be an int >= 1"),
    (dict(topk=True), "topk must be an int >= 1"),
    (dict(contrast_weight=-1.0), "contrast_weight must be a finite float >= 0"),
    (dict(contrast_weight=float("nan")), "contrast_weight must be a finite float >= 0"),
    (dict(chunk=torch.zeros(1, 3, 64, 65), prev=torch.zeros(1, 64, 65), has_prev=[True]), r"W \* A must be at most 4096"),
    (dict(prev=torch.zeros(3, 6, 3)), r"prev must be \(3, 6, 2\)"),
    (dict(has_prev=[1, 0, 1]), "has_prev must be 3 host bools"),
    (dict(shift=0), r"shift must be an int in \[1, W - 1\] = \[1, 5\]"),
    (dict(shift=6), r"shift must be an int in \[1, W - 1\] = \[1, 5\]"),
    (dict(weights=np.ones(5, dtype=np.float32)), r"weights must have W - shift = 4 entries, got 5"),
    ({}, "must be on one ROCm device"),
], ids=lambda v: None if isinstance(v, dict) else v[:24])
def test_select_bidirectional_refuses_bad_arguments(over, msg):
    with pytest.raises(ValueError, match="select_bidirectional: .*" + msg):
        rollout.select_bidirectional(**dict(_good(), **over))


# ------------------------------------------------------------------------------------------------------------------ ABI surface
_BID = dict(rows=16, has_prev=16, count=None, chunk=16, plan=16, weights=16, chosen=16, selected=16, scores=16, lambda_=16, bc=16, fc=16, m_b=4,
            num_envs=4, W=10, A=7, shift=4, N=4, M=4, K=2)
_NOISE = dict(rows=16, m_b=4, num_envs=4, seeds=16, draws=16, state_images=None, img_floats=0, goals=None, goal_floats=0, img_out=None, goal_out=None,
              x0=16, noise_floats=70, sigma_max=80.0, N=4, M=4)
_WARM = dict(rows=16, m_b=4, num_envs=4, seeds=16, draws=16, state_images=None, img_floats=0, goals=None, goal_floats=0, img_out=None, goal_out=None,
             x0=16, plan=16, W=10, A=7, shift=5, sigma_start=1.0, N=4, M=4)
_ids = lambda o: ",".join(f"{k}={v}" for k, v in o.items())


def test_the_new_exports_are_bound_and_the_abi_stays_13():
    lib = L.load()
    assert L.ABI_VERSION == 13 and lib.mode_hip_version() == 13
    for name, good in (("mode_env_gather_noise_bid", _NOISE), ("mode_env_gather_warm_bid", _WARM)):
        assert hasattr(lib, name) and len(L.PROTOTYPES[name][1]) == len(good) + 1              # (+ the stream)
        assert len(L.PROTOTYPES[name][1]) == len(L.PROTOTYPES[name.replace("_bid", "_cand")][1]) + 1
    assert hasattr(lib, "mode_env_select_bid") and [f[0] for f in L.ModeEnvBidDesc._fields_] == list(_BID)
    assert lib.mode_hip_sizeof(b"ModeEnvBidDesc") == C.sizeof(L.ModeEnvBidDesc) == 128
    old = [f[0] for f in L.ModeEnvSelectDesc._fields_]
    assert set(old) <= set(_BID) and C.sizeof(L.ModeEnvSelectDesc) == 96                       # the older struct's fields, and it is unchanged


@pytest.mark.parametrize("over", [dict(rows=None), dict(has_prev=None), dict(chunk=None), dict(plan=None), dict(weights=None), dict(chosen=None),
                                  dict(selected=None), dict(scores=None), dict(lambda_=None), dict(bc=None), dict(fc=None), dict(N=0), dict(N=-1),
                                  dict(M=0), dict(M=-1), dict(N=61), dict(N=1, M=64), dict(N=2 ** 31 - 1, M=2), dict(K=0), dict(K=-1), dict(W=64, A=65),
                                  dict(W=4097, A=1), dict(W=65536, A=65536), dict(W=0), dict(A=0), dict(shift=0), dict(shift=10), dict(shift=11),
                                  dict(m_b=0), dict(m_b=-3), dict(num_envs=0)], ids=_ids)
def test_select_bid_refuses_before_any_launch(over):
    """stream = None and pointers that must never be followed: every refusal returns MODE_ERR_BAD_ARG (-1) from the host-side check."""
    d = L.ModeEnvBidDesc(**dict(_BID, **over))
    assert L.load().mode_env_select_bid(C.byref(d), None) == -1, over


def test_select_bid_refuses_a_null_desc():
    assert L.load().mode_env_select_bid(None, None) == -1


@pytest.mark.parametrize("over", [dict(N=0), dict(M=0), dict(M=-1), dict(N=61), dict(N=64, M=1), dict(N=2 ** 31 - 1, M=2), dict(rows=None),
                                  dict(seeds=None), dict(draws=None), dict(x0=None), dict(m_b=0), dict(num_envs=0), dict(noise_floats=0)], ids=_ids)
def test_gather_noise_bid_refuses_before_any_launch(over):
    args = dict(_NOISE, **over)
    assert L.load().mode_env_gather_noise_bid(*args.values(), None) == -1, over


@pytest.mark.parametrize("over", [dict(N=0), dict(M=0), dict(M=-1), dict(N=61), dict(N=64, M=1), dict(plan=None), dict(rows=None), dict(x0=None),
                                  dict(W=64, A=65, shift=1), dict(shift=0), dict(shift=10), dict(sigma_start=float("nan")), dict(m_b=0)], ids=_ids)
def test_gather_warm_bid_refuses_before_any_launch(over):
    args = dict(_WARM, **over)
    assert L.load().mode_env_gather_warm_bid(*args.values(), None) == -1, over
