"""CPU: candidate selection in rollout.VectorEnvPolicy(candidates=N) - the constructor's and select_coherent's refusals, the weight table, the
new struct's size, the bad-argument paths of the new exports (they return before any launch), and the fp64 restatement the GPU tests hold the
kernel to (tests/cand_refs.py), including the share of seeded cases in which the fp32 argmin must equal the fp64 one."""
import ctypes as C

import numpy as np
import pytest
import torch

import mode_diffusion_policy_amd as M
from mode_diffusion_policy_amd import _lib as L
from mode_diffusion_policy_amd import rollout
from oracle.weights import get_config

import cand_refs as R


def _den():
    cfg = get_config("tiny")
    m = M.MoDeDiT(obs_dim=cfg.obs_dim, goal_dim=cfg.goal_dim, device="cpu", goal_conditioned=True, action_dim=cfg.action_dim, embed_dim=cfg.embed_dim,
                  embed_pdrob=0, attn_pdrop=0.0, n_layers=cfg.n_layers, n_heads=cfg.n_heads, goal_seq_len=1, obs_seq_len=1,
                  action_seq_len=cfg.action_seq_len, num_experts=cfg.num_experts, top_k=cfg.top_k)
    return M.GCDenoiser(m, 0.5).eval(), cfg


def _kw(cfg, **over):
    return dict(dict(act_window_size=cfg.action_seq_len, action_dim=cfg.action_dim, multistep=1), **over)


# ------------------------------------------------------------------------------------------------------------------ the constructor
@pytest.mark.parametrize("bad", [0, -1, 65, 1000, 2.0, 0.5, True, "4"])
def test_candidates_outside_the_range_or_not_an_int_is_refused(bad):
    den, cfg = _den()
    with pytest.raises(ValueError, match=r"candidates must be None or an int in \[1, 64\]"):
        rollout.VectorEnvPolicy(den, 4, candidates=bad, **_kw(cfg))


def test_candidates_need_an_overlap_to_score():
    den, cfg = _den()
    W = cfg.action_seq_len
    with pytest.raises(ValueError, match="multistep < act_window_size"):
        rollout.VectorEnvPolicy(den, 4, candidates=2, **_kw(cfg, multistep=W))
    with pytest.raises(ValueError, match="multistep < act_window_size"):                       # (the default multistep is the window)
        rollout.VectorEnvPolicy(den, 4, act_window_size=10, action_dim=cfg.action_dim, candidates=8)


def test_candidate_batch_stays_within_the_largest_bucket():
    den, cfg = _den()
    for n, N in ((513, 2), (17, 64), (L.MODE_ENV_MAX, 2)):
        with pytest.raises(ValueError, match=rf"num_envs \* candidates must be at most {L.MODE_ENV_MAX}"):
            rollout.VectorEnvPolicy(den, n, candidates=N, **_kw(cfg))


@pytest.mark.parametrize("bad", [0.0, -0.5, 1.0001, 2, float("nan"), float("inf"), "x", True])
def test_coherence_decay_outside_the_range_is_refused(bad):
    den, cfg = _den()
    with pytest.raises(ValueError, match=r"coherence_decay must be a finite float in \(0, 1\]"):
        rollout.VectorEnvPolicy(den, 4, candidates=4, coherence_decay=bad, **_kw(cfg))


def test_coherence_decay_is_only_legal_with_candidates():
    den, cfg = _den()
    with pytest.raises(ValueError, match="only legal with candidates"):
        rollout.VectorEnvPolicy(den, 4, coherence_decay=0.5, **_kw(cfg))


def test_valid_options_reach_the_older_checks():
    """Valid values pass the new checks; the refusals that were there before still speak (here: the parameters are on the host)."""
    den, cfg = _den()
    for kw in (dict(candidates=None), dict(candidates=1), dict(candidates=1, coherence_decay=0.9), dict(candidates=2), dict(candidates=64),
               dict(candidates=np.int64(8), coherence_decay=1.0), dict(candidates=4, coherence_decay=1e-3),
               dict(candidates=4, warm_start=5, temporal_ensemble=0.5), dict(candidates=1, multistep=cfg.action_seq_len)):
        with pytest.raises(ValueError, match="ROCm device"):
            rollout.VectorEnvPolicy(den, 4, **_kw(cfg, **kw))
    with pytest.raises(ValueError, match="ROCm device"):
        rollout.VectorEnvPolicy(den, 16, candidates=64, **_kw(cfg))                             # 16 * 64 = MODE_ENV_MAX: allowed
    with pytest.raises(ValueError, match="deterministic fused samplers"):
        rollout.VectorEnvPolicy(den, 4, candidates=4, sampler_type="euler_ancestral", **_kw(cfg))


# ------------------------------------------------------------------------------------------------------------------ the weight table
@pytest.mark.parametrize("rho,n", [(0.5, 9), (1.0, 6), (0.9, 63), (1e-3, 5), (0.37, 1)])
def test_coherence_weights_are_the_fp64_powers_rounded_to_fp32(rho, n):
    w = rollout.coherence_weights(rho, n)
    assert w.dtype == np.float32 and w.shape == (n,) and w[0] == 1.0
    want = np.array([rho ** i for i in range(n)], dtype=np.float64)
    assert np.array_equal(w, want.astype(np.float32))
    assert np.all(np.abs(w.astype(np.float64) - R.weights64(rho, n)) <= 2.0 ** -24 * R.weights64(rho, n) + 1e-45)
    assert rollout.coherence_weights(rho, 0).shape == (0,)


# ------------------------------------------------------------------------------------------------------------------ select_coherent's arguments
def _good(n=3, N=4, W=6, A=2):
    return dict(chunk=torch.zeros(n, N, W, A), prev=torch.zeros(n, W, A), has_prev=[True] * n, shift=2, weights=np.ones(W - 2, dtype=np.float32))


@pytest.mark.parametrize("over,msg", [
    (dict(chunk=torch.zeros(3, 6, 2)), r"chunk must be a non-empty \(n, N, W, A\) tensor"),
    (dict(chunk=np.zeros((3, 4, 6, 2))), r"chunk must be a non-empty \(n, N, W, A\) tensor"),
    (dict(chunk=torch.zeros(0, 4, 6, 2)), r"chunk must be a non-empty \(n, N, W, A\) tensor"),
    (dict(chunk=torch.zeros(3, 65, 6, 2)), r"N must be in \[1, 64\], got 65"),
    (dict(chunk=torch.zeros(1, 2, 64, 65), prev=torch.zeros(1, 64, 65), has_prev=[True]), r"W \* A must be at most 4096"),
    (dict(prev=torch.zeros(3, 6, 3)), r"prev must be \(3, 6, 2\)"),
    (dict(prev=torch.zeros(2, 6, 2)), r"prev must be \(3, 6, 2\)"),
    (dict(has_prev=[True, False]), "has_prev must be 3 host bools"),
    (dict(has_prev=[1, 0, 1]), "has_prev must be 3 host bools"),
    (dict(shift=0), r"shift must be an int in \[1, W - 1\] = \[1, 5\]"),
    (dict(shift=6), r"shift must be an int in \[1, W - 1\] = \[1, 5\]"),
    (dict(shift=2.0), r"shift must be an int in \[1, W - 1\] = \[1, 5\]"),
    (dict(weights=np.ones(5, dtype=np.float32)), r"weights must have W - shift = 4 entries, got 5"),
    ({}, "must be on one ROCm device"),
], ids=lambda v: None if isinstance(v, dict) else v[:24])
def test_select_coherent_refuses_bad_arguments(over, msg):
    with pytest.raises(ValueError, match="select_coherent: .*" + msg):
        rollout.select_coherent(**dict(_good(), **over))


# ------------------------------------------------------------------------------------------------------------------ ABI surface
_SEL = dict(rows=16, has_prev=16, count=None, chunk=16, plan=16, weights=16, chosen=16, selected=16, scores=16, m_b=4, num_envs=4, W=10, A=7, shift=4, N=8)
_NOISE = dict(rows=16, m_b=4, num_envs=4, seeds=16, draws=16, state_images=None, img_floats=0, goals=None, goal_floats=0, img_out=None, goal_out=None,
              x0=16, noise_floats=70, sigma_max=80.0, N=4)
_WARM = dict(rows=16, m_b=4, num_envs=4, seeds=16, draws=16, state_images=None, img_floats=0, goals=None, goal_floats=0, img_out=None, goal_out=None,
             x0=16, plan=16, W=10, A=7, shift=5, sigma_start=1.0, N=4)
_ids = lambda o: ",".join(f"{k}={v}" for k, v in o.items())


def test_the_new_exports_are_bound_and_the_abi_stays_13():
    lib = L.load()
    assert L.ABI_VERSION == 13 and lib.mode_hip_version() == 13
    for name, good in (("mode_env_gather_noise_cand", _NOISE), ("mode_env_gather_warm_cand", _WARM)):
        assert hasattr(lib, name) and len(L.PROTOTYPES[name][1]) == len(good) + 1              # (+ the stream)
    assert hasattr(lib, "mode_env_select") and [f[0] for f in L.ModeEnvSelectDesc._fields_] == list(_SEL)
    assert lib.mode_hip_sizeof(b"ModeEnvSelectDesc") == C.sizeof(L.ModeEnvSelectDesc) == 96


@pytest.mark.parametrize("over", [dict(rows=None), dict(has_prev=None), dict(chunk=None), dict(plan=None), dict(weights=None), dict(chosen=None),
                                  dict(selected=None), dict(scores=None), dict(N=0), dict(N=-1), dict(N=65), dict(W=64, A=65), dict(W=4097, A=1),
                                  dict(W=65536, A=65536), dict(W=0), dict(A=0), dict(A=-2), dict(shift=0), dict(shift=-1), dict(shift=10),
                                  dict(shift=11), dict(m_b=0), dict(m_b=-3), dict(num_envs=0)], ids=_ids)
def test_select_refuses_before_any_launch(over):
    """stream = None and pointers that must never be followed: every refusal returns MODE_ERR_BAD_ARG (-1) from the host-side check."""
    lib = L.load()
    d = L.ModeEnvSelectDesc(**dict(_SEL, **over))
    assert lib.mode_env_select(C.byref(d), None) == -1, over


def test_select_refuses_a_null_desc():
    assert L.load().mode_env_select(None, None) == -1


@pytest.mark.parametrize("over", [dict(N=0), dict(N=-1), dict(N=65), dict(rows=None), dict(seeds=None), dict(draws=None), dict(x0=None), dict(m_b=0),
                                  dict(num_envs=0), dict(noise_floats=0), dict(img_floats=-1), dict(goal_floats=-1)], ids=_ids)
def test_gather_noise_cand_refuses_before_any_launch(over):
    args = dict(_NOISE, **over)
    assert L.load().mode_env_gather_noise_cand(*args.values(), None) == -1, over


@pytest.mark.parametrize("over", [dict(N=0), dict(N=-1), dict(N=65), dict(plan=None), dict(rows=None), dict(seeds=None), dict(draws=None), dict(x0=None),
                                  dict(W=0), dict(A=0), dict(W=64, A=65, shift=1), dict(shift=0), dict(shift=10), dict(sigma_start=float("nan")),
                                  dict(sigma_start=-1e-30), dict(m_b=0), dict(num_envs=0)], ids=_ids)
def test_gather_warm_cand_refuses_before_any_launch(over):
    args = dict(_WARM, **over)
    assert L.load().mode_env_gather_warm_cand(*args.values(), None) == -1, over


# ------------------------------------------------------------------------------------------------------------------ the restatement
def test_restatement_of_the_score_and_the_rule():
    rng = np.random.default_rng(0)
    W, A, s, rho = 6, 3, 2, 0.5
    prev, x = rng.standard_normal((W, A)), rng.standard_normal((3, W, A))
    sc = R.scores64(x, prev, s, rho)
    for c in range(3):
        want = sum(rho ** w * sum((x[c, w, a] - prev[w + s, a]) ** 2 for a in range(A)) for w in range(W - s))
        assert abs(sc[c] - want) <= 1e-12 * want
    x[1, :W - s] = prev[s:]                                                              # the previous plan's own tail: score 0, whatever follows it
    assert R.scores64(x, prev, s, rho)[1] == 0.0
    nan = float("nan")
    assert R.select([3.0, 1.0, 2.0]) == 1 and R.select([2.0, 1.0, 1.0]) == 1 and R.select([1.0, 1.0]) == 0
    assert R.select([nan, 5.0, 4.0]) == 2 and R.select([1.0, nan, 0.5, nan]) == 2 and R.select([nan, nan, nan]) == 0 and R.select([nan, 7.0]) == 1
    assert R.select([0.0, 0.0, 0.0]) == 0 and R.select([np.inf, nan, np.inf]) == 0


def test_the_exact_argmin_comparison_covers_the_seeded_cases():
    """The GPU test compares the kernel's choice with the fp64 argmin only where the fp64 gap between the two best scores exceeds twice the
    score bound.  With the seeds and shapes that test uses, that must cover at least 95 % of the rows: checked here with the reference alone."""
    total = covered = 0
    for W, A, s, N in R.SHAPES:
        cands, prev = R.make_case(R.case_rng(W, A, s), R.CASE_ENVS, N, W, A, s)
        for i in range(R.CASE_ENVS):
            total += 1
            covered += bool(R.decisive(R.scores64(cands[i], prev[i], s, R.RHO), R.score_bound(W - s, A)))
    print(f"decisive: {covered} of {total}")
    assert total == len(R.SHAPES) * R.CASE_ENVS and covered >= 0.95 * total, (covered, total)
