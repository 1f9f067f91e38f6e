"""CPU: temporal ensembling in rollout.VectorEnvPolicy - the constructor's refusals, the entry point and descriptor it binds, and a NumPy
restatement of the rule (the one tests/test_gpu_vector_env_ensemble.py holds the kernel to) on hand-made plans."""
import ctypes as C

import numpy as np
import pytest

import mode_diffusion_policy_amd as M
from mode_diffusion_policy_amd import _lib as L
from mode_diffusion_policy_amd import rollout
from oracle.weights import get_config


def _den():
    cfg = get_config("tiny")
    m = M.MoDeDiT(obs_dim=cfg.obs_dim, goal_dim=cfg.goal_dim, device="cpu", goal_conditioned=True, action_dim=cfg.action_dim, embed_dim=cfg.embed_dim,
                  embed_pdrob=0, attn_pdrop=0.0, n_layers=cfg.n_layers, n_heads=cfg.n_heads, goal_seq_len=1, obs_seq_len=1,
                  action_seq_len=cfg.action_seq_len, num_experts=cfg.num_experts, top_k=cfg.top_k)
    return M.GCDenoiser(m, 0.5).eval(), cfg


def ensemble_reference(plans, t, W, m):
    """The rule, restated: ``plans`` = [(t_p, [W, A] array)], any order.  Live at t: 0 <= t - t_p < W.  Oldest first, x_i = row t - t_p of plan i,
    w_i = fp32(exp(-m i)) taken in fp64; a[t] = sum w_i x_i / sum w_i in fp64."""
    live = sorted(((tp, p) for tp, p in plans if 0 <= t - tp < W), key=lambda e: e[0])
    w = np.exp(-float(m) * np.arange(len(live), dtype=np.float64)).astype(np.float32).astype(np.float64)
    x = np.stack([np.asarray(p, dtype=np.float64)[t - tp] for tp, p in live])
    return (w[:, None] * x).sum(0) / w.sum()


def _plans(W, A, s, upto, seed=0):
    rng = np.random.default_rng(seed)
    return [(tp, rng.standard_normal((W, A)).astype(np.float32)) for tp in range(0, upto, s)]


# ------------------------------------------------------------------------------------------------------------------ refusals
@pytest.mark.parametrize("bad", [-0.5, float("nan"), float("inf"), -float("inf")])
def test_negative_or_non_finite_weight_is_refused(bad):
    den, cfg = _den()
    with pytest.raises(ValueError, match="temporal_ensemble"):
        rollout.VectorEnvPolicy(den, 4, act_window_size=cfg.action_seq_len, action_dim=cfg.action_dim, temporal_ensemble=bad)


def test_more_than_64_live_plans_are_refused():
    den, cfg = _den()
    with pytest.raises(ValueError, match="at most 64"):
        rollout.VectorEnvPolicy(den, 4, act_window_size=65, multistep=1, action_dim=cfg.action_dim, temporal_ensemble=0.0)
    with pytest.raises(ValueError, match="at most 64"):
        rollout.VectorEnvPolicy(den, 4, act_window_size=130, multistep=2, action_dim=cfg.action_dim, temporal_ensemble=0.01)


def test_valid_option_reaches_the_older_checks():
    """A valid weight passes the new checks; the refusals that were there before still speak (here: the parameters are on the host)."""
    den, cfg = _den()
    kw = dict(act_window_size=cfg.action_seq_len, action_dim=cfg.action_dim)
    for m in (0, 0.0, 0.01, 1, 50.0):
        with pytest.raises(ValueError, match="ROCm device"):
            rollout.VectorEnvPolicy(den, 4, multistep=1, temporal_ensemble=m, **kw)
    with pytest.raises(ValueError, match="extra_args"):
        rollout.VectorEnvPolicy(den, 4, extra_args={"s_churn": 0.1}, temporal_ensemble=0.0, **kw)
    import torch
    with pytest.raises(ValueError, match="generator"):
        rollout.VectorEnvPolicy(den, 4, generator=torch.Generator(), temporal_ensemble=0.0, **kw)
    with pytest.raises(ValueError, match="deterministic fused samplers"):
        rollout.VectorEnvPolicy(den, 4, sampler_type="euler_ancestral", temporal_ensemble=0.0, **kw)


# ------------------------------------------------------------------------------------------------------------------ ABI surface
def _desc(**over):
    pool = dict(num_envs=4, W=10, A=7, multistep=3, plan=16, counter=16, draws=16, out=16)
    ens = dict(ring=16, birth=16, t=16, weights=16, K=4)
    for k, v in over.items():
        (pool if k in pool or k in ("ctrl", "chunk") else ens)[k] = v
    return L.ModeEnvEnsDesc(pool=L.ModeEnvPoolDesc(**pool), **ens)


def test_ensemble_entry_point_and_descriptor():
    lib = L.load()
    assert hasattr(lib, "mode_env_commit_emit_ens") and "mode_env_commit_emit_ens" in L.PROTOTYPES
    assert lib.mode_hip_sizeof(b"ModeEnvEnsDesc") == C.sizeof(L.ModeEnvEnsDesc) > C.sizeof(L.ModeEnvPoolDesc)
    assert L.ModeEnvEnsDesc.pool.offset == 0 and L.ModeEnvEnsDesc.pool.size == lib.mode_hip_sizeof(b"ModeEnvPoolDesc")
    # bad-argument paths: refused before any launch (the pointers are never followed)
    assert lib.mode_env_commit_emit_ens(None, None) == -1
    for over in (dict(num_envs=0), dict(num_envs=L.MODE_ENV_MAX + 1), dict(multistep=11), dict(multistep=0), dict(A=65), dict(plan=None),
                 dict(counter=None), dict(draws=None), dict(out=None), dict(ctrl=16), dict(ring=None), dict(birth=None), dict(t=None),
                 dict(weights=None), dict(K=0), dict(K=3), dict(K=5), dict(K=65), dict(multistep=10)):
        assert lib.mode_env_commit_emit_ens(C.byref(_desc(**over)), None) == -1, over


def test_weight_table_is_fp64_exp_rounded_to_fp32():
    for m, K in ((0.0, 10), (0.01, 10), (1.0, 4), (50.0, 64)):
        w = rollout.ensemble_weights(m, K)
        assert w.dtype == np.float32 and w.shape == (K,) and w[0] == 1.0
        assert np.array_equal(w, np.array([np.float32(np.exp(np.float64(-m) * i)) for i in range(K)], dtype=np.float32))
    assert np.array_equal(rollout.ensemble_weights(0.0, 7), np.ones(7, dtype=np.float32))
    assert np.array_equal(rollout.ensemble_weights(1e300, 3), np.array([1, 0, 0], dtype=np.float32))


# ------------------------------------------------------------------------------------------------------------------ the rule
def test_restatement_single_plan_is_identity():
    W, A = 10, 7
    plans = _plans(W, A, W, 3 * W)                               # s = W: K = 1
    for t in range(3 * W):
        tp, p = plans[t // W]
        for m in (0.0, 0.01, 1.0):
            assert np.array_equal(ensemble_reference(plans, t, W, m), p[t - tp].astype(np.float64)), (t, m)


def test_restatement_zero_weight_is_the_mean():
    W, A, s = 10, 7, 3
    plans = _plans(W, A, s, 40)
    for t in (0, 2, 3, 9, 10, 11, 25, 38):
        rows = [p[t - tp].astype(np.float64) for tp, p in plans if 0 <= t - tp < W]
        assert len(rows) == min(t // s + 1, -(-(W - t % s) // s))
        np.testing.assert_allclose(ensemble_reference(plans, t, W, 0.0), np.mean(rows, 0), rtol=1e-15, atol=0)
    assert max(sum(0 <= t - tp < W for tp, _ in plans) for t in range(40)) == -(-W // s)        # at most K = ceil(W / s) live plans


def test_restatement_large_weight_tends_to_the_oldest_live_row():
    W, A, s = 10, 7, 1
    plans = _plans(W, A, s, 30)
    for t in (0, 4, 9, 17, 29):
        rows = [p[t - tp].astype(np.float64) for tp, p in plans if 0 <= t - tp < W]            # (listed oldest first)
        want, spread = rows[0], max(np.abs(r - rows[0]).max() for r in rows)
        for m in (1.0, 5.0, 20.0, 200.0):
            # |a - x_0| = |sum_{i>0} w_i (x_i - x_0)| / sum w_i <= (sum_{i>0} w_i) max|x_i - x_0|, since sum w_i >= w_0 = 1
            tail = float(rollout.ensemble_weights(m, len(rows)).astype(np.float64)[1:].sum())
            err = np.abs(ensemble_reference(plans, t, W, m) - want).max()
            assert err <= tail * spread * (1 + 1e-12), (t, m, err)
        assert np.array_equal(ensemble_reference(plans, t, W, 200.0), want)                      # exp(-200) is 0 in fp32


def test_restatement_order_is_by_birth_not_by_listing():
    W, A, s = 10, 7, 3
    plans = _plans(W, A, s, 20)
    for t in (7, 13):
        assert np.array_equal(ensemble_reference(plans, t, W, 0.7), ensemble_reference(plans[::-1], t, W, 0.7))
