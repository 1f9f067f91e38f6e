"""CPU: warm-started replanning in rollout.VectorEnvPolicy - the constructor's refusals, the entry point it binds and its bad-argument paths, and
the fp64 restatement of the latent formula (the one tests/test_gpu_vector_env_warm.py holds the kernel to)."""
import numpy as np
import pytest

import mode_diffusion_policy_amd as M
from mode_diffusion_policy_amd import _lib as L
from mode_diffusion_policy_amd import rollout
from oracle.weights import get_config

from warm_refs import np_noise, shift_hold_index, warm_latents


def _den():
    cfg = get_config("tiny")
    m = M.MoDeDiT(obs_dim=cfg.obs_dim, goal_dim=cfg.goal_dim, device="cpu", goal_conditioned=True, action_dim=cfg.action_dim, embed_dim=cfg.embed_dim,
                  embed_pdrob=0, attn_pdrop=0.0, n_layers=cfg.n_layers, n_heads=cfg.n_heads, goal_seq_len=1, obs_seq_len=1,
                  action_seq_len=cfg.action_seq_len, num_experts=cfg.num_experts, top_k=cfg.top_k)
    return M.GCDenoiser(m, 0.5).eval(), cfg


# ------------------------------------------------------------------------------------------------------------------ refusals
@pytest.mark.parametrize("bad", [0, 10, -1, 11, 5.0, 0.5, True, "5"])
def test_warm_start_outside_the_schedule_or_not_an_int_is_refused(bad):
    den, cfg = _den()
    assert cfg.action_seq_len > 1
    with pytest.raises(ValueError, match="warm_start"):
        rollout.VectorEnvPolicy(den, 4, act_window_size=cfg.action_seq_len, action_dim=cfg.action_dim, multistep=1, num_sampling_steps=10, warm_start=bad)


def test_warm_start_bounds_follow_num_sampling_steps():
    den, cfg = _den()
    kw = dict(act_window_size=cfg.action_seq_len, action_dim=cfg.action_dim, multistep=1)
    for n, k in ((4, 4), (4, 0), (2, 2), (1, 1)):                  # (a 1-step schedule has no level to resume from)
        with pytest.raises(ValueError, match="warm_start"):
            rollout.VectorEnvPolicy(den, 4, num_sampling_steps=n, warm_start=k, **kw)


def test_warm_start_needs_a_tail_of_the_old_plan():
    den, cfg = _den()
    W = cfg.action_seq_len
    with pytest.raises(ValueError, match="multistep < act_window_size"):
        rollout.VectorEnvPolicy(den, 4, act_window_size=W, action_dim=cfg.action_dim, multistep=W, warm_start=5)
    with pytest.raises(ValueError, match="multistep < act_window_size"):                       # (the default multistep is the window)
        rollout.VectorEnvPolicy(den, 4, act_window_size=10, action_dim=cfg.action_dim, warm_start=5)


def test_valid_option_reaches_the_older_checks():
    """A valid k passes the new checks; the refusals that were there before still speak (here: the parameters are on the host)."""
    den, cfg = _den()
    kw = dict(act_window_size=cfg.action_seq_len, action_dim=cfg.action_dim, multistep=1)
    for k in (1, 5, 9, np.int64(3)):
        with pytest.raises(ValueError, match="ROCm device"):
            rollout.VectorEnvPolicy(den, 4, warm_start=k, **kw)
    with pytest.raises(ValueError, match="ROCm device"):
        rollout.VectorEnvPolicy(den, 4, warm_start=3, num_sampling_steps=4, temporal_ensemble=0.5, **kw)
    with pytest.raises(ValueError, match="deterministic fused samplers"):
        rollout.VectorEnvPolicy(den, 4, warm_start=5, sampler_type="euler_ancestral", **kw)


# ------------------------------------------------------------------------------------------------------------------ ABI surface
_GOOD = dict(rows=16, m_b=4, num_envs=4, seeds=16, draws=16, state_images=None, img_floats=0, goals=None, goal_floats=0, img_out=None, goal_out=None,
             x0=16, plan=16, W=10, A=7, shift=5, sigma_start=1.0)


def test_gather_warm_is_bound_and_the_abi_stays_13():
    lib = L.load()
    assert L.ABI_VERSION == 13 and lib.mode_hip_version() == 13
    assert hasattr(lib, "mode_env_gather_warm") and "mode_env_gather_warm" in L.PROTOTYPES
    assert len(L.PROTOTYPES["mode_env_gather_warm"][1]) == len(_GOOD) + 1                    # (+ the stream)


@pytest.mark.parametrize("over", [dict(plan=None), dict(rows=None), dict(seeds=None), dict(draws=None), dict(x0=None), dict(W=0), dict(W=-3), dict(A=0),
                                  dict(A=-1), dict(W=64, A=65, shift=1), dict(W=4097, A=1, shift=1), dict(W=65536, A=65536, shift=1), dict(shift=0),
                                  dict(shift=-1), dict(shift=10), dict(shift=11), dict(sigma_start=float("nan")), dict(sigma_start=float("inf")),
                                  dict(sigma_start=-float("inf")), dict(sigma_start=-1e-30), dict(m_b=0), dict(m_b=-2), dict(num_envs=0),
                                  dict(num_envs=-1)], ids=lambda o: ",".join(f"{k}={v}" for k, v in o.items()))
def test_gather_warm_refuses_before_any_launch(over):
    """stream = None and pointers that must never be followed: every refusal returns MODE_ERR_BAD_ARG (-1) from the host-side check."""
    lib = L.load()
    args = dict(_GOOD, **over)
    assert lib.mode_env_gather_warm(*args.values(), None) == -1, over


# ------------------------------------------------------------------------------------------------------------------ the formula
@pytest.mark.parametrize("W,s", [(10, 1), (10, 9), (6, 5), (2, 1), (37, 5)])             # s = 1, s = W - 1, W = 1 + s
def test_shift_hold_index_map(W, s):
    idx = shift_hold_index(W, s)
    assert idx.tolist() == [min(w + s, W - 1) for w in range(W)]
    assert idx.tolist() == list(range(s, W)) + [W - 1] * s                               # the tail of the old plan, then its last row held
    assert idx[0] == s and idx[-1] == W - 1 and (np.diff(idx) >= 0).all()


@pytest.mark.parametrize("W,A,s", [(10, 7, 1), (10, 7, 9), (6, 3, 5)])
def test_restatement_of_the_latent_formula(W, A, s):
    rng = np.random.default_rng(W * A + s)
    plan = rng.standard_normal((W, A)).astype(np.float32)
    seed, draw = 2 ** 32 - 1, 2 ** 20
    x, z = warm_latents(plan, seed, draw, s, 0.0)
    assert np.array_equal(x, plan.astype(np.float64)[shift_hold_index(W, s)])              # sigma_start = 0: the shifted plan itself
    assert np.array_equal(z.reshape(-1), np_noise(seed, draw, W * A))                     # element e = w * A + a of the cold replan's stream
    for sigma in (0.37, 80.0):
        x, z2 = warm_latents(plan, seed, draw, s, sigma)
        assert np.array_equal(z, z2)
        for w in range(W):
            want = plan[min(w + s, W - 1)].astype(np.float64) + float(np.float32(sigma)) * z[w]
            assert np.array_equal(x[w], want), (sigma, w)
    # the same stream as the cold replan, another draw another noise
    assert not np.array_equal(np_noise(seed, draw, W * A), np_noise(seed, draw + 1, W * A))
