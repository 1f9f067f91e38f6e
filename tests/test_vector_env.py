"""CPU: the host-side contract of rollout.VectorEnvPolicy (bucket sizes, constructor validation) and the ABI 13 surface it binds."""
import ctypes as C

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


def test_buckets_are_powers_of_two_and_num_envs():
    assert rollout._buckets(1) == [1]
    assert rollout._buckets(5) == [1, 2, 4, 5]
    assert rollout._buckets(32) == [1, 2, 4, 8, 16, 32]
    assert rollout._buckets(33) == [1, 2, 4, 8, 16, 32, 33]


@pytest.mark.parametrize("sampler", ["lms", "euler_ancestral", "ancestral", "dpmpp_2s_ancestral", "dpmpp_2m_sde", "dpm_fast", "nope"])
def test_unsupported_samplers_are_refused_by_name(sampler):
    den, cfg = _den()
    with pytest.raises(ValueError, match="deterministic fused samplers"):
        rollout.VectorEnvPolicy(den, 4, sampler_type=sampler, act_window_size=cfg.action_seq_len, action_dim=cfg.action_dim)


def test_constructor_validation():
    den, cfg = _den()
    kw = dict(act_window_size=cfg.action_seq_len, action_dim=cfg.action_dim)
    with pytest.raises(ValueError, match="extra_args"):
        rollout.VectorEnvPolicy(den, 4, extra_args={"s_churn": 0.1}, **kw)
    import torch
    with pytest.raises(ValueError, match="generator"):
        rollout.VectorEnvPolicy(den, 4, generator=torch.Generator(), **kw)
    with pytest.raises(ValueError, match="num_envs"):
        rollout.VectorEnvPolicy(den, 0, **kw)
    with pytest.raises(ValueError, match="num_envs"):
        rollout.VectorEnvPolicy(den, L.MODE_ENV_MAX + 1, **kw)
    with pytest.raises(ValueError, match="GCDenoiser"):
        rollout.VectorEnvPolicy(lambda *a: None, 4, **kw)
    with pytest.raises(ValueError, match="ROCm device"):                     # the parameters are on the host here
        rollout.VectorEnvPolicy(den, 4, **kw)


def test_env_pool_abi():
    lib = L.load()
    assert L.ABI_VERSION == 13 and lib.mode_hip_version() == 13
    assert lib.mode_hip_sizeof(b"ModeEnvPoolDesc") == C.sizeof(L.ModeEnvPoolDesc)
    d = L.ModeEnvPoolDesc(num_envs=0, W=10, A=7, multistep=10)
    assert lib.mode_env_commit_emit(C.byref(d), None) == -1                   # bad-arg paths: refused before any launch
    d = L.ModeEnvPoolDesc(num_envs=4, W=10, A=7, multistep=11, plan=16, counter=16, draws=16, out=16)
    assert lib.mode_env_commit_emit(C.byref(d), None) == -1                   # multistep > W
    assert lib.mode_env_gather_noise(None, 4, 4, None, None, None, 0, None, 0, None, None, None, 70, 1.0, None) == -1
