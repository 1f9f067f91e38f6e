"""The rollout policies fed the cameras' own uint8 frames (camera_transforms=) on the MI355X: the tiny denoiser and the two FiLM-ResNet-18
encoders of tests/test_gpu_vector_env_frames.py at 64 x 64, from 48 x 40 and 20 x 20 uint8 sources.  A policy with camera_transforms and one
without, fed ``preprocess_cameras`` of the same frames, must emit the same bits: the only difference is where the transform ran."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import mode_diffusion_policy_amd as M  # noqa: E402
from mode_diffusion_policy_amd import _lib as L  # noqa: E402
from mode_diffusion_policy_amd import rollout  # noqa: E402

from test_gpu_vector_env import SIGMA_MAX, build  # noqa: E402
from test_gpu_vector_env_frames import encoders  # noqa: E402

SRC_S, SRC_G, OUT = (48, 40), (20, 20), (64, 64)
T_S = M.CameraTransform(OUT)
T_G = M.CameraTransform(OUT, mean=(0.5, 0.4, 0.3), std=(0.2, 0.25, 0.3))
TRANSFORMS = {"rgb_static": T_S, "rgb_gripper": T_G}


def u8_frames(cfg, n, seed):
    g = torch.Generator().manual_seed(seed)
    obs = {"rgb_obs": {"rgb_static": torch.randint(0, 256, (n, 1, *SRC_S, 3), dtype=torch.uint8, generator=g).cuda(),
                       "rgb_gripper": torch.randint(0, 256, (n, 1, *SRC_G, 3), dtype=torch.uint8, generator=g).cuda()}}
    return obs, torch.randn(n, cfg.goal_dim, generator=g).cuda()


def as_float(obs):
    """What a user of a policy without camera_transforms feeds it: the transform's fp32 output."""
    s, g = M.preprocess_cameras(obs["rgb_obs"]["rgb_static"], obs["rgb_obs"]["rgb_gripper"], T_S, T_G)
    return {"rgb_obs": {"rgb_static": s, "rgb_gripper": g}}


def vector(den, cfg, encs, n, transforms, **kw):
    return rollout.VectorEnvPolicy(den, n, act_window_size=cfg.action_seq_len, action_dim=cfg.action_dim, sigma_max=SIGMA_MAX,
                                   static_resnet=encs[0], gripper_resnet=encs[1], camera_transforms=transforms, **kw)


@pytest.mark.parametrize("autocast", [torch.bfloat16, None], ids=["bf16-encoders", "fp32-encoders"])
def test_vector_policy_with_transforms_equals_policy_fed_preprocessed_frames(autocast):
    cfg, m, den = build("noise", "bf16")
    encs = encoders(cfg)
    n = 4
    pu = vector(den, cfg, encs, n, TRANSFORMS, multistep=2, encoder_autocast=autocast)
    pf = vector(den, cfg, encs, n, None, multistep=2, encoder_autocast=autocast)
    # staggered: env 2 starts late, envs 1 and 3 are reset before the third step
    bits = torch.int16 if autocast == torch.bfloat16 else torch.int32
    active = [np.array([True, True, False, True]), np.array([True, False, True, True]), np.array([True, True, True, False])]
    replans = 0
    for t in range(3):
        obs, goal = u8_frames(cfg, n, 50 + t)
        if t == 2:
            pu.reset(envs=[1, 3], seeds=[91, 93]); pf.reset(envs=[1, 3], seeds=[91, 93])
        a = pu.step(obs, goal, active=active[t])
        b = pf.step(as_float(obs), goal, active=active[t])
        assert pu.replanned == pf.replanned
        replans += len(pu.replanned)
        mb = next(k for k in (1, 2, 4) if k >= len(pu.replanned))
        for k in (0, 1):                                                         # what the towers read: the same bits on both routes
            assert torch.equal(pu._enc_store[mb]["bufs"][k].view(bits), pf._enc_store[mb]["bufs"][k].view(bits)), (t, k)
        gap = float((a - b).norm() / b.norm())
        print(f"step {t}: {len(pu.replanned)} replans, relative gap of the actions {gap:.3e}")
        # bf16 towers (the policies' default) repeat bit for bit across the two policies' captures, so the actions must too; the fp32 towers'
        # convolutions come from the library, whose choice per capture does not (measured gap of the actions here: 1e-3 .. 3e-3 with identical
        # encoder inputs) - there the identical inputs above are what the transform's placement can guarantee
        if autocast == torch.bfloat16:
            assert torch.equal(a, b), t
            assert torch.equal(pu.plans, pf.plans), t
        assert torch.isfinite(a).all()
    assert replans >= 6
    st = pu._enc_store[4]
    assert st["bufs"][0].shape == (4, 1, 3, *OUT) and st["bufs"][0].dtype == (torch.bfloat16 if autocast == torch.bfloat16 else torch.float32)
    assert st["geom"][0][0] == (1, *SRC_S, 3) and st["geom"][1][0] == (1, *SRC_G, 3)          # the key holds the source H, W


def test_chunked_policy_with_transforms_equals_policy_fed_preprocessed_frames():
    cfg, m, den = build("noise", "bf16")
    encs = encoders(cfg)
    n = 3
    mk = lambda tr: rollout.ChunkedRolloutPolicy(den, act_window_size=cfg.action_seq_len, action_dim=cfg.action_dim, sigma_max=SIGMA_MAX, multistep=2,
                                                 static_resnet=encs[0], gripper_resnet=encs[1], camera_transforms=tr,
                                                 generator=torch.Generator(device="cuda").manual_seed(3))
    pu, pf = mk(TRANSFORMS), mk(None)
    for t in range(4):
        obs, goal = u8_frames(cfg, n, 60 + t)
        if t == 3:
            pu.reset(); pf.reset()
        a, b = pu.step(obs, goal), pf.step(as_float(obs), goal)
        assert torch.equal(a, b) and torch.equal(pu.pred_action_seq, pf.pred_action_seq), t
    (ent,) = pu.encoders._graphs.values()                                        # one graph entry, keyed and shaped by the transformed frames
    assert ent["s"].shape == (n, 1, 3, *OUT) and ent["s"].dtype == torch.bfloat16
    with pytest.raises(ValueError, match="camera's uint8"):
        pu.embed(as_float(obs), goal)


def test_rows_that_do_not_replan_are_not_read():
    cfg, m, den = build("noise", "bf16")
    encs = encoders(cfg)
    n = 6
    obs, goal = u8_frames(cfg, n, 70)
    envs = [1, 2, 4]
    act = np.zeros(n, dtype=bool)
    act[envs] = True
    poisoned = {"rgb_obs": {k: v.clone() for k, v in obs["rgb_obs"].items()}}
    for v in poisoned["rgb_obs"].values():
        for b in range(n):
            if b not in envs:
                v[b] = 255 - v[b]                                                # another image in every row that does not replan
    plans = []
    for o in (obs, poisoned):
        pol = vector(den, cfg, encs, n, TRANSFORMS)
        out = pol.step(o, goal, active=act)
        assert pol.replanned == envs
        plans.append((pol.plans[envs].clone(), out.clone()))
    assert torch.equal(plans[0][0], plans[1][0]) and torch.equal(plans[0][1], plans[1][1])
    other = vector(den, cfg, encs, n, TRANSFORMS)                                # (and the frames do matter)
    moved = {"rgb_obs": {k: v.clone() for k, v in obs["rgb_obs"].items()}}
    moved["rgb_obs"]["rgb_static"][2] = 255 - moved["rgb_obs"]["rgb_static"][2]
    other.step(moved, goal, active=act)
    assert not torch.equal(other.plans[2], plans[0][0][1]) and torch.equal(other.plans[1], plans[0][0][0])


def test_launch_and_replay_budget_equals_the_float_frame_policy(monkeypatch):
    cfg, m, den = build("noise", "bf16")
    _, _, den2 = build("noise", "bf16")                                          # (a denoiser each: a policy's warm-up renews its model's routing cache)
    encs = encoders(cfg)
    n = 4
    obs, goal = u8_frames(cfg, n, 80)
    pols = {"u8": (vector(den, cfg, encs, n, TRANSFORMS), obs), "float": (vector(den2, cfg, encs, n, None), as_float(obs))}
    for pol, o in pols.values():
        pol.warmup(o, goal)
    cnt = {"capture": 0, "replay": 0, "launch": []}
    cap, rep, chk = torch.cuda.CUDAGraph.capture_begin, torch.cuda.CUDAGraph.replay, L.check

    def counted_capture(self, *a, **k):
        cnt["capture"] += 1
        return cap(self, *a, **k)

    def counted_replay(self):
        cnt["replay"] += 1
        return rep(self)

    def counted_check(rc, what=""):                                              # every launch outside a graph returns through _lib.check
        cnt["launch"].append(what)
        return chk(rc, what)
    monkeypatch.setattr(torch.cuda.CUDAGraph, "capture_begin", counted_capture)
    monkeypatch.setattr(torch.cuda.CUDAGraph, "replay", counted_replay)
    monkeypatch.setattr(L, "check", counted_check)
    seen = {}
    for name, (pol, o) in pols.items():
        per_step = []
        for size in (1, 3, 2, 4):
            act = np.zeros(n, dtype=bool)
            act[:size] = True
            pol.reset(envs=list(range(size)))
            r0, l0 = cnt["replay"], len(cnt["launch"])
            pol.step(o, goal, active=act)
            assert pol.replanned == list(range(size))
            per_step.append((cnt["replay"] - r0, len(cnt["launch"]) - l0))
        seen[name] = per_step
    torch.cuda.synchronize()
    assert cnt["capture"] == 0
    assert seen["u8"] == seen["float"] == [(2, 2)] * 4, seen                     # two launches and two replays per replanning step
    assert cnt["launch"].count("frames_preprocess") == 4 and cnt["launch"].count("env_gather_frames") == 4


def test_eager_encoders_use_the_same_kernel(monkeypatch):
    cfg, m, den = build("noise", "bf16")
    encs = encoders(cfg)
    n = 4
    obs, goal = u8_frames(cfg, n, 90)
    act = np.array([True, False, True, True])
    graphed = vector(den, cfg, encs, n, TRANSFORMS)
    graphed.step(obs, goal, active=act)
    chunked = rollout.ChunkedRolloutPolicy(den, act_window_size=cfg.action_seq_len, action_dim=cfg.action_dim, sigma_max=SIGMA_MAX,
                                           static_resnet=encs[0], gripper_resnet=encs[1], camera_transforms=TRANSFORMS)
    tok_graphed = chunked.embed(obs, goal)["state_images"].clone()
    monkeypatch.setenv("MODE_HIP_GRAPH", "0")
    eager = vector(den, cfg, encs, n, TRANSFORMS)
    eager.step(obs, goal, active=act)
    assert eager._enc_store[4]["graph"] is None
    assert torch.equal(eager.plans, graphed.plans)
    assert torch.equal(chunked.embed(obs, goal)["state_images"], tok_graphed)
