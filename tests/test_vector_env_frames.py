"""CPU: the host-side contract of rollout.VectorEnvPolicy's raw-frame input (every refusal happens on host metadata, before any launch) and the
ABI 13 surface of the frame gather it binds."""
import ctypes as C
from types import SimpleNamespace

import pytest
import torch

from mode_diffusion_policy_amd import _lib as L
from mode_diffusion_policy_amd import rollout

N, G = 3, 6


def _policy(encoders=True, n_img=2):
    """The attributes the input check reads, without a device: a VectorEnvPolicy needs a ROCm device to be constructed."""
    pol = object.__new__(rollout.VectorEnvPolicy)
    pol.num_envs = N
    pol.model = SimpleNamespace(inner_model=SimpleNamespace(n_img_tokens=n_img, obs_dim=8, goal_dim=G))
    pol.encoders = object() if encoders else None
    pol._plan = torch.zeros(N, 1, 1)
    return pol


def _frames(T=1, dtype=torch.float32, n=N, hs=8, hg=6):
    return {"rgb_obs": {"rgb_static": torch.zeros(n, T, 3, hs, hs, dtype=dtype), "rgb_gripper": torch.zeros(n, T, 3, hg, hg, dtype=dtype)}}


def test_frames_are_accepted_and_passed_through():
    pol = _policy()
    obs = _frames()
    img, gl, frames = pol._check_inputs(obs, torch.zeros(N, G))
    assert img is None and frames[0] is obs["rgb_obs"]["rgb_static"] and frames[1] is obs["rgb_obs"]["rgb_gripper"]
    img, gl, frames = pol._check_inputs(_frames(dtype=torch.bfloat16), torch.zeros(N, 1, G))
    assert frames[0].dtype == torch.bfloat16
    # environments at a wider pitch are taken as they lie; a non-contiguous environment block is made contiguous
    wide = torch.zeros(N, 2, 3, 8, 8)[:, :1]
    obs = _frames()
    obs["rgb_obs"]["rgb_static"] = wide
    assert pol._check_inputs(obs, torch.zeros(N, G))[2][0] is wide
    obs["rgb_obs"]["rgb_static"] = torch.zeros(N, 1, 3, 8, 8).transpose(3, 4)
    f = pol._check_inputs(obs, torch.zeros(N, G))[2][0]
    assert f.is_contiguous() and f.shape == (N, 1, 3, 8, 8)
    img, _, frames = pol._check_inputs({"state_images": torch.zeros(N, 2, 8)}, torch.zeros(N, G))
    assert frames is None and img.shape == (N, 2, 8)


def test_without_encoders_raw_frames_are_refused():
    with pytest.raises(ValueError, match="embed raw camera"):
        _policy(encoders=False)._check_inputs(_frames(), torch.zeros(N, G))
    with pytest.raises(ValueError, match="embed raw camera"):
        _policy()._check_inputs({}, torch.zeros(N, G))


def test_mixed_inputs_are_refused():
    obs = _frames()
    obs["state_images"] = torch.zeros(N, 2, 8)
    with pytest.raises(ValueError, match="not both"):
        _policy()._check_inputs(obs, torch.zeros(N, G))


def _bad(mutate, match, **kw):
    obs = _frames(**kw)
    mutate(obs["rgb_obs"])
    with pytest.raises(ValueError, match=match):
        _policy()._check_inputs(obs, torch.zeros(N, G))


def test_camera_keys():
    _bad(lambda r: r.pop("rgb_gripper"), "cameras")
    _bad(lambda r: r.update(rgb_extra=torch.zeros(N, 1, 3, 4, 4)), "cameras")
    with pytest.raises(ValueError, match="cameras"):
        _policy()._check_inputs({"rgb_obs": [torch.zeros(1)]}, torch.zeros(N, G))


def test_shapes_and_rows():
    _bad(lambda r: r.update(rgb_static=torch.zeros(N + 1, 1, 3, 8, 8)), "one row per environment")
    _bad(lambda r: r.update(rgb_static=torch.zeros(N, 3, 8, 8)), r"\(3, T, 3, H, W\)")
    _bad(lambda r: r.update(rgb_gripper=torch.zeros(N, 1, 4, 8, 8)), "rgb_gripper")
    _bad(lambda r: r.update(rgb_gripper=[0]), "rgb_gripper")


def test_frame_count_T():
    _bad(lambda r: r.update(rgb_gripper=torch.zeros(N, 2, 3, 6, 6)), "same number of frames")
    obs = _frames(T=2)                                                          # 2 T = 4 != n_img_tokens = 2
    with pytest.raises(ValueError, match="n_img_tokens"):
        _policy()._check_inputs(obs, torch.zeros(N, G))
    assert _policy(n_img=4)._check_inputs(obs, torch.zeros(N, G))[2][0].shape[1] == 2


def test_dtype_and_device():
    _bad(lambda r: r.update(rgb_static=r["rgb_static"].half()), "float32 or bfloat16")
    _bad(lambda r: r.update(rgb_gripper=r["rgb_gripper"].to(torch.uint8)), "float32 or bfloat16")
    _bad(lambda r: r.update(rgb_static=torch.zeros(N, 1, 3, 8, 8, device="meta")), "must be on")
    with pytest.raises(ValueError, match="latent_goal"):
        _policy()._check_inputs(_frames(), torch.zeros(N + 1, G))


def test_frame_gather_abi():
    lib = L.load()
    assert L.ABI_VERSION == 13 and lib.mode_hip_version() == 13
    assert lib.mode_hip_sizeof(b"ModeEnvFramesDesc") == C.sizeof(L.ModeEnvFramesDesc)
    assert lib.mode_hip_sizeof(b"ModeEnvFramesCam") == C.sizeof(L.ModeEnvFramesCam)
    cam = dict(src=64, src_stride=12, row_elems=12, dst=64, src_dtype=L.MODE_F32, dst_dtype=L.MODE_BF16)
    ok = L.ModeEnvFramesDesc(rows=64, m_b=2, num_envs=3)
    ok.cam[0] = L.ModeEnvFramesCam(**cam)
    for bad in (dict(rows=None), dict(m_b=0), dict(num_envs=0), dict(m_b=65536)):                # refused before any launch
        d = L.ModeEnvFramesDesc.from_buffer_copy(ok)
        for k, v in bad.items():
            setattr(d, k, v)
        assert lib.mode_env_gather_frames(C.byref(d), None) == -1, bad
    for bad, rc in ((dict(src_stride=11), -1), (dict(row_elems=0), -1), (dict(dst=None), -1), (dict(src=66), -1),
                    (dict(src_dtype=L.MODE_BF16, dst_dtype=L.MODE_F32), -2), (dict(dst_dtype=7), -2)):
        d = L.ModeEnvFramesDesc.from_buffer_copy(ok)
        d.cam[1] = L.ModeEnvFramesCam(**{**cam, **bad})
        assert lib.mode_env_gather_frames(C.byref(d), None) == rc, bad
    d = L.ModeEnvFramesDesc(rows=64, m_b=2, num_envs=3)                                            # no camera at all
    assert lib.mode_env_gather_frames(C.byref(d), None) == -1
