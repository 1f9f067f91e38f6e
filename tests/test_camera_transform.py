"""CPU: the host-side contract of the camera transform - the ABI surface of mode_frames_preprocess (struct sizes, every refusal before any
launch), the validation of camera.CameraTransform and of the policies' camera_transforms=, and which frames a policy takes with and without it."""
import ctypes as C
from types import SimpleNamespace

import pytest
import torch

import mode_diffusion_policy_amd as M
from mode_diffusion_policy_amd import _lib as L
from mode_diffusion_policy_amd import camera, rollout

N, G = 3, 6


def test_struct_sizes_and_abi():
    lib = L.load()
    assert L.ABI_VERSION == 13 and lib.mode_hip_version() == 13                          # an addition, not a new ABI
    assert lib.mode_hip_sizeof(b"ModeFramePrepCam") == C.sizeof(L.ModeFramePrepCam) > 0
    assert lib.mode_hip_sizeof(b"ModeFramePrepDesc") == C.sizeof(L.ModeFramePrepDesc) > 0


def _cam(**kw):
    base = dict(src=64, src_stride=2 * 10 * 12 * 3, dst=64, shifts=None, T=2, H=10, W=12, OH=8, OW=16, dst_dtype=L.MODE_BF16, pad=0)
    base.update(kw)
    c = L.ModeFramePrepCam(**base)
    for i in range(3):
        c.mean[i], c.inv_std[i] = 0.5, 2.0
    return c


def test_entry_point_refusals_without_a_device():
    """Every refusal returns before any launch: the pointers here are not device memory."""
    lib = L.load()
    ok = L.ModeFramePrepDesc(rows=64, m_b=2, num_envs=3)
    ok.cam[0] = _cam()
    assert lib.mode_frames_preprocess(None, None) == -1
    for bad in (dict(m_b=0), dict(m_b=65536), dict(num_envs=0), dict(rows=None, m_b=4)):      # (rows NULL needs m_b <= num_envs)
        d = L.ModeFramePrepDesc.from_buffer_copy(ok)
        for k, v in bad.items():
            setattr(d, k, v)
        assert lib.mode_frames_preprocess(C.byref(d), None) == -1, bad
    for bad, rc in ((dict(src=None), -1), (dict(dst=None), -1), (dict(src_stride=2 * 10 * 12 * 3 - 1), -1), (dict(pad=-1), -1), (dict(T=0), -1),
                    (dict(H=0), -1), (dict(OW=-4), -1), (dict(dst=65), -1), (dict(shifts=66), -1),
                    (dict(H=801, OH=100, src_stride=2 * 801 * 12 * 3), -2),               # ratio 8.01
                    (dict(W=129, src_stride=2 * 10 * 129 * 3), -2),                       # 129 / 16 > 8
                    (dict(dst_dtype=7), -2),
                    (dict(T=1, H=2, W=2400, OH=2, OW=2400, src_stride=2 * 2400 * 3), -2)):    # one output row's working set > 64 KiB of LDS
        for slot in (0, 1):
            d = L.ModeFramePrepDesc.from_buffer_copy(ok)
            d.cam[slot] = _cam(**bad)
            assert lib.mode_frames_preprocess(C.byref(d), None) == rc, (bad, slot)
    d = L.ModeFramePrepDesc(rows=64, m_b=2, num_envs=3)                                   # no camera at all
    assert lib.mode_frames_preprocess(C.byref(d), None) == -1
    d = L.ModeFramePrepDesc.from_buffer_copy(ok)
    d.cam[0] = _cam(T=40000, src_stride=40000 * 10 * 12 * 3)                              # m_b * T frames > 65535
    assert lib.mode_frames_preprocess(C.byref(d), None) == -2


def test_camera_transform_validation():
    t = M.CameraTransform()
    assert t.size == (224, 224) and t.mean == camera.CLIP_MEAN and t.std == camera.CLIP_STD and t.shift_pad == 0
    assert M.CameraTransform(64).size == (64, 64) and M.CameraTransform((48, 40), shift_pad=4).shift_pad == 4
    assert t.out_shape((5, 2, 200, 200, 3)) == (5, 2, 3, 224, 224) and t.out_shape((5, 84, 84, 3)) == (5, 3, 224, 224)
    for bad in (dict(size=0), dict(size=(224,)), dict(size=(224, -1)), dict(size="big"), dict(mean=(0.5, 0.5)), dict(mean=(0.5, 0.5, float("nan"))),
                dict(std=(1.0, 0.0, 1.0)), dict(std=(1.0, -1.0, 1.0)), dict(std=None), dict(shift_pad=-1), dict(shift_pad=1.5), dict(shift_pad=True)):
        with pytest.raises(ValueError):
            M.CameraTransform(**bad)
    with pytest.raises(ValueError, match="more than 8"):
        M.CameraTransform(16).check_source(136, 16)
    M.CameraTransform(16).check_source(128, 128)


def test_draw_shifts_is_the_reference_draw():
    t = M.CameraTransform(16, shift_pad=3)
    s = t.draw_shifts(500, "cpu", torch.Generator().manual_seed(5))
    assert s.dtype == torch.int32 and s.shape == (500, 2) and int(s.min()) == 0 and int(s.max()) == 6
    want = torch.randint(0, 7, (500, 2), dtype=torch.int32, generator=torch.Generator().manual_seed(5))
    assert torch.equal(s, want)
    assert not M.CameraTransform(16).draw_shifts(9, "cpu").any()


def test_frames_contract_of_the_transform():
    t = M.CameraTransform(16)
    for bad, match in ((torch.zeros(2, 8, 8, 3), "uint8"), (torch.zeros(2, 3, 8, 8, dtype=torch.uint8), "camera frames"),
                       (torch.zeros(8, 8, 3, dtype=torch.uint8), "camera frames"), (torch.zeros(2, 8, 8, 3, dtype=torch.uint8), "ROCm device")):
        with pytest.raises(ValueError, match=match):
            t(bad)
    with pytest.raises(ValueError, match="dtype"):
        t(torch.zeros(2, 8, 8, 3, dtype=torch.uint8), dtype=torch.float16)
    with pytest.raises(ValueError, match="no camera"):
        M.preprocess_cameras(None, None, t, t)
    wide = torch.zeros(4, 2, 8, 8, 3, dtype=torch.uint8)[:, :1]                           # rows at a wider pitch are taken as they lie
    assert camera.check_frames_u8(wide) is wide
    tr = torch.zeros(4, 1, 8, 3, 8, dtype=torch.uint8).transpose(3, 4)
    assert camera.check_frames_u8(tr).is_contiguous()


def test_camera_transforms_argument_is_validated_in_the_constructor():
    t = M.CameraTransform(16)
    enc = object()
    for cls in (rollout.ChunkedRolloutPolicy, rollout.VectorEnvPolicy):
        extra = dict(num_envs=2) if cls is rollout.VectorEnvPolicy else {}
        with pytest.raises(ValueError, match="exactly the keys"):
            cls(None, static_resnet=enc, gripper_resnet=enc, camera_transforms={"rgb_static": t}, **extra)
        with pytest.raises(ValueError, match="exactly the keys"):
            cls(None, static_resnet=enc, gripper_resnet=enc, camera_transforms={"rgb_static": t, "rgb_gripper": t, "rgb_tactile": t}, **extra)
        with pytest.raises(ValueError, match="exactly the keys"):
            cls(None, static_resnet=enc, gripper_resnet=enc, camera_transforms=[t, t], **extra)
        with pytest.raises(ValueError, match="must be a CameraTransform"):
            cls(None, static_resnet=enc, gripper_resnet=enc, camera_transforms={"rgb_static": t, "rgb_gripper": (16, 16)}, **extra)
        with pytest.raises(ValueError, match="perceptual encoders"):
            cls(None, camera_transforms={"rgb_static": t, "rgb_gripper": t}, **extra)


def _policy(transforms, n_img=2):
    """The attributes the input check reads, without a device (a VectorEnvPolicy needs a ROCm device to be constructed)."""
    pol = object.__new__(rollout.VectorEnvPolicy)
    pol.num_envs = N
    pol.model = SimpleNamespace(inner_model=SimpleNamespace(n_img_tokens=n_img, obs_dim=8, goal_dim=G))
    pol.encoders = object()
    pol._plan = torch.zeros(N, 1, 1)
    pol.camera_transforms = transforms
    return pol


def _u8(T=1, n=N, hs=(12, 10), hg=(6, 6)):
    return {"rgb_obs": {"rgb_static": torch.zeros(n, T, *hs, 3, dtype=torch.uint8), "rgb_gripper": torch.zeros(n, T, *hg, 3, dtype=torch.uint8)}}


def test_policy_with_transforms_takes_uint8_and_refuses_float_frames():
    t = {"rgb_static": M.CameraTransform(8), "rgb_gripper": M.CameraTransform((8, 4))}
    pol = _policy(t)
    obs = _u8()
    img, gl, frames = pol._check_inputs(obs, torch.zeros(N, G))
    assert img is None and frames[0] is obs["rgb_obs"]["rgb_static"] and frames[1] is obs["rgb_obs"]["rgb_gripper"]
    for dt in (torch.float32, torch.bfloat16):
        bad = {"rgb_obs": {"rgb_static": torch.zeros(N, 1, 3, 8, 8, dtype=dt), "rgb_gripper": torch.zeros(N, 1, 3, 8, 8, dtype=dt)}}
        with pytest.raises(ValueError, match="built with camera_transforms takes the camera's uint8"):
            pol._check_inputs(bad, torch.zeros(N, G))
    for mutate, match in ((lambda r: r.pop("rgb_gripper"), "cameras"),
                          (lambda r: r.update(rgb_static=torch.zeros(N + 1, 1, 12, 10, 3, dtype=torch.uint8)), "one row per environment"),
                          (lambda r: r.update(rgb_static=torch.zeros(N, 12, 10, 3, dtype=torch.uint8)), "one row per environment"),
                          (lambda r: r.update(rgb_gripper=torch.zeros(N, 1, 3, 6, 6, dtype=torch.uint8)), "camera frames"),
                          (lambda r: r.update(rgb_gripper=torch.zeros(N, 2, 6, 6, 3, dtype=torch.uint8)), "same rows and number of frames"),
                          (lambda r: r.update(rgb_static=torch.zeros(N, 1, 65, 10, 3, dtype=torch.uint8)), "more than 8"),
                          (lambda r: r.update(rgb_static=torch.zeros(N, 1, 12, 10, 3, dtype=torch.uint8, device="meta")), "must be on")):
        obs = _u8()
        mutate(obs["rgb_obs"])
        with pytest.raises(ValueError, match=match):
            pol._check_inputs(obs, torch.zeros(N, G))
    with pytest.raises(ValueError, match="n_img_tokens"):
        pol._check_inputs(_u8(T=2), torch.zeros(N, G))
    assert _policy(t, n_img=4)._check_inputs(_u8(T=2), torch.zeros(N, G))[2][0].shape[1] == 2


def test_policy_without_transforms_still_refuses_uint8():
    pol = _policy(None)
    with pytest.raises(ValueError, match="float32 or bfloat16"):
        pol._check_inputs({"rgb_obs": {"rgb_static": torch.zeros(N, 1, 3, 8, 8, dtype=torch.uint8), "rgb_gripper": torch.zeros(N, 1, 3, 6, 6)}}, torch.zeros(N, G))
    with pytest.raises(ValueError):
        pol._check_inputs(_u8(), torch.zeros(N, G))                                        # HWC uint8 is not a float (n, T, 3, H, W) frame either
    ok = {"rgb_obs": {"rgb_static": torch.zeros(N, 1, 3, 8, 8), "rgb_gripper": torch.zeros(N, 1, 3, 6, 6)}}
    assert pol._check_inputs(ok, torch.zeros(N, G))[2][0] is ok["rgb_obs"]["rgb_static"]
