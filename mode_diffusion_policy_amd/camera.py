"""Camera frames as an environment delivers them -> the perceptual encoders' input, on the device in one launch.

A CALVIN / LIBERO environment or a real camera hands over ``uint8 (H, W, 3)`` frames at its own resolution; the reference agent puts
``Resize -> (RandomShiftsAug when training) -> ScaleImageTensor -> Normalize`` between them and the encoders.  ``CameraTransform`` is that
sequence as one HIP kernel (csrc/frame_prep.hip; the semantics, element by element, are the comment of ``mode_frames_preprocess`` in
include/mode_hip.h): antialiased bilinear resize, quantisation to uint8 levels, an integer shift of the edge-replicated image, ``/ 255``,
``(x - mean) / std``, stored as the NCHW fp32 / bf16 tensor the stem reads.  ``preprocess_cameras`` runs both cameras in the same launch; the
rollout policies (``camera_transforms=``) call it with their replanning rows, so a frame is read as the camera's bytes and written once.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence, Tuple

import numpy as np
import torch

CLIP_MEAN = (0.48145466, 0.4578275, 0.40821073)
CLIP_STD = (0.26862954, 0.26130258, 0.27577711)
_DTYPES = (torch.float32, torch.bfloat16)
MAX_RATIO = 8          # in / out per axis, the kernel's limit


class CameraTransform:
    """One camera's transform: ``size = (OH, OW)`` of the encoder input, per-channel ``mean`` / ``std`` of the normalisation (of the image scaled
    to [0, 1]), ``shift_pad`` the pad of the random shift (0 = none; shifts are given per call, see ``draw_shifts``).  Plain values, validated here.

    ``t(frames_u8, shifts=None, out=None, dtype=torch.float32)``: ``frames_u8`` uint8 ``(B, H, W, 3)`` or ``(B, T, H, W, 3)`` on a ROCm device; the
    rows (dim 0) may lie at any pitch, everything inside a row must be contiguous.  Returns ``(B, [T,] 3, OH, OW)`` in ``dtype`` (or writes the
    contiguous ``out`` and returns it).  ``shifts``: int32 ``(B [* T], 2)`` device tensor of ``(sx, sy)`` per frame, each in ``[0, 2 shift_pad]``
    (out-of-range values are clamped on the device); ``shift_pad`` is the unshifted crop.  The inputs are integers: there is no autograd."""

    def __init__(self, size=(224, 224), mean: Sequence[float] = CLIP_MEAN, std: Sequence[float] = CLIP_STD, shift_pad: int = 0):
        if isinstance(size, (int, np.integer)) and not isinstance(size, bool):
            size = (int(size), int(size))
        try:
            size = tuple(int(v) for v in size)
            ok = len(size) == 2 and all(v > 0 for v in size)
        except (TypeError, ValueError):
            ok = False
        if not ok:
            raise ValueError(f"size must be a positive int or (OH, OW), got {size!r}")
        vals = []
        for name, v in (("mean", mean), ("std", std)):
            try:
                v = tuple(float(x) for x in v)
            except (TypeError, ValueError):
                v = ()
            if len(v) != 3 or not all(np.isfinite(v)):
                raise ValueError(f"{name} must be three finite floats (one per channel), got {mean if name == 'mean' else std!r}")
            vals.append(v)
        if not all(s > 0 for s in vals[1]):
            raise ValueError(f"std must be positive, got {vals[1]!r}")
        if isinstance(shift_pad, bool) or not isinstance(shift_pad, (int, np.integer)) or shift_pad < 0:
            raise ValueError(f"shift_pad must be an int >= 0, got {shift_pad!r}")
        self.size, self.mean, self.std, self.shift_pad = size, vals[0], vals[1], int(shift_pad)

    def __repr__(self):
        return f"CameraTransform(size={self.size}, mean={self.mean}, std={self.std}, shift_pad={self.shift_pad})"

    def out_shape(self, frames_shape) -> Tuple[int, ...]:
        """Shape of the transformed frames for ``frames_u8`` of ``frames_shape`` ((B, [T,] H, W, 3))."""
        return tuple(frames_shape[:-3]) + (3,) + self.size

    def check_source(self, H: int, W: int, name: str = "frames") -> None:
        """The kernel's geometry limit, on host metadata: at most ``MAX_RATIO`` source pixels per output pixel on either axis."""
        if H > MAX_RATIO * self.size[0] or W > MAX_RATIO * self.size[1]:
            raise ValueError(f"{name}: {H} x {W} -> {self.size[0]} x {self.size[1]} shrinks an axis by more than {MAX_RATIO}")

    def draw_shifts(self, n_frames: int, device, generator: Optional[torch.Generator] = None) -> torch.Tensor:
        """``RandomShiftsAug``'s draw, one per frame: int32 ``(n_frames, 2)`` uniform on ``{0, ..., 2 shift_pad}``."""
        return torch.randint(0, 2 * self.shift_pad + 1, (int(n_frames), 2), dtype=torch.int32, device=device, generator=generator)

    def __call__(self, frames_u8, shifts=None, out=None, dtype=torch.float32):
        return _run([(self, frames_u8, shifts, out)], dtype)[0]


def check_frames_u8(f, name: str = "frames", device=None) -> torch.Tensor:
    """``f`` as the kernel reads it: uint8 (B, H, W, 3) or (B, T, H, W, 3), non-empty, each row one contiguous block (made so otherwise)."""
    if not torch.is_tensor(f) or f.dim() not in (4, 5) or f.shape[-1] != 3 or f.numel() == 0:
        raise ValueError(f"{name} must be uint8 (B, H, W, 3) or (B, T, H, W, 3) camera frames, got {tuple(getattr(f, 'shape', ()))}")
    if f.dtype != torch.uint8:
        raise ValueError(f"{name} must be uint8 camera frames (H, W, 3 last), got {f.dtype}")
    if device is not None and f.device != torch.device(device):
        raise ValueError(f"{name} must be on {device}, got {f.device}")
    if not (f[0].is_contiguous() and (f.shape[0] == 1 or f.stride(0) >= f[0].numel())):
        f = f.contiguous()
    return f


def _cam_desc(L, t: CameraTransform, f: torch.Tensor, dst: torch.Tensor, shifts, m_b: int):
    """One ModeFramePrepCam: ``f`` checked uint8 frames, ``dst`` the contiguous (m_b [* T], 3, OH, OW) output."""
    T = f.shape[1] if f.dim() == 5 else 1
    H, W = f.shape[-3], f.shape[-2]
    t.check_source(H, W)
    if shifts is not None:
        if not torch.is_tensor(shifts) or shifts.dtype != torch.int32 or tuple(shifts.shape) != (m_b * T, 2) or shifts.device != f.device:
            raise ValueError(f"shifts must be an int32 ({m_b * T}, 2) tensor on {f.device} (one (sx, sy) per output frame), got "
                             f"{getattr(shifts, 'dtype', type(shifts).__name__)} {tuple(getattr(shifts, 'shape', ()))}")
        shifts = shifts.contiguous()
    cam = L.ModeFramePrepCam(src=f.data_ptr(), src_stride=f.stride(0) if f.shape[0] > 1 else f[0].numel(), dst=dst.data_ptr(),
                             shifts=None if shifts is None else shifts.data_ptr(), T=T, H=H, W=W, OH=t.size[0], OW=t.size[1],
                             dst_dtype=L.MODE_BF16 if dst.dtype == torch.bfloat16 else L.MODE_F32, pad=t.shift_pad)
    for i in range(3):
        cam.mean[i] = t.mean[i]
        cam.inv_std[i] = 1.0 / t.std[i]
    return cam, shifts


def launch(cams, rows_ptr: Optional[int], m_b: int, num_envs: int) -> None:
    """``mode_frames_preprocess`` on the current stream: ``cams`` = up to two ``(transform, frames_u8 (num_envs, ...), dst, shifts)`` (None = that
    camera is skipped), output row j < m_b from source row ``rows[j]`` (``rows_ptr`` a device int32 pointer; None: j -> j)."""
    from . import _lib as L
    from .engine import _stream
    d = L.ModeFramePrepDesc(rows=rows_ptr, m_b=m_b, num_envs=num_envs)
    keep = []
    dev = None
    for k, cam in enumerate(cams):
        if cam is None:
            continue
        t, f, dst, shifts = cam
        d.cam[k], s = _cam_desc(L, t, f, dst, shifts, m_b)
        keep.append(s)
        dev = f.device
    with torch.cuda.device(dev):
        L.check(L.load().mode_frames_preprocess(C.byref(d), _stream()), "frames_preprocess")


def _run(items, dtype):
    """The public calls: every (transform, frames, shifts, out) of ``items`` that has frames, all rows, one launch."""
    if dtype not in _DTYPES:
        raise ValueError(f"dtype must be torch.float32 or torch.bfloat16, got {dtype}")
    cams, outs, B = [], [], None
    for k, (t, f, shifts, out) in enumerate(items):
        if f is None:
            cams.append(None); outs.append(None)
            continue
        if not isinstance(t, CameraTransform):
            raise ValueError(f"camera {k}: expected a CameraTransform, got {type(t).__name__}")
        f = check_frames_u8(f, f"camera {k}")
        if f.device.type != "cuda":
            raise ValueError(f"camera {k}: the frames must be on a ROCm device (there is no CPU path), got {f.device}")
        if B is not None and f.shape[0] != B:
            raise ValueError(f"both cameras must carry the same number of rows, got {B} and {f.shape[0]}")
        B = f.shape[0]
        shape = t.out_shape(f.shape)
        if out is None:
            out = torch.empty(shape, dtype=dtype, device=f.device)
        elif (not torch.is_tensor(out) or tuple(out.shape) != shape or out.dtype not in _DTYPES or out.device != f.device or not out.is_contiguous()):
            raise ValueError(f"camera {k}: out must be a contiguous float32 / bfloat16 {shape} tensor on {f.device}, got "
                             f"{getattr(out, 'dtype', type(out).__name__)} {tuple(getattr(out, 'shape', ()))}")
        cams.append((t, f, out, shifts)); outs.append(out)
    if B is None:
        raise ValueError("no camera frames given")
    if B > 65535:
        raise ValueError(f"at most 65535 rows per call, got {B}")
    launch(cams, None, B, B)
    return outs


@torch.no_grad()
def preprocess_cameras(static_u8, gripper_u8, t_static: CameraTransform, t_gripper: CameraTransform, shifts=(None, None), out=(None, None),
                       dtype=torch.float32):
    """Both cameras' transforms in ONE launch: ``(static, gripper)`` outputs as ``CameraTransform.__call__`` returns them.  A camera given as
    None is skipped (its output is None).  ``shifts`` / ``out``: one entry per camera."""
    return tuple(_run([(t_static, static_u8, shifts[0], out[0]), (t_gripper, gripper_u8, shifts[1], out[1])], dtype))
