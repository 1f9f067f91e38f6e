"""Episodes held on the device, and the training batch of step ``t`` as a pure function of ``(seed, t)``.

``EpisodeStore`` takes whole episodes (actions, one goal embedding, optionally both cameras' uint8 frames) from the host, and ``finalize()``
uploads them once into flat device buffers.  ``WindowStream.batch(t)`` then draws ``batch_size`` windows of ``window`` consecutive actions in ONE
HIP launch (csrc/data_stream.hip; the expressions, bit for bit, are the comment of ``mode_data_sample_windows`` in include/mode_hip.h), plus one
``mode_frames_preprocess`` launch that reads the drawn frames straight out of the store when it holds cameras.  There is no host work per step,
no host sync and no state: a run resumed at step ``t`` with the same seed and store sees the same windows, noise, sigma uniforms and shifts.

Windows are drawn i.i.d. uniformly over all window starts, WITH replacement - this is not an epoch permutation: within any stretch of steps
some starts repeat and others are not seen.  Reading CALVIN / LIBERO files, goal images and sharding the store across ranks are not part of this
module (rank ``r`` of a data-parallel run may simply use ``seed + 16 * r``: the stream's keys use ``seed .. seed + 3``).
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence

import numpy as np
import torch

from .camera import CameraTransform

MAX_BATCH = 65535          # the kernels' limits (include/mode_hip.h)
MAX_WINDOW_FLOATS = 4096
MAX_GOAL_DIM = 4096
_PADS = ("hold", "none")


def _host(x, name: str) -> np.ndarray:
    """``x`` (numpy array or CPU / device tensor) as a numpy array, dtype kept."""
    if torch.is_tensor(x):
        return x.detach().cpu().numpy()
    if isinstance(x, np.ndarray):
        return x
    raise ValueError(f"{name} must be a numpy array or a torch tensor, got {type(x).__name__}")


class EpisodeStore:
    """``add_episode(actions [L, A] float, goal [G] float, rgb_static=None, rgb_gripper=None)`` with frames uint8 ``[L, H, W, 3]`` /
    ``[L, Hg, Wg, 3]``: either both cameras for every episode or for none, one geometry per camera.  ``finalize(normalize)`` uploads

        actions [S, A] fp32 (S = total steps), ep_begin [E + 1] int32, goals [E, G] fp32, frames_static / frames_gripper [S, H, W, 3] uint8,
        lo / hi / scale [A] fp32 (None without normalisation)

    to ``device``; afterwards the store is read-only.  ``normalize="minmax"``: ``lo`` / ``hi`` per action dimension over all steps,
    ``scale = 2 / (hi - lo)`` computed in fp64 and rounded to fp32, 0 where ``hi == lo`` (such a dimension normalises to -1); ``(lo, hi)``: the
    caller's bounds, same formula; ``None``: the stream returns the stored bits.  Every refusal is a ``ValueError`` raised before anything is
    allocated on the device."""

    def __init__(self, action_dim: int, goal_dim: int, device="cuda"):
        for name, v in (("action_dim", action_dim), ("goal_dim", goal_dim)):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v <= 0:
                raise ValueError(f"{name} must be a positive int, got {v!r}")
        self.action_dim, self.goal_dim, self.device = int(action_dim), int(goal_dim), torch.device(device)
        self._episodes = []                      # host side, until finalize(): (actions fp32, goal fp32, static u8 | None, gripper u8 | None)
        self._steps = 0
        self._cams: Optional[tuple] = None       # None until the first episode: then () or ((H, W), (Hg, Wg))
        self.finalized = False
        self.actions = self.ep_begin = self.goals = self.frames_static = self.frames_gripper = self.lo = self.hi = self.scale = None
        self.lengths: Optional[np.ndarray] = None

    @property
    def num_steps(self) -> int:
        return self._steps

    @property
    def num_episodes(self) -> int:
        return len(self._episodes) if not self.finalized else len(self.lengths)

    @property
    def has_cameras(self) -> bool:
        return bool(self._cams)

    def add_episode(self, actions, goal, rgb_static=None, rgb_gripper=None) -> None:
        if self.finalized:
            raise ValueError("the store is finalized: it is read-only")
        a, g = _host(actions, "actions"), _host(goal, "goal")
        if a.ndim != 2 or a.shape[0] < 1 or a.shape[1] != self.action_dim or not np.issubdtype(a.dtype, np.floating):
            raise ValueError(f"actions must be a float [L >= 1, {self.action_dim}] array, got {a.dtype} {a.shape}")
        if g.shape != (self.goal_dim,) or not np.issubdtype(g.dtype, np.floating):
            raise ValueError(f"goal must be a float [{self.goal_dim}] array, got {g.dtype} {g.shape}")
        with np.errstate(over="ignore"):
            a = np.ascontiguousarray(a, dtype=np.float32)
        if not np.isfinite(a).all():
            raise ValueError("actions hold a non-finite value (or one that overflows fp32)")
        L = a.shape[0]
        if (rgb_static is None) != (rgb_gripper is None):
            raise ValueError("give both cameras' frames or neither")
        cams, frames = (), (None, None)
        if rgb_static is not None:
            frames = tuple(_host(f, n) for f, n in ((rgb_static, "rgb_static"), (rgb_gripper, "rgb_gripper")))
            for f, n in zip(frames, ("rgb_static", "rgb_gripper")):
                if f.dtype != np.uint8 or f.ndim != 4 or f.shape[0] != L or f.shape[3] != 3 or f.shape[1] < 1 or f.shape[2] < 1:
                    raise ValueError(f"{n} must be uint8 [{L}, H, W, 3] frames (one per step), got {f.dtype} {f.shape}")
            cams = tuple(f.shape[1:3] for f in frames)
        if self._cams is not None and cams != self._cams:
            raise ValueError(f"camera presence and geometry must be the same for every episode: had {self._cams or 'no cameras'}, got {cams or 'no cameras'}")
        if self._steps + L >= 2 ** 31:
            raise ValueError(f"the store holds at most 2^31 - 1 steps, this episode would make {self._steps + L}")
        self._cams = cams
        self._episodes.append((a, np.ascontiguousarray(g, dtype=np.float32), *(None if f is None else np.ascontiguousarray(f) for f in frames)))
        self._steps += L

    def _bounds(self, normalize):
        """(lo, hi, scale) fp32 host vectors, or None."""
        A = self.action_dim
        if normalize is None:
            return None
        if isinstance(normalize, str):
            if normalize != "minmax":
                raise ValueError(f"normalize must be 'minmax', None or (lo, hi), got {normalize!r}")
            lo = np.min([e[0].min(axis=0) for e in self._episodes], axis=0)
            hi = np.max([e[0].max(axis=0) for e in self._episodes], axis=0)
        else:
            try:
                lo, hi = (np.asarray(_host(v, "bound") if torch.is_tensor(v) else v, dtype=np.float32) for v in normalize)
            except (TypeError, ValueError):
                raise ValueError(f"normalize must be 'minmax', None or (lo, hi), got {normalize!r}") from None
            if lo.shape != (A,) or hi.shape != (A,) or not (np.isfinite(lo).all() and np.isfinite(hi).all()) or (hi < lo).any():
                raise ValueError(f"normalize=(lo, hi) needs two finite [{A}] vectors with hi >= lo")
        lo, hi = lo.astype(np.float32), hi.astype(np.float32)
        span = hi.astype(np.float64) - lo.astype(np.float64)
        scale = np.where(span > 0, 2.0 / np.where(span > 0, span, 1.0), 0.0).astype(np.float32)
        if not np.isfinite(scale).all():
            raise ValueError("normalize: 2 / (hi - lo) overflows fp32 in some dimension")
        return lo, hi, scale

    def finalize(self, normalize="minmax") -> "EpisodeStore":
        if self.finalized:
            raise ValueError("the store is finalized: it is read-only")
        if not self._episodes:
            raise ValueError("the store is empty: add at least one episode")
        bounds = self._bounds(normalize)
        lengths = np.array([e[0].shape[0] for e in self._episodes], dtype=np.int64)
        begin = np.concatenate([[0], np.cumsum(lengths)])
        S, dev = int(begin[-1]), self.device
        if S >= 2 ** 31:
            raise ValueError(f"the store holds at most 2^31 - 1 steps, got {S}")
        self.actions = torch.empty(S, self.action_dim, dtype=torch.float32, device=dev)
        self.goals = torch.from_numpy(np.stack([e[1] for e in self._episodes])).to(dev)
        self.ep_begin = torch.from_numpy(begin.astype(np.int32)).to(dev)
        fr = [None, None]
        for q in range(2 if self._cams else 0):
            fr[q] = torch.empty(S, *self._cams[q], 3, dtype=torch.uint8, device=dev)
        for ep, b in zip(self._episodes, begin[:-1]):            # episode by episode: the host never holds a second copy of the frames
            n = ep[0].shape[0]
            self.actions[b: b + n].copy_(torch.from_numpy(ep[0]))
            for q in range(2):
                if fr[q] is not None:
                    fr[q][b: b + n].copy_(torch.from_numpy(ep[2 + q]))
        self.frames_static, self.frames_gripper = fr
        if bounds is not None:
            self.lo, self.hi, self.scale = (torch.from_numpy(v).to(dev) for v in bounds)
        self.lengths = lengths
        self._episodes = []
        self.finalized = True
        return self


class WindowStream:
    """``batch(step)`` -> the training batch of step ``step`` as a dict of device tensors, without a host sync:

        actions [B, W, A] fp32 (normalised), action_mask [B, W] fp32 (1 = a real step, 0 = a padded one), latent_goal [B, G] fp32,
        index [B] int32 (the window's first store row = the observation's frame row), episode [B] int32,
        noise [B, W, A] fp32 (unit normal) and u [B] fp64 (uniform strictly inside (0, 1), for the sigma density) unless ``noise=False``,
        rgb_obs {"rgb_static", "rgb_gripper"} [B, 3, OH, OW] with ``camera_transforms=(t_static, t_gripper)``, and then also
        shifts {"rgb_static", "rgb_gripper"} int32 [B, 2] (None for a transform with ``shift_pad == 0``)

    ``pad="none"`` draws only windows that lie inside an episode (episodes shorter than ``window`` are never drawn); ``pad="hold"`` lets a window
    start at every step, holds the episode's last action past its end and marks those rows with ``action_mask = 0``.  Draws are i.i.d. uniform
    over the starts, with replacement (not an epoch permutation).  Row ``j`` of step ``t`` depends on ``(seed, t, j)`` and the store only:
    ``noise[j] == rollout.env_noise([(seed + 1 + j * 0x9E3779B9) % 2**32], [t], W, A, 1.0)[0]``."""

    def __init__(self, store: EpisodeStore, batch_size: int, window: int, seed: int = 0, pad: str = "hold",
                 camera_transforms: Optional[Sequence[CameraTransform]] = None, noise: bool = True, frame_dtype=torch.float32):
        if not isinstance(store, EpisodeStore) or not store.finalized:
            raise ValueError("WindowStream needs a finalized EpisodeStore")
        for name, v, hi in (("batch_size", batch_size, MAX_BATCH), ("window", window, MAX_WINDOW_FLOATS), ("seed", seed, 2 ** 32 - 1)):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < (0 if name == "seed" else 1) or v > hi:
                raise ValueError(f"{name} must be an int in {0 if name == 'seed' else 1}..{hi}, got {v!r}")
        if window * store.action_dim > MAX_WINDOW_FLOATS:
            raise ValueError(f"window * action_dim must be at most {MAX_WINDOW_FLOATS}, got {window} * {store.action_dim}")
        if store.goal_dim > MAX_GOAL_DIM:
            raise ValueError(f"goal_dim must be at most {MAX_GOAL_DIM}, got {store.goal_dim}")
        if pad not in _PADS:
            raise ValueError(f"pad must be one of {_PADS}, got {pad!r}")
        if frame_dtype not in (torch.float32, torch.bfloat16):
            raise ValueError(f"frame_dtype must be torch.float32 or torch.bfloat16, got {frame_dtype}")
        if camera_transforms is not None:
            camera_transforms = tuple(camera_transforms)
            if len(camera_transforms) != 2 or not all(isinstance(t, CameraTransform) for t in camera_transforms):
                raise ValueError("camera_transforms must be (static, gripper) CameraTransforms")
            if not store.has_cameras:
                raise ValueError("camera_transforms given, but the store holds no frames")
            for t, f, n in zip(camera_transforms, (store.frames_static, store.frames_gripper), ("rgb_static", "rgb_gripper")):
                t.check_source(f.shape[1], f.shape[2], n)
        n_e = store.lengths if pad == "hold" else np.maximum(0, store.lengths - window + 1)
        starts = np.concatenate([[0], np.cumsum(n_e)])
        if starts[-1] == 0:
            raise ValueError(f"no window of {window} steps fits any episode (pad='none'): nothing to draw")
        self.store, self.batch_size, self.window, self.seed, self.pad, self.noise = store, int(batch_size), int(window), int(seed), pad, bool(noise)
        self.camera_transforms, self.frame_dtype = camera_transforms, frame_dtype
        self.n_total = int(starts[-1])
        self.starts = torch.from_numpy(starts.astype(np.int32)).to(store.device)            # the device table the kernel searches

    def batch(self, step: int) -> dict:
        from . import _lib as L
        from . import camera
        from .engine import _stream
        if isinstance(step, bool) or not isinstance(step, (int, np.integer)) or not 0 <= step < 2 ** 32:
            raise ValueError(f"step must be an int in 0..2^32 - 1, got {step!r}")
        st, B, W = self.store, self.batch_size, self.window
        A, G, dev = st.action_dim, st.goal_dim, st.device
        if dev.type != "cuda":
            raise ValueError(f"WindowStream.batch: the store must be on a ROCm device (there is no CPU path), got {dev}")
        f32 = lambda *s: torch.empty(s, dtype=torch.float32, device=dev)
        i32 = lambda *s: torch.empty(s, dtype=torch.int32, device=dev)
        out = {"actions": f32(B, W, A), "action_mask": f32(B, W), "latent_goal": f32(B, G), "index": i32(B), "episode": i32(B)}
        if self.noise:
            out["noise"], out["u"] = f32(B, W, A), torch.empty(B, dtype=torch.float64, device=dev)
        tr = self.camera_transforms
        shifts = [i32(B, 2) if tr is not None and tr[q].shift_pad > 0 else None for q in range(2)]
        p = lambda t: None if t is None else t.data_ptr()
        d = L.ModeDataStreamDesc(actions=p(st.actions), ep_begin=p(st.ep_begin), starts=p(self.starts), goals=p(st.goals), lo=p(st.lo), scale=p(st.scale),
                                 S=st.actions.shape[0], E=st.goals.shape[0], A=A, G=G, W=W, B=B, n_total=self.n_total, seed=self.seed, step=int(step),
                                 out_actions=p(out["actions"]), action_mask=p(out["action_mask"]), latent_goal=p(out["latent_goal"]),
                                 index=p(out["index"]), episode=p(out["episode"]), noise=p(out.get("noise")), u=p(out.get("u")))
        for q in range(2):
            d.shifts[q] = p(shifts[q])
            d.shift_pad[q] = tr[q].shift_pad if tr is not None else 0
        with torch.cuda.device(dev):
            L.check(L.load().mode_data_sample_windows(C.byref(d), _stream()), "data_sample_windows")
        if tr is not None:
            frames = (st.frames_static, st.frames_gripper)
            dst = [torch.empty(tr[q].out_shape((B,) + tuple(frames[q].shape[1:])), dtype=self.frame_dtype, device=dev) for q in range(2)]
            camera.launch([(tr[q], frames[q], dst[q], shifts[q]) for q in range(2)], out["index"].data_ptr(), B, frames[0].shape[0])
            out["rgb_obs"] = {"rgb_static": dst[0], "rgb_gripper": dst[1]}
            out["shifts"] = {"rgb_static": shifts[0], "rgb_gripper": shifts[1]}
        return out
