"""Episodes held on the device, and the training batch of step ``t`` as a pure function of ``(seed, t)``.

``EpisodeStore`` takes whole episodes (actions, one goal embedding, optionally both cameras' uint8 frames) from the host, and ``finalize()``
uploads them once into flat device buffers.  ``WindowStream.batch(t)`` then draws ``batch_size`` windows of ``window`` consecutive actions in ONE
HIP launch (csrc/data_stream.hip; the expressions, bit for bit, are the comment of ``mode_data_sample_windows`` in include/mode_hip.h), plus one
``mode_frames_preprocess`` launch that reads the drawn frames straight out of the store when it holds cameras.  There is no host work per step,
no host sync and no state: a run resumed at step ``t`` with the same seed and store sees the same windows, noise, sigma uniforms and shifts.

By default windows are drawn i.i.d. uniformly over all window starts, WITH replacement: within any stretch of steps some starts repeat and
others are not seen.  ``WindowStream(order="epoch")`` visits every start exactly once per epoch instead - a keyed permutation the kernel evaluates
per row, so there is still no stored shuffle and nothing to checkpoint but the step counter - and ``WindowStream(episode_weights=w)`` draws the
episode from a weighted mixture (``mixture_weights`` builds ``w`` for datasets or tasks of unequal size) and the start uniformly within it; both
run ``mode_data_sample_windows_ordered``, one launch in place of the default's.  Reading CALVIN / LIBERO files and sharding the store across
ranks are not part of this module (rank ``r`` of a data-parallel run may simply use ``seed + 16 * r``: the stream's keys use ``seed .. seed + 7``).

Goal images (hindsight relabelling): a store that also holds one goal-space embedding per step (``add_episode(step_goals=[L, G])``, typically the
image-goal encoder's output for that step's frame, computed offline) lets ``WindowStream`` / ``WindowSweep(goal="hindsight", goal_horizon=(lo,
hi))`` replace a row's episode goal by the embedding of a step ``lo .. hi`` steps after the window's first one - the episode's final step once
that passes its end - in ONE further launch (``mode_data_relabel_goals``) with counter-based draws: no host work, no sync, the same bits when
step ``t`` is asked for again.  ``hindsight_prob`` mixes both kinds of goal row by row.  Not provided: encoding goal FRAMES inside the stream
(``goal_index`` lets a caller gather ``store.frames_static[goal_index]`` and run an encoder of their own), fusing the relabel into the sampling
launches, geometric or otherwise non-uniform horizon densities, disk formats, epoch order with weights (weighted sampling without replacement),
per-epoch curricula and a sharded store.

Holding episodes out: ``split_episodes`` names a training and a validation set of episode ids, ``WindowStream(episodes=train_ids)`` draws from
the first only, and ``WindowSweep(episodes=val_ids)`` enumerates every window of the second exactly once, a batch per launch
(``mode_data_sweep_windows``) - what ``validation.Validator`` runs the sampler on.  The normalisation stays the store's own: the bounds of
``finalize("minmax")`` are taken over ALL episodes, the held-out ones included; ``finalize((lo, hi))`` with bounds of the training episodes
avoids that.
"""
from __future__ import annotations

from fractions import Fraction
from typing import Optional, Sequence

import numpy as np
import torch

from . import _lib
from ._checks import _checked_float, _checked_int
from .camera import CameraTransform
from .engine import _launch, _ptr

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


def _as_numpy(x, name: str, dtype=None) -> np.ndarray:
    """A numpy array from a tensor or a sequence: ``np.asarray`` with its own TypeError / ValueError for what it does not take."""
    return np.asarray(_host(x, name) if torch.is_tensor(x) else x, dtype=dtype)


def _checked_u32(v, name: str) -> int:
    return _checked_int(v, 0, 2 ** 32 - 1, f"{name} must be an int in 0..2^32 - 1, got {v!r}")


class EpisodeStore:
    """``add_episode(actions [L, A] float, goal [G] float, rgb_static=None, rgb_gripper=None, step_goals=None)`` with frames uint8
    ``[L, H, W, 3]`` / ``[L, Hg, Wg, 3]``: either both cameras for every episode or for none, one geometry per camera; ``step_goals`` float
    ``[L, G]``, the embedding of every step's observation in the goal space (finite), for every episode or for none.  ``finalize(normalize)`` uploads

        actions [S, A] fp32 (S = total steps), ep_begin [E + 1] int32, goals [E, G] fp32, frames_static / frames_gripper [S, H, W, 3] uint8,
        lo / hi / scale [A] fp32 (None without normalisation), step_goals [S, G] in ``step_goal_dtype`` (None without them; torch.float32, or
        torch.bfloat16 for half the memory: one round-to-nearest-even of the fp32 values, torch's, at upload)

    to ``device``; afterwards the store is read-only.  ``normalize="minmax"``: ``lo`` / ``hi`` per action dimension over all steps,
    ``scale = 2 / (hi - lo)`` computed in fp64 and rounded to fp32, 0 where ``hi == lo`` (such a dimension normalises to -1); ``(lo, hi)``: the
    caller's bounds, same formula; ``None``: the stream returns the stored bits.  Every refusal is a ``ValueError`` raised before anything is
    allocated on the device."""

    def __init__(self, action_dim: int, goal_dim: int, device="cuda", step_goal_dtype=torch.float32):
        for name, v in (("action_dim", action_dim), ("goal_dim", goal_dim)):
            _checked_int(v, 1, None, f"{name} must be a positive int, got {v!r}")
        if step_goal_dtype not in (torch.float32, torch.bfloat16):
            raise ValueError(f"step_goal_dtype must be torch.float32 or torch.bfloat16, got {step_goal_dtype}")
        self.action_dim, self.goal_dim, self.device, self.step_goal_dtype = int(action_dim), int(goal_dim), torch.device(device), step_goal_dtype
        # host side, until finalize(): (actions fp32, goal fp32, static u8 | None, gripper u8 | None, step goals fp32 | None)
        self._episodes = []
        self._steps = 0
        self._cams: Optional[tuple] = None       # None until the first episode: then () or ((H, W), (Hg, Wg))
        self._has_step_goals: Optional[bool] = None      # None until the first episode
        self.finalized = False
        self.actions = self.ep_begin = self.goals = self.frames_static = self.frames_gripper = self.lo = self.hi = self.scale = self.step_goals = None
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

    def add_episode(self, actions, goal, rgb_static=None, rgb_gripper=None, step_goals=None) -> None:
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
        sg = None
        if step_goals is not None:
            sg = _host(step_goals, "step_goals")
            if sg.shape != (L, self.goal_dim) or not np.issubdtype(sg.dtype, np.floating):
                raise ValueError(f"step_goals must be a float [{L}, {self.goal_dim}] array (one embedding per step), got {sg.dtype} {sg.shape}")
            with np.errstate(over="ignore"):
                sg = np.ascontiguousarray(sg, dtype=np.float32)
            # bf16 rounds to nearest even: from 2^128 - 2^119 (halfway between the largest bf16 and 2^128) on, a finite fp32 becomes inf
            if not np.isfinite(sg).all() or (self.step_goal_dtype == torch.bfloat16 and (np.abs(sg) >= np.float32(2.0 ** 128 - 2.0 ** 119)).any()):
                raise ValueError(f"step_goals hold a non-finite value (or one that overflows {'bf16' if self.step_goal_dtype == torch.bfloat16 else 'fp32'})")
        if self._has_step_goals is not None and (sg is not None) != self._has_step_goals:
            raise ValueError(f"give step_goals for every episode or for none: had {'them' if self._has_step_goals else 'none'}, "
                             f"got {'none' if sg is None else 'them'}")
        if self._steps + L >= 2 ** 31:
            raise ValueError(f"the store holds at most 2^31 - 1 steps, this episode would make {self._steps + L}")
        self._cams, self._has_step_goals = cams, sg is not None
        self._episodes.append((a, np.ascontiguousarray(g, dtype=np.float32), *(None if f is None else np.ascontiguousarray(f) for f in frames), sg))
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
                lo, hi = (_as_numpy(v, "bound", np.float32) for v in normalize)
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
        if self._has_step_goals:
            self.step_goals = torch.empty(S, self.goal_dim, dtype=self.step_goal_dtype, device=dev)
        for ep, b in zip(self._episodes, begin[:-1]):            # episode by episode: the host never holds a second copy of the frames
            n = ep[0].shape[0]
            self.actions[b: b + n].copy_(torch.from_numpy(ep[0]))
            for q in range(2):
                if fr[q] is not None:
                    fr[q][b: b + n].copy_(torch.from_numpy(ep[2 + q]))
            if self.step_goals is not None:                      # fp32 -> bf16: torch's round-to-nearest-even, wherever the copy converts
                self.step_goals[b: b + n].copy_(torch.from_numpy(ep[4]))
        self.frames_static, self.frames_gripper = fr
        if bounds is not None:
            self.lo, self.hi, self.scale = (torch.from_numpy(v).to(dev) for v in bounds)
        self.lengths = lengths
        self._episodes = []
        self.finalized = True
        return self


def split_episodes(store: EpisodeStore, val_fraction: Optional[float] = None, val_episodes=None, seed: int = 0):
    """``(train_ids, val_ids)``: two sorted, disjoint int64 numpy arrays that together cover ``range(store.num_episodes)``.  ``val_fraction=f``
    (0 < f < 1) holds out ``max(1, round(f * E))`` episodes, the first of ``numpy.random.default_rng(seed).permutation(E)``;
    ``val_episodes=ids`` holds out the caller's.  ValueError for neither or both arguments, a fraction outside (0, 1), an id out of range, a
    repeated id, or a side left empty."""
    if not isinstance(store, EpisodeStore):
        raise ValueError("split_episodes needs an EpisodeStore")
    E = store.num_episodes
    if (val_fraction is None) == (val_episodes is None):
        raise ValueError("give exactly one of val_fraction and val_episodes")
    if val_fraction is not None:
        f = _checked_float(val_fraction, 0.0, 1.0, f"val_fraction must lie strictly inside (0, 1), got {val_fraction!r}", lo_open=True, hi_open=True)
        val = np.random.default_rng(seed).permutation(E)[: max(1, int(round(f * E)))]
    else:
        val = _episode_ids(val_episodes, E, "val_episodes")
    val = np.sort(np.asarray(val, dtype=np.int64))
    train = np.setdiff1d(np.arange(E, dtype=np.int64), val)
    if len(val) == 0 or len(train) == 0:
        raise ValueError(f"the split leaves a side empty: {len(train)} training and {len(val)} validation episodes of {E}")
    return train, val


def _episode_ids(ids, E: int, name: str) -> np.ndarray:
    """``ids`` as a sorted int64 array of distinct episode numbers in [0, E); ValueError otherwise."""
    try:
        arr = _as_numpy(ids, name)
    except (TypeError, ValueError):
        raise ValueError(f"{name} must be a sequence of episode ids") from None
    if arr.ndim != 1 or (arr.size and (arr.dtype == np.bool_ or not np.issubdtype(arr.dtype, np.integer))):
        raise ValueError(f"{name} must be a 1-d sequence of ints, got {arr.dtype} {arr.shape}")
    arr = arr.astype(np.int64)
    if arr.size and (arr.min() < 0 or arr.max() >= E):
        raise ValueError(f"{name} holds an id outside 0..{E - 1}")
    if len(np.unique(arr)) != len(arr):
        raise ValueError(f"{name} repeats an id")
    return np.sort(arr)


def _start_counts(lengths: np.ndarray, window: int, pad: str, stride: int = 1) -> np.ndarray:
    """How many windows start in each episode, ``stride`` steps apart: ``pad="hold"`` starts one at every stride-th step, ``ceil(L / stride)``;
    ``pad="none"`` only where the whole window fits, ``(L - W) // stride + 1`` when ``L >= W``, else none."""
    return -(-lengths // stride) if pad == "hold" else np.where(lengths >= window, (lengths - window) // stride + 1, 0)


def _start_table(n_e: np.ndarray, episodes, what: str):
    """The ``starts`` table the kernels search: the prefix sums of ``n_e``, with ``n_e = 0`` for an episode that ``episodes`` (None = all) does
    not list - the search never finds an episode without starts.  -> (int64 host table, n_total); ValueError when nothing is left."""
    n_e = np.asarray(n_e, dtype=np.int64)
    if episodes is not None:
        keep = np.zeros(len(n_e), dtype=bool)
        keep[_episode_ids(episodes, len(n_e), "episodes")] = True
        n_e = np.where(keep, n_e, 0)
    starts = np.concatenate([[0], np.cumsum(n_e)])
    if starts[-1] == 0:
        raise ValueError(what)
    return starts, int(starts[-1])


def _check_window_args(store, batch_size, window, seed, pad, camera_transforms, frame_dtype, who: str):
    """The constructor checks WindowStream and WindowSweep share; returns the transforms as a tuple (or None)."""
    if not isinstance(store, EpisodeStore) or not store.finalized:
        raise ValueError(f"{who} needs a finalized EpisodeStore")
    for name, v, lo, hi in (("batch_size", batch_size, 1, MAX_BATCH), ("window", window, 1, MAX_WINDOW_FLOATS), ("seed", seed, 0, 2 ** 32 - 1)):
        _checked_int(v, lo, hi, f"{name} must be an int in {lo}..{hi}, got {v!r}")
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
    return camera_transforms


_GOALS = ("episode", "hindsight")
MAX_HORIZON = 2 ** 31 - 1


def _check_goal_args(store: EpisodeStore, goal, goal_horizon, hindsight_prob, who: str, sweep: bool):
    """The goal keywords WindowStream and WindowSweep share -> None for ``goal="episode"``, else ``(lo, hi, thresh)`` of
    ``mode_data_relabel_goals``.  A sweep's horizon may also be an int ``d`` (lo = hi = d) or ``"last"`` (the episode's final step)."""
    if not isinstance(goal, str) or goal not in _GOALS:
        raise ValueError(f"goal must be one of {_GOALS}, got {goal!r}")
    prob = _checked_float(hindsight_prob, 0.0, 1.0, f"hindsight_prob must lie in [0, 1], got {hindsight_prob!r}")
    if goal == "episode":
        if goal_horizon is not None:
            raise ValueError(f"goal_horizon={goal_horizon!r} needs goal='hindsight': goal='episode' draws no goal step")
        return None
    if store.step_goals is None:
        raise ValueError(f"{who}(goal='hindsight') needs a store with step_goals (EpisodeStore.add_episode(step_goals=))")
    if goal_horizon is None:
        raise ValueError(f"{who}(goal='hindsight') needs goal_horizon=(lo, hi), offsets in steps from the window's first step")
    is_int = lambda v: not isinstance(v, bool) and isinstance(v, (int, np.integer))
    if sweep and isinstance(goal_horizon, str) and goal_horizon == "last":
        lo = hi = MAX_HORIZON
    elif sweep and is_int(goal_horizon):
        lo = hi = int(goal_horizon)
    elif isinstance(goal_horizon, (tuple, list)) and len(goal_horizon) == 2 and all(is_int(v) for v in goal_horizon):
        lo, hi = (int(v) for v in goal_horizon)
    else:
        raise ValueError(f"goal_horizon must be (lo, hi), two ints{', an int or last' if sweep else ''}, got {goal_horizon!r}")
    if not 0 <= lo <= hi <= MAX_HORIZON:
        raise ValueError(f"goal_horizon needs 0 <= lo <= hi <= 2^31 - 1, got {goal_horizon!r}")
    return lo, hi, int(round(prob * 2.0 ** 32))


def _relabel_goals(store: EpisodeStore, out: dict, ids: Optional[torch.Tensor], seed: int, step: int, plan) -> None:
    """One ``mode_data_relabel_goals`` launch behind the sampling launch that filled ``out``: ``latent_goal`` updated in place, ``goal_index`` /
    ``goal_offset`` / ``goal_kind`` added.  ``ids`` None: a row's draws are keyed by its place; a sweep passes its ``window``."""
    lo, hi, thresh = plan
    B, dev = out["index"].shape[0], store.device
    out["goal_index"], out["goal_offset"] = (torch.empty(B, dtype=torch.int32, device=dev) for _ in range(2))
    out["goal_kind"] = torch.empty(B, dtype=torch.float32, device=dev)
    d = _lib.ModeDataGoalDesc(step_goals=store.step_goals.data_ptr(), ep_begin=store.ep_begin.data_ptr(), index=out["index"].data_ptr(),
                              episode=out["episode"].data_ptr(), ids=None if ids is None else ids.data_ptr(), thresh=thresh,
                              goal_dtype=_lib.MODE_BF16 if store.step_goals.dtype == torch.bfloat16 else _lib.MODE_F32, S=store.step_goals.shape[0],
                              E=store.goals.shape[0], G=store.goal_dim, B=B, seed=seed, step=step, lo=lo, hi=hi,
                              latent_goal=out["latent_goal"].data_ptr(), goal_index=out["goal_index"].data_ptr(),
                              goal_offset=out["goal_offset"].data_ptr(), goal_kind=out["goal_kind"].data_ptr())
    _launch(_lib.load().mode_data_relabel_goals, d, dev)


_ORDERS = ("iid", "epoch")


def _cut_table(episode_weights, n_e: np.ndarray) -> np.ndarray:
    """The int64 ``cut`` table of ``mode_data_sample_windows_ordered`` (include/mode_hip.h) for the weights ``w`` [E] and the start counts ``n_e``
    (0 for an episode that is not listed or that no window fits): mass ``w_e`` where ``n_e > 0`` else 0, ``C`` its fp64 running sum in episode
    order, ``cut[e] = floor(2^32 * (C_e / C_E))``, ``cut[E] = 2^32``.  ValueError for weights that are not E finite non-negative numbers, a total
    mass of 0 (or one that overflows fp64), or a positive mass whose interval comes out empty."""
    E = len(n_e)
    try:
        w = _as_numpy(episode_weights, "episode_weights")
        if w.dtype == np.bool_ or not (np.issubdtype(w.dtype, np.floating) or np.issubdtype(w.dtype, np.integer)):
            raise TypeError
        w = w.astype(np.float64)
    except (TypeError, ValueError):
        raise ValueError("episode_weights must be a sequence of numbers, one per episode") from None
    if w.shape != (E,):
        raise ValueError(f"episode_weights must hold one number per episode of the store ({E}), got shape {w.shape}")
    if not np.isfinite(w).all() or (w < 0).any():
        raise ValueError("episode_weights must be finite and non-negative")
    mass = np.where(np.asarray(n_e) > 0, w, 0.0)
    with np.errstate(over="ignore"):
        run = np.concatenate([[0.0], np.cumsum(mass)])
    if not run[-1] > 0.0 or not np.isfinite(run[-1]):
        raise ValueError("episode_weights leave no mass on an episode with a window start (or their sum overflows): nothing to draw")
    cut = np.floor(2.0 ** 32 * (run / run[-1])).astype(np.int64)
    cut[-1] = 2 ** 32
    empty = (mass > 0) & (cut[1:] == cut[:-1])
    if empty.any():
        e = int(np.argmax(empty))
        raise ValueError(f"episode_weights[{e}] = {w[e]!r} is positive but below 2^-32 of the total mass: it rounds to an empty interval (give 0 "
                         f"to leave the episode out)")
    return cut


def mixture_weights(store: EpisodeStore, groups, group_weights, episodes=None, window: Optional[int] = None, pad: str = "hold") -> np.ndarray:
    """Per-episode weights (fp64 numpy [E]) for ``WindowStream(episode_weights=)`` under which a batch row comes from group ``d`` with probability
    ``group_weights[d] / sum(group_weights)`` and, within the group, from each of its window starts with equal probability:

        w_e = p_d * n_e / N_d,   d = groups[e],  p_d = group_weights[d] / sum(group_weights),  N_d = the sum of n_e over the group

    ``groups`` [E] holds every episode's group number in ``0 .. len(group_weights) - 1`` (a dataset of a pre-training mixture, a task of a suite).
    ``n_e`` counts the starts the stream will see: ``L_e`` for ``pad="hold"`` (the default; ``window`` is not needed), ``max(0, L_e - window + 1)``
    for ``pad="none"``, and 0 for an episode that ``episodes=`` (the stream's own keyword; None = all) does not list - pass the stream the same
    ``window``, ``pad`` and ``episodes``.  ValueError for a ``groups`` of another size or with a number out of range, group weights that are not
    finite, non-negative and of positive sum, and a group of positive weight without a start.

    Per-START weights need no helper: a start of episode ``e`` is drawn with probability proportional to ``s_e`` under
    ``episode_weights = s * n_e`` (``s = 1``: the uniform draw over the starts that the stream makes without weights)."""
    if not isinstance(store, EpisodeStore) or not store.finalized:
        raise ValueError("mixture_weights needs a finalized EpisodeStore")
    if pad not in _PADS:
        raise ValueError(f"pad must be one of {_PADS}, got {pad!r}")
    E = store.num_episodes
    if pad == "none":
        window = _checked_int(window, 1, None, f"pad='none' needs window, an int >= 1, got {window!r}")
    n_e = np.diff(_start_table(_start_counts(store.lengths, window, pad), episodes, "no window fits any selected episode: nothing to weigh")[0])
    try:
        p = np.asarray(group_weights, dtype=np.float64)
        g = _as_numpy(groups, "groups")
    except (TypeError, ValueError):
        raise ValueError("groups must be a sequence of ints and group_weights a sequence of numbers") from None
    if p.ndim != 1 or p.size == 0 or not np.isfinite(p).all() or (p < 0).any() or not p.sum() > 0 or not np.isfinite(p.sum()):
        raise ValueError("group_weights must be a non-empty 1-d sequence of finite non-negative numbers with a positive sum")
    if g.shape != (E,) or g.dtype == np.bool_ or not np.issubdtype(g.dtype, np.integer) or g.min() < 0 or g.max() >= p.size:
        raise ValueError(f"groups must hold one int in 0..{p.size - 1} per episode of the store ({E})")
    N = np.bincount(g, weights=n_e.astype(np.float64), minlength=p.size)
    if ((p > 0) & (N == 0)).any():
        raise ValueError(f"group {int(np.argmax((p > 0) & (N == 0)))} has a positive weight but no window start")
    p = p / p.sum()
    return np.where(n_e > 0, p[g] * n_e / np.where(N[g] > 0, N[g], 1.0), 0.0)


def _frames_of(store: EpisodeStore, tr, shifts, index: torch.Tensor, B: int, frame_dtype) -> dict:
    """``rgb_obs`` of a batch: one ``mode_frames_preprocess`` launch that reads the store rows ``index`` (``shifts[q]`` None: no shift)."""
    from . import camera
    frames = (store.frames_static, store.frames_gripper)
    dst = [torch.empty(tr[q].out_shape((B,) + tuple(frames[q].shape[1:])), dtype=frame_dtype, device=store.device) for q in range(2)]
    camera.launch([(tr[q], frames[q], dst[q], shifts[q]) for q in range(2)], index.data_ptr(), B, frames[0].shape[0])
    return {"rgb_static": dst[0], "rgb_gripper": dst[1]}


def _window_outputs(src, who: str):
    """What ``WindowStream.batch`` and ``WindowSweep.batch`` (``src``; ``who`` names it in the refusal) share: the device check, the five outputs
    of a located window and the descriptor fields that ModeDataStreamDesc and ModeDataSweepDesc have in common, as keyword arguments."""
    st, B, W = src.store, src.batch_size, src.window
    A, G, dev = st.action_dim, st.goal_dim, st.device
    if dev.type != "cuda":
        raise ValueError(f"{who}.batch: the store must be on a ROCm device (there is no CPU path), got {dev}")
    f32 = lambda *s: torch.empty(s, dtype=torch.float32, device=dev)
    i32 = lambda *s: torch.empty(s, dtype=torch.int32, device=dev)
    out = {"actions": f32(B, W, A), "action_mask": f32(B, W), "latent_goal": f32(B, G), "index": i32(B), "episode": i32(B)}
    return out, dict(actions=_ptr(st.actions), ep_begin=_ptr(st.ep_begin), starts=_ptr(src.starts), goals=_ptr(st.goals), lo=_ptr(st.lo),
                     scale=_ptr(st.scale), S=st.actions.shape[0], E=st.goals.shape[0], A=A, G=G, W=W, B=B, n_total=src.n_total, seed=src.seed,
                     out_actions=_ptr(out["actions"]), action_mask=_ptr(out["action_mask"]), latent_goal=_ptr(out["latent_goal"]),
                     index=_ptr(out["index"]), episode=_ptr(out["episode"]))


class WindowStream:
    """``batch(step)`` -> the training batch of step ``step`` as a dict of device tensors, without a host sync:

        actions [B, W, A] fp32 (normalised), action_mask [B, W] fp32 (1 = a real step, 0 = a padded one), latent_goal [B, G] fp32,
        index [B] int32 (the window's first store row = the observation's frame row), episode [B] int32,
        noise [B, W, A] fp32 (unit normal) and u [B] fp64 (uniform strictly inside (0, 1), for the sigma density) unless ``noise=False``,
        rgb_obs {"rgb_static", "rgb_gripper"} [B, 3, OH, OW] with ``camera_transforms=(t_static, t_gripper)``, and then also
        shifts {"rgb_static", "rgb_gripper"} int32 [B, 2] (None for a transform with ``shift_pad == 0``)

    ``pad="none"`` draws only windows that lie inside an episode (episodes shorter than ``window`` are never drawn); ``pad="hold"`` lets a window
    start at every step, holds the episode's last action past its end and marks those rows with ``action_mask = 0``.  By default draws are i.i.d. uniform
    over the starts, with replacement (``order`` and ``episode_weights`` below change that).  Row ``j`` of step ``t`` depends on ``(seed, t, j)`` and the store only:
    ``noise[j] == rollout.env_noise([(seed + 1 + j * 0x9E3779B9) % 2**32], [t], W, A, 1.0)[0]``.

    ``episodes=ids`` (``split_episodes``) draws from the listed episodes only: an episode that is not listed gets no starts, and the kernel's search
    never finds an episode without starts.  None, the default, builds the table of all episodes.  The normalisation stays the store's own - the
    bounds of ``finalize("minmax")`` include the episodes left out here; ``finalize((lo, hi))`` avoids that.

    ``goal="hindsight", goal_horizon=(lo, hi)`` (ints, ``0 <= lo <= hi <= 2^31 - 1``; the store must hold ``step_goals``) relabels in one further
    launch (``mode_data_relabel_goals`` in include/mode_hip.h states the draws bit for bit): row ``j`` is chosen with probability
    ``hindsight_prob`` (``thresh = round(hindsight_prob * 2^32)``), draws an offset uniformly in ``lo .. hi`` and, if chosen, gets
    ``latent_goal[j] = store.step_goals[goal_index[j]]`` with ``goal_index = min(index + offset, the episode's last row)``; a row that is not
    chosen keeps its episode's goal - both modalities mixed row by row in one forward.  The batch gains ``goal_index``, ``goal_offset`` (int32
    [B], written for every row) and ``goal_kind`` (fp32 [B], 1 = relabelled).  The draws use the keys ``seed + 4`` and ``seed + 5`` and depend on
    ``(seed, t, j)`` only.  ``goal="episode"``, the default, is the stream without any of this: the same launches, keys and bits.

    ``order="epoch"``: every window exactly once per epoch, still without host work, state or a stored shuffle (``mode_data_sample_windows_ordered``
    in include/mode_hip.h states it bit for bit).  With ``n = n_total`` row ``j`` of step ``t`` has the global position ``P = t * B + j`` (64 bits),
    the epoch ``P // n`` and the place ``q = P % n`` in it, and draws window number ``perm(seed, epoch, n)(q)`` - a keyed bijection of ``[0, n)``
    (a balanced Feistel network of 10 rounds with cycle walking, key ``seed + 6``) that the kernel evaluates per row.  The ``n`` consecutive
    positions of an epoch visit every window start once; ``B`` need not divide ``n``: a batch that straddles an epoch boundary continues in the next
    epoch's permutation, nothing is dropped and nothing repeats within an epoch.  The batch gains ``epoch`` and ``position`` (int64 [B]; select
    ``epoch == k`` to cut at the boundary).  ``epoch_of(step)`` is the epoch of the step's first row and ``steps_per_epoch`` the exact
    ``fractions.Fraction(n, B)``: "train 30 epochs" is ``range(ceil(30 * steps_per_epoch))``.  Rows depend on ``(seed, t, j, B)``: resuming needs the
    same batch size.

    ``episode_weights=w`` (``E`` finite non-negative numbers; ``order="iid"`` only): episode ``e`` is drawn with probability proportional to ``w_e``
    over the episodes that ``episodes=`` lists and that have a start, then a start uniformly among that episode's - i.i.d., with replacement, in
    integer arithmetic (an int64 table of cuts of ``[0, 2^32]``, the start from key ``seed + 7``).  ``mixture_weights`` builds ``w`` for a weighted
    mixture of datasets or tasks; re-weighting is a new stream on the same store.  A weight of 0 leaves an episode out; a positive weight below
    ``2^-32`` of the total is refused, as are negative or non-finite weights, a wrong size and a total of 0 - ``ValueError`` before anything is
    allocated.  ``index`` and ``episode`` differ from the unweighted stream's; noise, ``u``, shifts and the hindsight draws stay keyed by
    ``(seed, t, j)`` in every mode.  Without either keyword the stream issues exactly the launches it always did.  Not provided: epoch order WITH
    weights (weighted sampling without replacement), per-epoch curricula, a sharded store, disk formats."""

    def __init__(self, store: EpisodeStore, batch_size: int, window: int, seed: int = 0, pad: str = "hold",
                 camera_transforms: Optional[Sequence[CameraTransform]] = None, noise: bool = True, frame_dtype=torch.float32, episodes=None,
                 goal: str = "episode", goal_horizon=None, hindsight_prob: float = 1.0, order: str = "iid", episode_weights=None):
        camera_transforms = _check_window_args(store, batch_size, window, seed, pad, camera_transforms, frame_dtype, "WindowStream")
        self.goal, self._goal_plan = goal, _check_goal_args(store, goal, goal_horizon, hindsight_prob, "WindowStream", sweep=False)
        if not isinstance(order, str) or order not in _ORDERS:
            raise ValueError(f"order must be one of {_ORDERS}, got {order!r}")
        if order == "epoch" and episode_weights is not None:
            raise ValueError("episode_weights needs order='iid': an epoch order with weights (weighted sampling without replacement) is not provided")
        starts, n_total = _start_table(_start_counts(store.lengths, window, pad), episodes, f"no window of {window} steps fits any "
                                       f"{'episode' if episodes is None else 'selected episode'} (pad={pad!r}): nothing to draw")
        cut = None if episode_weights is None else _cut_table(episode_weights, np.diff(starts))
        self.store, self.batch_size, self.window, self.seed, self.pad, self.noise = store, int(batch_size), int(window), int(seed), pad, bool(noise)
        self.camera_transforms, self.frame_dtype = camera_transforms, frame_dtype
        self.order = order
        self.n_total = n_total
        self.starts = torch.from_numpy(starts.astype(np.int32)).to(store.device)            # the device table the kernel searches
        self.cut = None if cut is None else torch.from_numpy(cut).to(store.device)          # int64 [E + 1], a weighted mixture's table

    @property
    def steps_per_epoch(self) -> Fraction:
        """``n_total / batch_size`` as an exact ``fractions.Fraction`` (``float()`` it for a plot, ``math.ceil`` it for a step count)."""
        return Fraction(self.n_total, self.batch_size)

    def epoch_of(self, step: int) -> int:
        """The epoch of row 0 of step ``step`` under ``order="epoch"``: ``(step * B) // n_total``.  The step's last row is in the same epoch or the next."""
        return (_checked_u32(step, "step") * self.batch_size) // self.n_total

    def batch(self, step: int) -> dict:
        step = _checked_u32(step, "step")
        out, common = _window_outputs(self, "WindowStream")
        st, B, W, dev = self.store, self.batch_size, self.window, self.store.device
        if self.noise:
            out["noise"] = torch.empty(B, W, st.action_dim, dtype=torch.float32, device=dev)
            out["u"] = torch.empty(B, dtype=torch.float64, device=dev)
        tr = self.camera_transforms
        shifts = [torch.empty(B, 2, dtype=torch.int32, device=dev) if tr is not None and tr[q].shift_pad > 0 else None for q in range(2)]
        d = _lib.ModeDataStreamDesc(**common, step=step, noise=_ptr(out.get("noise")), u=_ptr(out.get("u")))
        for q in range(2):
            d.shifts[q] = _ptr(shifts[q])
            d.shift_pad[q] = tr[q].shift_pad if tr is not None else 0
        if self.order == "iid" and self.cut is None:
            _launch(_lib.load().mode_data_sample_windows, d, dev)
        else:
            epoch = self.order == "epoch"
            if epoch:
                out["epoch"], out["position"] = (torch.empty(B, dtype=torch.int64, device=dev) for _ in range(2))
            o = _lib.ModeDataOrderDesc(s=d, mode=_lib.MODE_ORDER_EPOCH if epoch else _lib.MODE_ORDER_WEIGHTED, cut=_ptr(self.cut), epoch=_ptr(out.get("epoch")),
                                       position=_ptr(out.get("position")))
            _launch(_lib.load().mode_data_sample_windows_ordered, o, dev)
        if self._goal_plan is not None:
            _relabel_goals(st, out, None, self.seed, step, self._goal_plan)
        if tr is not None:
            out["rgb_obs"] = _frames_of(st, tr, shifts, out["index"], B, self.frame_dtype)
            out["shifts"] = {"rgb_static": shifts[0], "rgb_gripper": shifts[1]}
        return out


class WindowSweep:
    """Every window of the selected episodes exactly once, ``batch_size`` per launch: ``len(sweep) = ceil(n_total / B)`` batches, and
    ``batch(i, draw=0)`` -> the windows numbered ``i * B .. i * B + B - 1`` of a fixed enumeration as a dict of device tensors, without a host sync
    and without state (csrc/data_stream.hip; the expressions, bit for bit, are the comment of ``mode_data_sweep_windows`` in include/mode_hip.h):

        actions, action_mask, latent_goal, index, episode: as ``WindowStream`` returns them for a window at that place,
        valid [B] fp32 (1 = a window of the enumeration, 0 = a padding row of the last batch: it repeats the last window with a zero action_mask),
        window [B] int32 (the window's number), noise [B, W, A] fp32 (unit normal times ``noise_scale``), and
        rgb_obs {"rgb_static", "rgb_gripper"} [B, 3, OH, OW] with ``camera_transforms`` - no random shift: every transform is applied with its
        shift table absent

    Windows are numbered episode by episode, ``stride`` steps apart: with ``pad="hold"`` episode e has ``ceil(L_e / stride)`` windows (every
    stride-th step starts one; the last action is held past the end under ``action_mask = 0``), with ``pad="none"`` ``(L_e - W) // stride + 1`` when
    ``L_e >= W``, else none.  ``episodes=ids`` (``split_episodes``) sweeps the listed episodes only; None sweeps all.  ``B`` is fixed, so whatever
    consumes the batches (a captured sampler graph) sees one shape; weigh the rows with ``valid``.

    A row's noise belongs to its WINDOW, not to its place in a batch - ``noise[j] == rollout.env_noise([(seed + 1 + window[j] * 0x9E3779B9) %
    2**32], [draw], W, A, noise_scale)[0]`` - so a sweep gives a window the same noise at every batch size, and ``draw`` numbers independent
    repeats.  There is no ``u``.  The normalisation is the store's own (see ``WindowStream``).

    ``goal="hindsight"`` with ``goal_horizon=(lo, hi)``, an int ``d`` (``lo = hi = d``) or ``"last"`` (``lo = hi = 2^31 - 1``: the episode's final
    step) and ``hindsight_prob`` relabel as in ``WindowStream``, with the draws keyed by ``(seed, draw, window[j])``: a window's goal belongs to
    the window like its noise, the same at every batch size, and a padding row is relabelled like the window it repeats.  Such a sweep validates
    the image-goal modality; ``goal="episode"``, the default, is the sweep without any of this."""

    def __init__(self, store: EpisodeStore, batch_size: int, window: int, stride: int = 1, pad: str = "hold", episodes=None, seed: int = 0,
                 camera_transforms: Optional[Sequence[CameraTransform]] = None, frame_dtype=torch.float32, noise_scale: float = 1.0,
                 goal: str = "episode", goal_horizon=None, hindsight_prob: float = 1.0):
        camera_transforms = _check_window_args(store, batch_size, window, seed, pad, camera_transforms, frame_dtype, "WindowSweep")
        self.goal, self._goal_plan = goal, _check_goal_args(store, goal, goal_horizon, hindsight_prob, "WindowSweep", sweep=True)
        stride = _checked_int(stride, 1, None, f"stride must be an int >= 1, got {stride!r}")
        if isinstance(noise_scale, bool) or not np.isfinite(float(noise_scale)):
            raise ValueError(f"noise_scale must be a finite number, got {noise_scale!r}")
        starts, n_total = _start_table(_start_counts(store.lengths, window, pad, stride), episodes, f"no window of {window} steps fits any "
                                       f"{'episode' if episodes is None else 'selected episode'} (pad={pad!r}): nothing to sweep")
        self.store, self.batch_size, self.window, self.stride, self.pad, self.seed = store, int(batch_size), int(window), stride, pad, int(seed)
        self.camera_transforms, self.frame_dtype, self.noise_scale = camera_transforms, frame_dtype, float(noise_scale)
        self.n_total = n_total
        self.starts = torch.from_numpy(starts.astype(np.int32)).to(store.device)            # the device table the kernel searches

    def __len__(self) -> int:
        return -(-self.n_total // self.batch_size)

    def batch(self, i: int, draw: int = 0, noise_scale: Optional[float] = None) -> dict:
        """``noise_scale``: this batch's factor in place of the sweep's own (``validation.Validator`` asks for its ``sigma_max``)."""
        scale = self.noise_scale if noise_scale is None else float(noise_scale)
        if not np.isfinite(scale):
            raise ValueError(f"noise_scale must be a finite number, got {noise_scale!r}")
        i = _checked_int(i, 0, len(self) - 1, f"batch index must be an int in 0..{len(self) - 1}, got {i!r}")
        draw = _checked_u32(draw, "draw")
        out, common = _window_outputs(self, "WindowSweep")
        st, B, dev = self.store, self.batch_size, self.store.device
        out["valid"], out["window"] = torch.empty(B, dtype=torch.float32, device=dev), torch.empty(B, dtype=torch.int32, device=dev)
        out["noise"] = torch.empty(B, self.window, st.action_dim, dtype=torch.float32, device=dev)
        d = _lib.ModeDataSweepDesc(**common, stride=self.stride, first=i * B, draw=draw, noise_scale=scale, valid=_ptr(out["valid"]),
                                   window=_ptr(out["window"]), noise=_ptr(out["noise"]))
        _launch(_lib.load().mode_data_sweep_windows, d, dev)
        if self._goal_plan is not None:
            _relabel_goals(st, out, out["window"], self.seed, draw, self._goal_plan)
        if self.camera_transforms is not None:
            out["rgb_obs"] = _frames_of(st, self.camera_transforms, (None, None), out["index"], B, self.frame_dtype)
        return out
