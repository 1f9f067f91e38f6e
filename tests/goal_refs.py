"""Numpy restatement of hindsight goal relabelling as include/mode_hip.h states it (mode_data_relabel_goals): the two counter-based draws, the
clamp of the goal step to the episode's last one, the copy of the stored embedding (bf16 expanded exactly) and the rows that keep their episode
goal.  Validated without a GPU by tests/test_goal_references.py; the GPU tests compare the kernel against it bit for bit."""
from __future__ import annotations

import numpy as np

from data_refs import episode_lengths, lowbias32, make_store, stream_seed  # noqa: F401  (make_store / episode_lengths: re-exported for the tests)

LAST = 2 ** 31 - 1          # the horizon data.WindowSweep(goal_horizon="last") passes: past the end of every episode
FULL = 2 ** 32              # thresh of hindsight_prob = 1


def step_goal_table(eps, G: int, seed: int = 1):
    """One [L, G] fp32 table of per-step goal embeddings per episode of the test store."""
    rng = np.random.default_rng(1000 + seed)
    return [rng.standard_normal((e[0].shape[0], G)).astype(np.float32) for e in eps]


def bf16_bits(x):
    """fp32 -> bf16 bits (uint16), round to nearest even (finite values)."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> np.uint64(16)) & np.uint64(1))) >> np.uint64(16)).astype(np.uint16)


def bf16_expand(bits):
    """bf16 bits -> fp32, exactly: bits << 16."""
    return (np.asarray(bits, dtype=np.uint16).astype(np.uint32) << np.uint32(16)).view(np.float32)


def thresh_of(prob: float) -> int:
    return int(round(prob * 2.0 ** 32))


def draws(seed: int, step: int, ids, lo: int, hi: int, thresh: int):
    """(kind [B] bool, d [B] int64) of the rows with the given ids (uint32 values)."""
    ids = np.asarray(ids, dtype=np.int64).astype(np.uint64) & np.uint64(0xFFFFFFFF)
    k4, k5 = stream_seed((seed + 4) & 0xFFFFFFFF, step), stream_seed((seed + 5) & 0xFFFFFFFF, step)
    kind = lowbias32(np.uint64(k5) ^ ids) < np.uint64(thresh)
    d = lo + ((lowbias32(np.uint64(k4) ^ ids) * np.uint64(hi - lo + 1)) >> np.uint64(32)).astype(np.int64)
    return kind, d


def relabel(begin, index, episode, seed: int, step: int, lo: int, hi: int, thresh: int, ids=None):
    """begin [E + 1]: the episodes' first rows; index, episode [B]: what the sampling launch wrote; ids None: id = j.
    -> dict(goal_index, goal_offset int32 [B], goal_kind fp32 [B], d int64 [B], last int64 [B])."""
    begin = np.asarray(begin, dtype=np.int64)
    index, episode = np.asarray(index, dtype=np.int64), np.asarray(episode, dtype=np.int64)
    B = index.shape[0]
    kind, d = draws(seed, step, np.arange(B) if ids is None else ids, lo, hi, thresh)
    last = begin[episode + 1] - 1
    r = np.minimum(index + d, last)
    return dict(goal_index=r.astype(np.int32), goal_offset=(r - index).astype(np.int32), goal_kind=kind.astype(np.float32), d=d, last=last)


def relabelled_goals(latent_goal, step_goals, ref):
    """latent_goal [B, G] fp32 (the episode goals the sampling launch wrote), step_goals [S, G] fp32 (for a bf16 store: bf16_expand of its bits)
    -> the rows with goal_kind = 1 replaced by step_goals[goal_index], the others untouched."""
    out = np.array(latent_goal, dtype=np.float32, copy=True)
    on = ref["goal_kind"] == 1
    out[on] = np.asarray(step_goals, dtype=np.float32)[ref["goal_index"][on]]
    return out
