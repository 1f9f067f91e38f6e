"""Numpy restatement of the validation sweep and the masked action error as include/mode_hip.h states them (mode_data_sweep_windows,
mode_action_error): the enumeration of the windows, the row body of the training stream (tests/data_refs.py: the same search, padding and unfused
fp32 normalisation), and the error sums in fp64 in the kernel's stated order - lane by lane, then the xor butterfly - so that the GPU tests can
compare bit for bit.  Validated without a GPU by tests/test_val_references.py."""
from __future__ import annotations

import numpy as np

import data_refs as R


def window_counts(lengths, W: int, stride: int, pad: str, episodes=None):
    """n_e per episode: ceil(L / stride) (hold) | L >= W ? (L - W) // stride + 1 : 0 (none) | 0 for an episode that is not selected."""
    n = []
    for e, L in enumerate(int(v) for v in lengths):
        if episodes is not None and e not in set(int(v) for v in episodes):
            n.append(0)
        elif pad == "hold":
            n.append(-(-L // stride))
        else:
            n.append((L - W) // stride + 1 if L >= W else 0)
    return np.asarray(n, dtype=np.int64)


def sweep_table(lengths, W: int, stride: int, pad: str, episodes=None):
    return np.concatenate([[0], np.cumsum(window_counts(lengths, W, stride, pad, episodes))]).astype(np.int64)


def num_batches(n_total: int, B: int) -> int:
    return -(-n_total // B)


def sweep_windows(eps, W: int, B: int, i: int, stride: int, pad: str, norm=None, episodes=None):
    """Batch i of the sweep: index, episode, window [B] int32; valid [B], action_mask [B, W], actions [B, W, A], latent_goal [B, G] fp32.
    norm = (lo, scale) fp32 or None.  A row past the end repeats the last window with valid = 0 and a zero mask."""
    lengths = [e[0].shape[0] for e in eps]
    begin = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    acts, goals = np.concatenate([e[0] for e in eps]), np.stack([e[1] for e in eps])
    starts = sweep_table(lengths, W, stride, pad, episodes)
    n_total = int(starts[-1])
    assert 0 <= i * B < n_total
    A = acts.shape[1]
    out = dict(index=np.zeros(B, np.int32), episode=np.zeros(B, np.int32), window=np.zeros(B, np.int32), valid=np.zeros(B, np.float32),
               action_mask=np.zeros((B, W), np.float32), actions=np.zeros((B, W, A), np.float32), latent_goal=np.zeros((B, goals.shape[1]), np.float32))
    for j in range(B):
        live = i * B + j < n_total
        g = min(i * B + j, n_total - 1)
        e = R.locate(g, starts)
        idx = int(begin[e] + stride * (g - starts[e]))
        last = int(begin[e + 1] - 1)
        assert begin[e] <= idx <= last
        out["index"][j], out["episode"][j], out["window"][j], out["valid"][j] = idx, e, g, 1.0 if live else 0.0
        for w in range(W):
            x = acts[min(idx + w, last)]
            out["action_mask"][j, w] = 1.0 if live and idx + w <= last else 0.0
            out["actions"][j, w] = x if norm is None else (x - norm[0]) * norm[1] - np.float32(1.0)      # fp32 numpy: each operation rounded, none fused
        out["latent_goal"][j] = goals[e]
    return out


def window_noise_seeds(seed: int, windows):
    """s_g = (seed + 1 + g * 0x9E3779B9) mod 2^32: the noise of window g is rollout.env_noise([s_g], [draw], W, A, noise_scale)."""
    return [(seed + 1 + int(g) * R.GOLDEN) & 0xFFFFFFFF for g in windows]


# ------------------------------------------------------------------------------------------------------------ masked action error, fp64
def _positive(x, shape):
    if x is None:
        return np.ones(shape, np.float32)
    x = np.asarray(x, np.float32)
    with np.errstate(invalid="ignore"):
        return np.where(x > 0, x, np.float32(0.0)).astype(np.float32)


def _terms(pred, target, mask, weight, unit):
    """c [B, W] fp64 (from the fp32 product) and e [B, W, A] fp64 (from the fp32 difference)."""
    pred, target = np.asarray(pred, np.float32), np.asarray(target, np.float32)
    B, W, A = pred.shape
    with np.errstate(all="ignore"):
        cf = (_positive(weight, (B,))[:, None] * _positive(mask, (B, W))).astype(np.float32)
        d = (pred - target).astype(np.float32)
        e = d.astype(np.float64) if unit is None else d.astype(np.float64) * np.asarray(unit, np.float64)[None, None, :]
    return cf.astype(np.float64), e


def _butterfly(v):
    """[64, ...] lane sums -> what every lane holds after the xor butterfly 32, 16, 8, 4, 2, 1."""
    lanes = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[lanes ^ o]
    return v[0]


def action_error(pred, target, mask=None, weight=None, unit=None, into=None):
    """(sq [W * A], ab [W * A], cnt [W]) fp64 in the kernel's order: lane l adds its terms b = l, l + 64, ... ascending, skipping c == 0; the 64 lane
    sums go through the butterfly; `into` = (sq, ab, cnt) of earlier calls, to which the sums are added (accumulate = 1)."""
    c, e = _terms(pred, target, mask, weight, unit)
    B, W, A = e.shape
    sq, ab, cn = np.zeros((64, W, A)), np.zeros((64, W, A)), np.zeros((64, W))
    with np.errstate(all="ignore"):
        for b in range(B):
            l, cb = b % 64, c[b]
            live = cb > 0
            t2, t1 = cb[:, None] * (e[b] * e[b]), cb[:, None] * np.abs(e[b])
            sq[l] = np.where(live[:, None], sq[l] + t2, sq[l])
            ab[l] = np.where(live[:, None], ab[l] + t1, ab[l])
            cn[l] = np.where(live, cn[l] + cb, cn[l])
        out = (_butterfly(sq).reshape(W * A), _butterfly(ab).reshape(W * A), _butterfly(cn))
        if into is not None:
            out = tuple(o + s for o, s in zip(into, out))
    return out


def action_error_plain(pred, target, mask=None, weight=None, unit=None):
    """The same sums with numpy's own fp64 summation, terms with c == 0 dropped."""
    c, e = _terms(pred, target, mask, weight, unit)
    B, W, A = e.shape
    live = np.broadcast_to((c > 0)[:, :, None], e.shape)
    with np.errstate(all="ignore"):
        t2 = np.where(live, c[:, :, None] * e * e, 0.0)
        t1 = np.where(live, c[:, :, None] * np.abs(e), 0.0)
    return t2.sum(axis=0).reshape(W * A), t1.sum(axis=0).reshape(W * A), c.sum(axis=0)


_SUMS = {3: ("sq", "ab", "cnt"), 2: ("sq", "cnt")}                              # mode_action_error's accumulators | mode_level_error's


def same_sums(got, want, what) -> None:
    """Asserts that the accumulators ``got`` carry the bits of ``want`` (tuples of numpy arrays)."""
    for g, w, name in zip(got, want, _SUMS[len(want)]):
        assert R.same_bits(g, w), (what, name, float(np.abs(g - w).max()) if g.shape == w.shape else (g.shape, w.shape))


def bits(t):
    """A device tensor's elements as a flat array of unsigned words (fp64: 64 bits, else 32)."""
    return t.detach().cpu().numpy().reshape(-1).view(np.uint64 if t.element_size() == 8 else np.uint32)


def same(res, acc) -> bool:
    """A validator's result ``res`` holds the bits of the reference accumulators ``acc``."""
    return all(np.array_equal(bits(res[k]), a.reshape(-1).view(np.uint64)) for k, a in zip(_SUMS[len(acc)], acc))


def held_out_setup(dtype, W: int, A: int, B: int, seed: int, step_goals: bool = False, sweep_kw=None):
    """GPU: the tiny c1e4 denoiser (training mode), the store of data_refs.make_store (episodes of 1, 9, 10 and 13 steps at W = 10: 33 windows) with
    features stored per step, and its sweep -> (den, m, store, sweep, embed)."""
    import torch
    import goal_refs as GR
    import mode_diffusion_policy_amd as M
    from mode_diffusion_policy_amd import data
    from test_gpu_train import build_train
    cfg, sd, m = build_train("c1e4", 210, dtype)
    den = M.GCDenoiser(m, 0.5).train()
    eps = R.make_store(W, A, cfg.goal_dim, seed=3)
    sg = GR.step_goal_table(eps, cfg.goal_dim) if step_goals else [None] * len(eps)
    st = data.EpisodeStore(A, cfg.goal_dim)
    for e, s in zip(eps, sg):
        st.add_episode(e[0], e[1], step_goals=s)
    st.finalize("minmax")
    feats = torch.randn(st.num_steps, cfg.n_img_tokens, cfg.obs_dim, device="cuda", generator=torch.Generator(device="cuda").manual_seed(1))
    embed = lambda b: {"state_images": feats[b["index"].long()]}
    return den, m, st, data.WindowSweep(st, B, W, seed=seed, **(sweep_kw or {})), embed
