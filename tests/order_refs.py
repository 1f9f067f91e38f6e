"""Numpy restatement of the ordered draws of the training batch stream as include/mode_hip.h states them (mode_data_sample_windows_ordered): the
epoch permutation (a balanced Feistel network with cycle walking, keyed by seed and epoch), the integer cut table of a weighted episode mixture,
both draws, and the batch they give on top of the row logic and the u / shifts draws of tests/data_refs.py.  Validated without a GPU by
tests/test_order_references.py; the GPU tests compare the kernel against it bit for bit."""
from __future__ import annotations

import numpy as np

import data_refs as R
from data_refs import GOLDEN, lowbias32, stream_seed

M32 = 0xFFFFFFFF
ROUNDS = 10                 # MODE_PERM_ROUNDS of include/mode_hip.h
EPOCH, WEIGHTED = 1, 2      # MODE_ORDER_EPOCH, MODE_ORDER_WEIGHTED


# ---------------------------------------------------------------------------------------------------------------- the epoch permutation
def perm_bits(n: int) -> int:
    """The smallest even number >= max(2, bit length of n - 1)."""
    b = max(2, int(n - 1).bit_length())
    return b + (b & 1)


def epoch_key(seed: int, ep: int) -> int:
    """ke = mode_stream_seed(seed + 6 + ep_hi * 0x9E3779B9, ep_lo), the sum and product modulo 2^32."""
    ep_lo, ep_hi = ep & M32, (ep >> 32) & M32
    return stream_seed((seed + 6 + ep_hi * GOLDEN) & M32, ep_lo)


def feistel(v, ke: int, h: int, rounds: int = ROUNDS):
    """One application of the network to an array of values < 2^(2 h): `rounds` times (L, R) -> (R, L ^ (lowbias32(ke ^ (R | (r << 16))) & mask))."""
    v = np.asarray(v, dtype=np.uint64)
    mask = np.uint64((1 << h) - 1)
    L, Rr = v >> np.uint64(h), v & mask
    for r in range(rounds):
        L, Rr = Rr, L ^ (lowbias32(np.asarray(ke, dtype=np.uint64) ^ (Rr | np.uint64(r << 16))) & mask)
    return (L << np.uint64(h)) | Rr


def perm(seed: int, ep: int, n: int, q=None, rounds: int = ROUNDS, walks: bool = False):
    """perm(seed, ep, n)(q) for the places q (default: all of [0, n)) as int64; with walks=True also the number of applications each place took."""
    q = np.arange(n, dtype=np.uint64) if q is None else np.asarray(q, dtype=np.uint64)
    assert q.size == 0 or int(q.max()) < n
    h, ke = perm_bits(n) // 2, epoch_key(seed, ep)
    v = feistel(q, ke, h, rounds)
    steps = np.ones(q.shape, dtype=np.int64)
    out = v >= np.uint64(n)
    while out.any():
        v[out] = feistel(v[out], ke, h, rounds)
        steps[out] += 1
        assert int(steps.max()) <= 1 << (2 * h)                   # the kernel's bound: a walk that starts inside [0, n) never reaches it
        out = v >= np.uint64(n)
    return (v.astype(np.int64), steps) if walks else v.astype(np.int64)


def epoch_rows(seed: int, step: int, B: int, n: int):
    """(epoch, position, g) int64 [B] of the rows of step `step`: P = step * B + j, ep = P div n, q = P mod n, g = perm(seed, ep, n)(q)."""
    P = [step * B + j for j in range(B)]                          # Python ints: 64 bits and more
    ep, q = np.array([p // n for p in P], dtype=np.int64), np.array([p % n for p in P], dtype=np.int64)
    g = np.zeros(B, dtype=np.int64)
    for e in np.unique(ep):
        rows = ep == e
        g[rows] = perm(seed, int(e), n, q[rows])
    return ep, q, g


# ---------------------------------------------------------------------------------------------------------------- weighted episode mixtures
def episode_mass(weights, n_e):
    """The mass of episode e: its weight where it has a start (n_e > 0: it is listed and a window fits), else 0; fp64."""
    w, n_e = np.asarray(weights, dtype=np.float64), np.asarray(n_e, dtype=np.int64)
    return np.where(n_e > 0, w, 0.0)


def cut_table(mass):
    """cut [E + 1] int64: cut[e] = floor(2^32 * (C_e / C_E)) with C the fp64 running sum of the masses in episode order (C_0 = 0), cut[E] = 2^32."""
    C = np.concatenate([[0.0], np.cumsum(np.asarray(mass, dtype=np.float64))])
    cut = np.floor(2.0 ** 32 * (C / C[-1])).astype(np.int64)
    cut[-1] = 2 ** 32
    return cut


def weighted_rows(seed: int, step: int, B: int, cut, n_e):
    """(episode, p) int64 [B]: r1 = lowbias32(k ^ j), k = mode_stream_seed(seed, step), the largest e with cut[e] <= r1 (the binary search of
    data_refs.locate on the int64 table); r2 = lowbias32(mode_stream_seed(seed + 7, step) ^ j), p = (r2 * n_e) >> 32."""
    j = np.arange(B, dtype=np.uint64)
    r1 = lowbias32(np.uint64(stream_seed(seed, step)) ^ j)
    r2 = lowbias32(np.uint64(stream_seed((seed + 7) & M32, step)) ^ j)
    e = np.array([R.locate(int(r), cut) for r in r1], dtype=np.int64)
    p = ((r2 * np.asarray(n_e, dtype=np.uint64)[e]) >> np.uint64(32)).astype(np.int64)
    return e, p


# ---------------------------------------------------------------------------------------------------------------- the batch
def start_counts(lengths, W: int, pad: str, episodes=None):
    """n_e [E] int64: the starts of every episode, 0 for one that `episodes` (None = all) does not list."""
    lengths = np.asarray(lengths, dtype=np.int64)
    n_e = lengths if pad == "hold" else np.maximum(0, lengths - W + 1)
    if episodes is not None:
        keep = np.zeros(len(lengths), dtype=bool)
        keep[np.asarray(episodes, dtype=np.int64)] = True
        n_e = np.where(keep, n_e, 0)
    return n_e.astype(np.int64)


def sample_windows_ordered(eps, W: int, B: int, seed: int, step: int, pad: str, norm=None, shift_pads=(0, 0), order="iid", episode_weights=None,
                           episodes=None):
    """The batch of `step` of data.WindowStream(order=, episode_weights=, episodes=): the keys of data_refs.sample_windows - u and shifts are that
    function's own, the rows follow its row logic from the (episode, p) the ordered draw locates - plus epoch / position int64 [B] for
    order="epoch"."""
    assert order in ("iid", "epoch") and not (order == "epoch" and episode_weights is not None)
    out = R.sample_windows(eps, W, B, seed, step, pad, norm, shift_pads)                     # u and shifts: keyed by (seed, step, j) in every mode
    lengths = [e[0].shape[0] for e in eps]
    begin = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    acts, goals = np.concatenate([e[0] for e in eps]), np.stack([e[1] for e in eps])
    n_e = start_counts(lengths, W, pad, episodes)
    starts = np.concatenate([[0], np.cumsum(n_e)]).astype(np.int64)
    n = int(starts[-1])
    if order == "epoch":
        out["epoch"], out["position"], g = epoch_rows(seed, step, B, n)
        ep_of = np.array([R.locate(int(x), starts) for x in g], dtype=np.int64)
        p = g - starts[ep_of]
    elif episode_weights is not None:
        ep_of, p = weighted_rows(seed, step, B, cut_table(episode_mass(episode_weights, n_e)), n_e)
    else:
        g = R.draw_starts(seed, step, B, n)
        ep_of = np.array([R.locate(int(x), starts) for x in g], dtype=np.int64)
        p = g - starts[ep_of]
    for j in range(B):
        e = int(ep_of[j])
        idx, last = int(begin[e] + p[j]), int(begin[e + 1] - 1)
        assert begin[e] <= idx <= last and n_e[e] > 0 and 0 <= p[j] < n_e[e]
        out["index"][j], out["episode"][j] = idx, e
        for w in range(W):
            x = acts[min(idx + w, last)]
            out["action_mask"][j, w] = 1.0 if idx + w <= last else 0.0
            out["actions"][j, w] = x if norm is None else (x - norm[0]) * norm[1] - np.float32(1.0)      # fp32 numpy: each operation rounded, none fused
        out["latent_goal"][j] = goals[e]
    return out


# ---------------------------------------------------------------------------------------------------------------- statistics of the permutation
def perm_epochs(seed: int, epochs: int, n: int, rounds: int = ROUNDS):
    """[epochs, n] int64: row ep is perm(seed, ep, n) of all places, for ep = 0 .. epochs - 1 - the expressions of perm() with one key per row."""
    h = perm_bits(n) // 2
    ke = np.array([epoch_key(seed, ep) for ep in range(epochs)], dtype=np.uint64)[:, None]
    step = lambda v, k: feistel(v, k, h, rounds)                   # (feistel broadcasts an array of keys like a single one)
    v = step(np.broadcast_to(np.arange(n, dtype=np.uint64), (epochs, n)), ke)
    kk = np.broadcast_to(ke, v.shape)
    out = v >= np.uint64(n)
    while out.any():
        v[out] = step(v[out], kk[out])
        out = v >= np.uint64(n)
    return v.astype(np.int64)


def place_chi_square(seed: int, n: int, epochs: int, rounds: int = ROUNDS) -> float:
    """Chi-square of the n x n table count[q][g] over the epochs 0 .. epochs - 1 against epochs / n per cell: n (n - 1) on average for uniform
    permutations (every cell is binomial(epochs, 1 / n): variance over mean = 1 - 1 / n, times n^2 cells)."""
    g = perm_epochs(seed, epochs, n, rounds)
    count = np.bincount((np.arange(n)[None, :] * n + g).ravel(), minlength=n * n)
    want = epochs / n
    return float(((count - want) ** 2).sum() / want)


def successor_count(seed: int, n: int, epochs: int, rounds: int = ROUNDS) -> int:
    """How many of the epochs * (n - 1) neighbouring places (q, q + 1) get neighbouring windows, perm(q + 1) == perm(q) + 1: each with
    probability 1 / n under a uniform permutation."""
    g = perm_epochs(seed, epochs, n, rounds)
    return int((g[:, 1:] == g[:, :-1] + 1).sum())
