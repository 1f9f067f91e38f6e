"""CPU: the numpy restatement of the ordered draws (tests/order_refs.py) against what include/mode_hip.h promises of
mode_data_sample_windows_ordered - the epoch permutation is a bijection of good quality, the cut table of a weighted mixture never selects an
episode without mass - and the host side of data.WindowStream(order=, episode_weights=) and data.mixture_weights.  No kernel is launched here."""
import math
from fractions import Fraction

import numpy as np
import pytest

import data_refs as R
import order_refs as O
from mode_diffusion_policy_amd import data

W = 4
SIZES = (1, 2, 3, 5, 6, 16, 17, 64, 65, 1000, 4097, 2 ** 16, 2 ** 16 + 1)
SEEDS = (0, 1, 2)


def test_round_count_and_header_agree():
    import os
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mode_hip.h")).read()
    assert f"#define MODE_PERM_ROUNDS {O.ROUNDS}\n" in header and 6 <= O.ROUNDS <= 10
    assert f"#define MODE_ORDER_EPOCH {O.EPOCH}\n" in header and f"#define MODE_ORDER_WEIGHTED {O.WEIGHTED}\n" in header


def test_perm_bits():
    assert [O.perm_bits(n) for n in (1, 2, 3, 4, 5, 16, 17, 64, 65, 4097, 2 ** 16, 2 ** 16 + 1, 2 ** 31 - 1)] == [2, 2, 2, 2, 4, 4, 6, 6, 8, 14, 16, 18, 32]
    for n in range(2, 300):
        assert (1 << O.perm_bits(n)) < 4 * n and (1 << O.perm_bits(n)) >= n                     # the walk's domain: n <= 2^bits < 4 n


def test_perm_is_a_bijection():
    """(a) every size, seeds 0 / 7 / 2^32 - 3 (seed + 6 wraps) and epochs 0, 1, 5, 2^32 - 1, 2^32 and 2^32 + 5 (ep_hi != 0).  The longest walk
    seen: 54 applications, at n = 2^16 + 1 (domain 2^18, almost 4 n); 41 at n = 4097, 24 at 65, 16 at 17, 9 at 5 and 6."""
    longest = {}
    for n in SIZES:
        for seed in (0, 7, 2 ** 32 - 3):
            for ep in (0, 1, 5, 2 ** 32 - 1, 2 ** 32, 2 ** 32 + 5):
                g, walk = O.perm(seed, ep, n, walks=True)
                assert g.min() == 0 and g.max() == n - 1 and len(np.unique(g)) == n, (n, seed, ep)
                longest[n] = max(longest.get(n, 0), int(walk.max()))
    print("longest walks:", longest)
    assert longest[16] == 1 and longest[64] == 1 and longest[2 ** 16] == 1                      # n = 2^bits: no walk
    assert max(longest.values()) <= 64                 # (an application lands inside with probability > 1 / 4: a walk past 64 has probability < 1e-8)
    # single places agree with the whole permutation (the kernel evaluates one place per row)
    full = O.perm(3, 2, 1000)
    assert np.array_equal(O.perm(3, 2, 1000, [0, 999, 500]), full[[0, 999, 500]])


def test_perm_quality_of_the_chosen_round_count():
    """(b) with ROUNDS = 10, seeds 0 / 1 / 2, epochs 0 .. T - 1:
        place-occupancy chi-square, n = 6, T = 6000 (uniform: 30, sd 7.07):        37.3, 35.9, 28.2   (+1.03, +0.84, -0.25 sd)
        place-occupancy chi-square, n = 37, T = 3700 (uniform: 1332, sd 50.9):     1294.5, 1339.3, 1340.3   (-0.74, +0.14, +0.16 sd)
        neighbours that stay neighbours, n = 1000, T = 200 (uniform: 199.8 of 199800, sd 14.1):   210, 187, 208   (+0.72, -0.91, +0.58 sd)
    The same statistics with 6 rounds: chi-square at n = 6 of 47.6, 53.9, 47.7 (+2.5, +3.4, +2.5 sd: inside the bound, but all on one side);
    8 rounds: 23.2, 57.2, 25.2 (one at +3.8 sd).  Every bound is 4 standard deviations of the uniform permutation's statistic."""
    for seed in SEEDS:
        for n, T in ((6, 6000), (37, 3700)):
            chi = O.place_chi_square(seed, n, T)
            print(f"seed {seed} n {n}: chi-square {chi:.1f}, expected {n * (n - 1)}, sd {math.sqrt(2) * (n - 1):.1f}")
            assert abs(chi - n * (n - 1)) <= 4 * math.sqrt(2) * (n - 1), (seed, n, chi)
        n, T = 1000, 200
        hits, trials = O.successor_count(seed, n, T), T * (n - 1)
        sd = math.sqrt(trials * (1 / n) * (1 - 1 / n))
        print(f"seed {seed} n {n}: {hits} successors of {trials}, expected {trials / n:.1f}, sd {sd:.1f}")
        assert abs(hits - trials / n) <= 4 * sd, (seed, hits)
    assert np.array_equal(O.perm_epochs(1, 4, 37)[3], O.perm(1, 3, 37))                         # the statistics' batched form is perm() itself


def test_epochs_and_seeds_give_different_permutations():
    """(c)"""
    for n in (6, 37, 4097):
        perms = {(seed, ep): tuple(O.perm(seed, ep, n)) for seed in SEEDS for ep in (0, 1, 2, 2 ** 32, 2 ** 32 + 1)}
        assert len(set(perms.values())) == len(perms), n
    assert O.epoch_key(0, 2 ** 32) != O.epoch_key(0, 0) and O.epoch_key(0, 2 ** 32) == R.stream_seed((6 + R.GOLDEN) & O.M32, 0)


def test_epoch_rows_cover_every_window_once_and_straddle_boundaries():
    for n, B in ((15, 4), (15, 7), (5, 4), (16, 7), (1, 4)):
        seen = {}
        for t in range(0, (6 * n) // B + 2):
            ep, q, g = O.epoch_rows(9, t, B, n)
            assert np.array_equal(ep * n + q, t * B + np.arange(B))
            for e, x in zip(ep.tolist(), g.tolist()):
                seen.setdefault(e, []).append(x)
        for e in range(6):
            assert sorted(seen[e]) == list(range(n)), (n, B, e)
    ep, q, g = O.epoch_rows(0, 2 ** 32 - 1, 7, 1)                                               # 64-bit positions, ep_hi != 0 at n = 1
    assert ep.tolist() == [(2 ** 32 - 1) * 7 + j for j in range(7)] and ep[0] >= 2 ** 32 and not q.any() and not g.any()


# ---------------------------------------------------------------------------------------------------------------- weighted mixtures
MASSES = ((0, 1, 0, 3), (2, 1, 3, 0), (0, 0, 5, 0), (1, 1, 1, 1), (1e-3, 7.5, 0, 2.25), (0, 3, 0, 0, 1, 0, 0, 2, 0), (1.0,), (1, 2 ** 31))


def test_cut_table_is_monotone_and_never_selects_a_zero_mass_episode():
    """(d)"""
    for mass in MASSES:
        m = np.asarray(mass, dtype=np.float64)
        E, cut = len(m), O.cut_table(m)
        assert cut.dtype == np.int64 and len(cut) == E + 1 and cut[0] == 0 and cut[E] == 2 ** 32 and (np.diff(cut) >= 0).all()
        C = np.concatenate([[0.0], np.cumsum(m)])
        assert [int(c) for c in cut[:-1]] == [math.floor(2.0 ** 32 * (C[e] / C[E])) for e in range(E)]              # the stated floors
        assert np.array_equal(np.diff(cut), np.array([cut[e + 1] - cut[e] for e in range(E)])) and (np.diff(cut)[m == 0] == 0).all()
        assert (np.diff(cut)[m > 0] > 0).all()
        probes = {0, 2 ** 32 - 1} | {int(c) for c in cut if c < 2 ** 32} | {int(c) - 1 for c in cut if c > 0}
        for r in sorted(probes):
            e = R.locate(r, cut)
            assert 0 <= e < E and m[e] > 0 and cut[e] <= r < cut[e + 1], (mass, r, e)
    # the draw: an episode's share of 2^32 is its share of the mass to within one unit, and p stays inside the episode
    cut = O.cut_table(np.array([0.0, 1.0, 0.0, 3.0]))
    assert cut.tolist() == [0, 0, 2 ** 30, 2 ** 30, 2 ** 32]
    e, p = O.weighted_rows(5, 3, 4096, cut, np.array([1, 3, 4, 7]))
    assert set(e.tolist()) == {1, 3} and abs(int((e == 1).sum()) - 1024) <= 5 * math.sqrt(4096 * 0.25 * 0.75)
    assert p[e == 1].min() == 0 and p[e == 1].max() == 2 and p[e == 3].min() == 0 and p[e == 3].max() == 6


def cpu_store(lengths=(1, 3, 4, 7), A=3, G=5):
    st = data.EpisodeStore(A, G, device="cpu")
    for L in lengths:
        st.add_episode(np.zeros((L, A), np.float32), np.zeros(G, np.float32))
    return st.finalize(None)


def test_the_host_table_is_the_reference_table():
    st = cpu_store()
    for w, pad, episodes in (((0, 1, 0, 3), "hold", None), ((2, 1, 3, 0), "hold", None), ((1, 1, 1, 1), "none", None), ((5, 1, 2, 3), "hold", [1, 2, 3]),
                             ((1e-3, 7.5, 0, 2.25), "hold", [0, 1, 3])):
        ws = data.WindowStream(st, 8, W, pad=pad, episodes=episodes, episode_weights=w)
        n_e = O.start_counts([1, 3, 4, 7], W, pad, episodes)
        assert ws.cut.dtype.is_floating_point is False and ws.cut.tolist() == O.cut_table(O.episode_mass(w, n_e)).tolist(), (w, pad, episodes)
        assert ws.order == "iid" and ws.starts.tolist() == np.concatenate([[0], np.cumsum(n_e)]).tolist()
    plain = data.WindowStream(st, 8, W)
    assert plain.cut is None and plain.order == "iid"


def test_refusals_need_no_device():
    """(d) / GPU case 7: every refusal is a ValueError out of the constructor, on a store that has no device at all."""
    st = cpu_store()
    ok = dict(batch_size=8, window=W)
    for order in ("EPOCH", "shuffle", "", None, 1, True):
        with pytest.raises(ValueError, match="order"):
            data.WindowStream(st, **ok, order=order)
    bad_w = ((1, 1, 1), (1, 1, 1, 1, 1), (1, -1, 1, 1), (1, float("nan"), 1, 1), (1, float("inf"), 1, 1), (0, 0, 0, 0), "abcd", ((1, 1), (1, 1)),
             (True, False, True, True), 3.0, (1e-30, 1, 1, 1), (1e308, 1e308, 1e308, 1e308))
    for w in bad_w:
        with pytest.raises(ValueError, match="episode_weights"):
            data.WindowStream(st, **ok, episode_weights=w)
    with pytest.raises(ValueError, match="episode_weights"):                                      # all the mass on episodes without a start
        data.WindowStream(st, **ok, pad="none", episode_weights=(1, 1, 0, 0))
    with pytest.raises(ValueError, match="episode_weights"):                                      # ... or on an episode that is not listed
        data.WindowStream(st, **ok, episodes=[0, 1], episode_weights=(0, 0, 1, 1))
    with pytest.raises(ValueError, match="order='iid'"):
        data.WindowStream(st, **ok, order="epoch", episode_weights=(1, 1, 1, 1))
    ws = data.WindowStream(st, **ok, order="epoch")
    with pytest.raises(ValueError, match="ROCm"):
        ws.batch(0)                                                                               # there is no CPU path
    for step in (-1, 2 ** 32, 1.5, True):
        with pytest.raises(ValueError, match="step"):
            ws.epoch_of(step)


def test_epoch_helpers():
    st = cpu_store()
    ws = data.WindowStream(st, 4, W, order="epoch")
    assert ws.n_total == 15 and ws.steps_per_epoch == Fraction(15, 4) and isinstance(ws.steps_per_epoch, Fraction)
    assert [ws.epoch_of(t) for t in range(9)] == [0, 0, 0, 0, 1, 1, 1, 1, 2] and ws.epoch_of(2 ** 32 - 1) == ((2 ** 32 - 1) * 4) // 15
    assert math.ceil(30 * ws.steps_per_epoch) == 113                                              # "train 30 epochs"
    for t in (0, 3, 4, 113, 2 ** 32 - 1):
        assert ws.epoch_of(t) == int(O.epoch_rows(0, t, 4, 15)[0][0])
    assert data.WindowStream(st, 5, W, pad="none", episodes=[3]).steps_per_epoch == Fraction(4, 5)


def test_mixture_weights_arithmetic():
    """(e) w_e = p_d n_e / N_d: the group's share of the cut table is p_d, an episode's share of its group n_e / N_d."""
    st = cpu_store((1, 3, 4, 7, 10))
    groups = [0, 1, 0, 1, 2]
    w = data.mixture_weights(st, groups, (1.0, 2.0, 1.0))
    assert w.dtype == np.float64 and np.allclose(w, [0.25 * 1 / 5, 0.5 * 3 / 10, 0.25 * 4 / 5, 0.5 * 7 / 10, 0.25], rtol=1e-15, atol=0)
    assert math.isclose(w.sum(), 1.0, rel_tol=1e-15) and math.isclose(w[[1, 3]].sum(), 0.5, rel_tol=1e-15)
    # pad="none" counts the starts the stream will see; an episode without one gets no weight
    w = data.mixture_weights(st, groups, (3, 1, 0), window=W, pad="none")
    assert np.allclose(w, [0, 0, 0.75, 0.25, 0], rtol=1e-15, atol=0)
    # episodes= leaves an episode out of its group's N_d
    w = data.mixture_weights(st, groups, (1, 1, 2), episodes=[0, 1, 3, 4])
    assert np.allclose(w, [0.25, 0.25 * 3 / 10, 0, 0.25 * 7 / 10, 0.5], rtol=1e-15, atol=0)
    # the weights go straight into a stream: the groups' shares of [0, 2^32) are p_d to within a unit per episode
    ws = data.WindowStream(st, 8, W, episodes=[0, 1, 3, 4], episode_weights=w)
    share = np.diff(np.asarray(ws.cut.tolist(), dtype=np.float64)) / 2.0 ** 32
    assert abs(share[[0, 2]].sum() - 0.25) < 1e-8 and abs(share[[1, 3]].sum() - 0.25) < 1e-8 and abs(share[4] - 0.5) < 1e-8 and share[2] == 0
    # per-start weights, the docstring's recipe: s = 1 is the uniform draw over the starts
    uni = data.WindowStream(st, 8, W, episode_weights=st.lengths)
    assert np.abs(np.asarray(uni.cut.tolist()) - np.floor(2.0 ** 32 * np.concatenate([[0], np.cumsum(st.lengths)]) / 25)).max() <= 1
    for bad in (dict(groups=[0, 1, 0, 1]), dict(groups=[0, 1, 0, 1, 3]), dict(groups=[0, 1, 0, 1, -1]), dict(groups=[0.0, 1, 0, 1, 2]),
                dict(group_weights=(1, -1, 1)), dict(group_weights=(0, 0, 0)), dict(group_weights=(1, float("nan"), 1)), dict(group_weights=()),
                dict(group_weights=(1, 1, 1), episodes=[0, 1, 2, 3]),                               # group 2 has weight but no start
                dict(pad="none"), dict(pad="zero"), dict(window=0, pad="none")):
        with pytest.raises(ValueError):
            data.mixture_weights(st, **{**dict(groups=groups, group_weights=(1.0, 2.0, 1.0)), **bad})
    with pytest.raises(ValueError, match="finalized"):
        data.mixture_weights(data.EpisodeStore(3, 5, device="cpu"), [], ())


def test_reference_batch_keeps_the_default_and_the_keyed_draws():
    """sample_windows_ordered without the keywords is data_refs.sample_windows, and u / shifts are the same in every mode."""
    eps = R.make_store(W, 3, 8, seed=2)
    base = R.sample_windows(eps, W, 7, 11, 5, "hold", shift_pads=(2, 0))
    same = O.sample_windows_ordered(eps, W, 7, 11, 5, "hold", shift_pads=(2, 0))
    for k in ("index", "episode", "action_mask", "actions", "latent_goal", "u"):
        assert np.array_equal(base[k], same[k]), k
    ep = O.sample_windows_ordered(eps, W, 7, 11, 5, "hold", shift_pads=(2, 0), order="epoch")
    wt = O.sample_windows_ordered(eps, W, 7, 11, 5, "hold", shift_pads=(2, 0), episode_weights=(0, 1, 0, 3))
    for b in (ep, wt):
        assert np.array_equal(b["u"], base["u"]) and np.array_equal(b["shifts"][0], base["shifts"][0]) and b["shifts"][1] is None
    assert ep["epoch"].tolist() == [2, 2, 2, 2, 2, 2, 2] and ep["position"].tolist() == list(range(5, 12)) and "epoch" not in wt
    assert set(wt["episode"].tolist()) <= {1, 3} and not np.array_equal(ep["index"], base["index"])
