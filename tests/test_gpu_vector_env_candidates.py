"""rollout.VectorEnvPolicy(candidates=N) on the MI355X (c1e4 weights, oracle.weights): the select kernel against the fp64 restatement of
tests/cand_refs.py, the candidate gathers against env_noise / env_warm_latents, replans against "the fused sampler on the gathered candidate
batch, then select_coherent" (bit for bit), the default path against a policy built without the keyword, the combinations with warm_start,
temporal_ensemble and raw frames, and the capture / replay / sync / memory budget."""
import ctypes as C
import gc

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from mode_diffusion_policy_amd import _lib as L  # noqa: E402
from mode_diffusion_policy_amd import rollout  # noqa: E402

import cand_refs as R  # noqa: E402
from test_gpu_vector_env_camera import TRANSFORMS, u8_frames  # noqa: E402
from test_gpu_vector_env_frames import encoders, frames, rows_of, tokens  # noqa: E402
from test_gpu_vector_env_warm import SAMPLERS, SIGMA_MAX, _drain, build, count_graphs, obs, policy  # noqa: E402

SENTINEL, ISENT, GUARD = -12345.0, -77, 64
U32 = 0xFFFFFFFF
_stream = lambda: torch.cuda.current_stream().cuda_stream


def guarded(n, fill=SENTINEL, dtype=torch.float32):
    """(n-element view, its buffer) with GUARD words of ``fill`` in front of and behind the view, the view filled too."""
    buf = torch.full((2 * GUARD + n,), fill, dtype=dtype, device="cuda")
    return buf[GUARD:GUARD + n], buf


def guards_intact(buf, n, fill=SENTINEL):
    return bool((buf[:GUARD] == fill).all() and (buf[GUARD + n:] == fill).all())


# ------------------------------------------------------------------------------------------------------------------ 1. the select kernel
NUM_ENVS = R.CASE_ENVS
ROWS = [3, 0, 2, -1, NUM_ENVS, 4, 1, 1, 1]                                            # two entries out of range; padding by repetition; env 5 not listed


def _select(rows, cands, prev, has_prev, shift, wt):
    """mode_env_select on sentinel-filled outputs with guard words: cands [num_envs, N, W, A] (chunk row j = the candidates of rows[j], zeros
    for an out-of-range entry), prev [num_envs, W, A].  Returns (chunk [m_b, N, W, A], chosen [m_b, W, A], selected [num_envs],
    scores [num_envs, N], guards intact)."""
    n, N, W, A = cands.shape
    mb = len(rows)
    chunk = torch.stack([cands[r] if 0 <= r < n else torch.zeros_like(cands[0]) for r in rows]).contiguous()
    r = torch.tensor(rows, dtype=torch.int32, device="cuda")
    mask = torch.from_numpy(rollout._mask_words(np.asarray(has_prev, dtype=bool), (n + 31) // 32).view("<i4").copy()).cuda()
    w = torch.from_numpy(np.asarray(wt, dtype=np.float32)).cuda()
    chosen, b0 = guarded(mb * W * A)
    selected, b1 = guarded(n, ISENT, torch.int32)
    scores, b2 = guarded(n * N)
    d = L.ModeEnvSelectDesc(rows=r.data_ptr(), has_prev=mask.data_ptr(), count=None, chunk=chunk.data_ptr(), plan=prev.data_ptr(), weights=w.data_ptr(),
                            chosen=chosen.data_ptr(), selected=selected.data_ptr(), scores=scores.data_ptr(), m_b=mb, num_envs=n, W=W, A=A,
                            shift=shift, N=N)
    L.check(L.load().mode_env_select(C.byref(d), _stream()), "env_select")
    torch.cuda.synchronize()
    ok = guards_intact(b0, mb * W * A) and guards_intact(b1, n, ISENT) and guards_intact(b2, n * N)
    return chunk, chosen.view(mb, W, A), selected, scores.view(n, N), ok


@pytest.mark.parametrize("W,A,shift,N", R.SHAPES)
def test_select_matches_restatement(W, A, shift, N):
    """Every fp32 score within (n + 4) 2^-24 relative of the fp64 score, n = L * A (cand_refs.score_bound: derived, not measured); the selected
    candidate's fp64 score within (1 + 2 bound) of the fp64 minimum, always; equal to the fp64 argmin wherever the fp64 gap between the two
    best exceeds 2 bound (tests/test_vector_env_candidates.py pins that this covers >= 95 % of these seeded rows)."""
    c_np, p_np = R.make_case(R.case_rng(W, A, shift), NUM_ENVS, N, W, A, shift)
    cands, prev = torch.from_numpy(c_np).cuda(), torch.from_numpy(p_np).cuda()
    L_, bound = W - shift, R.score_bound(W - shift, A)
    wt = rollout.coherence_weights(R.RHO, L_)
    chunk, chosen, selected, scores, ok = _select(ROWS, cands, prev, [True] * NUM_ENVS, shift, wt)
    assert ok
    sel, sc = selected.cpu().numpy(), scores.cpu().double().numpy()
    listed = sorted({r for r in ROWS if 0 <= r < NUM_ENVS})
    for r in range(NUM_ENVS):
        if r not in listed:                                                               # an environment nobody listed: untouched
            assert sel[r] == ISENT and (scores[r] == SENTINEL).all(), r
    worst, exact = 0.0, 0
    for j, r in enumerate(ROWS):
        if not 0 <= r < NUM_ENVS:
            assert (chosen[j] == SENTINEL).all(), j                                       # untouched
            continue
        ref = R.scores64(c_np[r], p_np[r], shift, R.RHO)
        err = np.abs(sc[r] - ref) / ref
        worst = max(worst, float(err.max()))
        assert np.all(err <= bound), (j, r, float(err.max()), bound)
        assert 0 <= sel[r] < N and ref[sel[r]] <= ref.min() * (1.0 + 2.0 * bound), (j, r)
        if R.decisive(ref, bound):
            exact += 1
            assert sel[r] == R.select(ref) == int(np.argmin(ref)), (j, r)
        assert torch.equal(chosen[j], chunk[j, sel[r]]), (j, r)                           # the winner's rows, bit for bit
    print(f"select W={W} A={A} shift={shift} N={N}: worst score error / bound = {worst / bound:.3f}; {exact} of {len(ROWS) - 2} rows compared exactly")
    solo = _select([1], cands, prev, [True] * NUM_ENVS, shift, wt)                        # a padded call and a solo call: identical rows
    assert solo[4] and solo[2][1] == selected[1] and torch.equal(solo[3][1], scores[1])
    assert all(torch.equal(solo[1][0], chosen[j]) for j in (6, 7, 8))


def test_select_count_skips_the_rows_behind_it():
    """ModeEnvSelectDesc.count (the control block's m): rows j >= *count are left untouched, as warmup's captures need."""
    W, A, s, N = 10, 7, 4, 4
    c_np, p_np = R.make_case(R.case_rng(W, A, s), 3, N, W, A, s)
    chunk, prev = torch.from_numpy(c_np).cuda(), torch.from_numpy(p_np).cuda()
    rows, ones = torch.tensor([0, 1, 2], dtype=torch.int32, device="cuda"), torch.full((1,), -1, dtype=torch.int32, device="cuda")
    w = torch.from_numpy(rollout.coherence_weights(0.5, W - s)).cuda()
    full = rollout.select_coherent(chunk, prev, [True] * 3, s, w)
    for m in (0, 2):
        count = torch.tensor([m], dtype=torch.int32, device="cuda")
        chosen, selected, scores = torch.full((3, W, A), SENTINEL, device="cuda"), torch.full((3,), ISENT, dtype=torch.int32, device="cuda"), \
            torch.full((3, N), SENTINEL, device="cuda")
        d = L.ModeEnvSelectDesc(rows=rows.data_ptr(), has_prev=ones.data_ptr(), count=count.data_ptr(), chunk=chunk.data_ptr(), plan=prev.data_ptr(),
                                weights=w.data_ptr(), chosen=chosen.data_ptr(), selected=selected.data_ptr(), scores=scores.data_ptr(), m_b=3,
                                num_envs=3, W=W, A=A, shift=s, N=N)
        L.check(L.load().mode_env_select(C.byref(d), _stream()), "env_select")
        assert torch.equal(chosen[:m], full[0][:m]) and torch.equal(selected[:m], full[1][:m]) and torch.equal(scores[:m], full[2][:m])
        assert (chosen[m:] == SENTINEL).all() and (selected[m:] == ISENT).all() and (scores[m:] == SENTINEL).all()


def test_select_constructed_cases():
    W, A, s, N = 10, 7, 4, 5
    rng = np.random.default_rng(3)
    prev = torch.from_numpy(rng.standard_normal((4, W, A)).astype(np.float32)).cuda()
    tail = prev[:, np.minimum(np.arange(W) + s, W - 1)]
    chunk = tail[:, None] + torch.from_numpy(rng.standard_normal((4, N, W, A)).astype(np.float32)).cuda()
    w = rollout.coherence_weights(0.5, W - s)
    # row 0: candidates 1 and 3 identical and the closest -> the lower index;  row 1: no previous plan -> all scores exactly 0, candidate 0;
    # row 2: candidate 0 would win but holds one NaN in a scored element, candidate 4 one in an unscored row (w >= L: harmless);
    # row 3: every candidate holds a NaN -> candidate 0
    chunk[0, 1] = chunk[0, 3] = tail[0] + 1e-3
    chunk[2, 0] = tail[2]
    chunk[2, 0, 2, 3] = float("nan")
    chunk[2, 4, W - 1, 0] = float("nan")
    chunk[3, :, 0, 0] = float("nan")
    chosen, selected, scores = rollout.select_coherent(chunk, prev, [True, False, True, True], s, w)
    sel = selected.cpu().tolist()
    assert sel[0] == 1 and scores[0, 1] == scores[0, 3] and (scores[0, 1] < scores[0, [0, 2, 4]]).all()
    assert sel[1] == 0 and (scores[1] == 0).all() and scores[1].dtype == torch.float32
    ref2 = R.scores64(chunk[2].cpu().numpy(), prev[2].cpu().numpy(), s, 0.5)
    assert np.isnan(ref2[0]) and not np.isnan(ref2[1:]).any() and sel[2] == R.select(ref2) == 1 + int(np.argmin(ref2[1:]))
    assert torch.isnan(scores[2, 0]) and not torch.isnan(scores[2, 1:]).any()
    assert sel[3] == 0 and torch.isnan(scores[3]).all()
    for i in range(4):                                                                    # bit for bit, NaN payloads included
        assert torch.equal(chosen[i].view(torch.int32), chunk[i, sel[i]].view(torch.int32)), i
    # a NaN that is not in front: candidate 2 NaN, the others finite
    chunk[0, 2, 0, 0] = float("nan")
    assert rollout.select_coherent(chunk[:1], prev[:1], [True], s, w)[1].item() == 1


# ------------------------------------------------------------------------------------------------------------------ 2. the candidate gathers
SEEDS, DRAWS = [0, 7, 2 ** 32 - 1, 123456789, 2 ** 20], [0, 3, 2 ** 20, 2 ** 32 - 1, 9]
G_ROWS = [3, 0, 2, -1, 5, 4, 1, 1, 1]


@pytest.mark.parametrize("W,A,N", [(10, 7, 3), (37, 7, 2), (64, 64, 64)])
@pytest.mark.parametrize("warm", [False, True], ids=["noise", "warm"])
def test_candidate_gathers_are_the_single_row_gathers_at_draw_times_n_plus_c(warm, W, A, N):
    n, mb, shift, sigma = 5, len(G_ROWS), 4, 0.37
    rng = np.random.default_rng(W + N)
    plan = torch.from_numpy(rng.standard_normal((n, W, A)).astype(np.float32)).cuda()
    img, goals = torch.from_numpy(rng.standard_normal((n, 6)).astype(np.float32)).cuda(), torch.from_numpy(rng.standard_normal((n, 5)).astype(np.float32)).cuda()
    r = torch.tensor(G_ROWS, dtype=torch.int32, device="cuda")
    s, d = rollout._u32_as_i32(SEEDS).cuda(), rollout._u32_as_i32(DRAWS).cuda()
    x0, bx = guarded(mb * N * W * A)
    io, bi = guarded(mb * N * 6)
    go, bg = guarded(mb * N * 5)
    head = (r.data_ptr(), mb, n, s.data_ptr(), d.data_ptr(), img.data_ptr(), 6, goals.data_ptr(), 5, io.data_ptr(), go.data_ptr(), x0.data_ptr())
    if warm:
        L.check(L.load().mode_env_gather_warm_cand(*head, plan.data_ptr(), W, A, shift, sigma, N, _stream()), "env_gather_warm_cand")
    else:
        L.check(L.load().mode_env_gather_noise_cand(*head, W * A, SIGMA_MAX, N, _stream()), "env_gather_noise_cand")
    torch.cuda.synchronize()
    assert guards_intact(bx, mb * N * W * A) and guards_intact(bi, mb * N * 6) and guards_intact(bg, mb * N * 5)
    x0, io, go = x0.view(mb, N, W, A), io.view(mb, N, 6), go.view(mb, N, 5)
    for j, e in enumerate(G_ROWS):
        if not 0 <= e < n:
            assert (x0[j] == SENTINEL).all() and (io[j] == SENTINEL).all() and (go[j] == SENTINEL).all(), j       # untouched
            continue
        draws = [(DRAWS[e] * N + c) & U32 for c in range(N)]                              # uint32 arithmetic: DRAWS holds 2^32 - 1
        if warm:
            ref = rollout.env_warm_latents(plan[[e] * N], [SEEDS[e]] * N, draws, shift, sigma)
        else:
            ref = rollout.env_noise([SEEDS[e]] * N, draws, W, A, SIGMA_MAX, "cuda")
        assert torch.equal(x0[j], ref), (j, e)
        assert torch.equal(io[j], img[e].expand(N, -1)) and torch.equal(go[j], goals[e].expand(N, -1)), (j, e)
    assert (DRAWS[3] * N + N - 1) > U32                                                   # the wrap was exercised


# ------------------------------------------------------------------------------------------------------------------ 3. exact replans
def _cand_reference(pol, den, sampler, img, goal, seeds, draws, prev, rows, has_prev, warm_k=None):
    """What a candidate replan of ``rows`` (bucket-padded environment list) must produce: the fused sampler on the hand-built mb * N batch -
    cold latents, or (``warm_k``) warm ones through the sub-schedule - then select_coherent against the previous plans."""
    N, s = pol.candidates, pol.multistep
    W, A = pol.act_window_size, pol.action_dim
    sched = pol._schedule(img.device)
    rc = [r for r in rows for _ in range(N)]
    dr = [(draws[r] * N + c) & U32 for r in rows for c in range(N)]
    if warm_k is None:
        x0, sig = rollout.env_noise([seeds[r] for r in rc], dr, W, A, SIGMA_MAX, "cuda"), sched
    else:
        x0, sig = rollout.env_warm_latents(prev[rc], [seeds[r] for r in rc], dr, s, sched[warm_k]), sched[warm_k:].clone()
    ref = SAMPLERS[sampler](den, {"state_images": img[rc].contiguous()}, x0, goal[rc].contiguous(), sig, disable=True)
    return rollout.select_coherent(ref.view(len(rows), N, W, A), prev[rows], [bool(has_prev[r]) for r in rows], s,
                                   rollout.coherence_weights(pol.coherence_decay, W - s))


@pytest.mark.parametrize("sampler,w", [("ddim", None), ("heun", None), ("dpmpp_2m", None), ("ddim", 2.5)])
def test_replans_equal_fused_sampler_on_candidate_batch_then_selection(sampler, w):
    cfg, m, den = build("bf16")
    den.guidance_scale = w
    n, s, N = 8, 4, 3
    pol = policy(den, cfg, n, sampler_type=sampler, multistep=s, candidates=N)
    assert pol.coherence_decay == 0.5 and (pol.selected == -1).all() and pol.candidate_scores.shape == (n, N)
    img, goal = obs(cfg, n, 1)
    seeds = [11, 12, 13, 14, 15, 16, 17, 18]
    pol.reset(seeds=seeds)
    zero = torch.zeros_like(pol.plans)
    out = pol.step({"state_images": img}, goal)                                           # the first replan of an episode: candidate 0
    chosen, selected, scores = _cand_reference(pol, den, sampler, img, goal, seeds, [0] * n, zero, list(range(n)), [False] * n)
    assert pol.replanned == list(range(n)) and (pol.selected == 0).all() and (pol.candidate_scores == 0).all()
    assert torch.equal(pol.plans, chosen) and torch.equal(out, chosen[:, 0]) and (selected == 0).all()
    picked = set()
    for step, envs in enumerate(([1, 4, 6], [0, 2, 3, 5, 7], [4])):                      # m = 3 (bucket 4), 5 (bucket 8), 1
        _drain(pol, img, goal, envs)
        act = np.zeros(n, dtype=bool)
        act[envs] = True
        draws, prev, psel, psc = pol.draws.cpu().tolist(), pol.plans.clone(), pol.selected.clone(), pol.candidate_scores.clone()
        out = pol.step({"state_images": img}, goal, active=act)
        assert pol.replanned == envs
        mb, m_ = next(b for b in (1, 2, 4, 8) if b >= len(envs)), len(envs)
        rows = envs + [envs[-1]] * (mb - m_)
        chosen, selected, scores = _cand_reference(pol, den, sampler, img, goal, seeds, draws, prev, rows, [True] * n)
        assert torch.equal(pol.plans[envs], chosen[:m_]), (sampler, step)
        assert torch.equal(out[envs], chosen[:m_, 0]) and not out[~torch.from_numpy(act).cuda()].any()
        assert torch.equal(pol.selected[envs], selected[:m_]) and torch.equal(pol.candidate_scores[envs], scores[:m_])
        assert (scores[:m_] > 0).all()
        assert pol.draws.cpu().tolist() == [d + (i in envs) for i, d in enumerate(draws)]
        others = [b for b in range(n) if b not in envs]
        assert torch.equal(pol.plans[others], prev[others]) and torch.equal(pol.selected[others], psel[others])
        assert torch.equal(pol.candidate_scores[others], psc[others])
        picked |= set(selected[:m_].cpu().tolist())
    assert len(picked) > 1                                                                # (the selection is not trivially candidate 0)
    # a replan after a reset has nothing to be coherent with: candidate 0 again, next to an environment that has
    pol.reset(envs=[4])
    _drain(pol, img, goal, [2])
    act = np.zeros(n, dtype=bool)
    act[[2, 4]] = True
    draws, prev = pol.draws.cpu().tolist(), pol.plans.clone()
    pol.step({"state_images": img}, goal, active=act)
    chosen, selected, scores = _cand_reference(pol, den, sampler, img, goal, seeds, draws, prev, [2, 4], [b != 4 for b in range(n)])
    assert torch.equal(pol.plans[[2, 4]], chosen) and torch.equal(pol.selected[[2, 4]], selected) and torch.equal(pol.candidate_scores[[2, 4]], scores)
    assert pol.selected[4] == 0 and (pol.candidate_scores[4] == 0).all() and (pol.candidate_scores[2] > 0).all()


# ------------------------------------------------------------------------------------------------------------------ 4. defaults
class _CountingLib:
    """The policy's library handle with every call counted by name."""

    def __init__(self, lib):
        self._lib, self.calls = lib, {}

    def __getattr__(self, name):
        fn = getattr(self._lib, name)

        def counted(*a):
            self.calls[name] = self.calls.get(name, 0) + 1
            return fn(*a)
        return counted


@pytest.mark.parametrize("cand", [None, 1])
def test_candidates_none_and_one_are_the_policy_without_the_keyword(cand, monkeypatch):
    cfg, m, den = build("bf16")
    n, steps, s = 5, 12, 4
    rng = np.random.default_rng(5)
    resets = {t: sorted(rng.choice(n, size=int(rng.integers(1, 3)), replace=False).tolist()) for t in (2, 5, 9)}
    active = rng.random((steps, n)) > 0.2
    g = torch.Generator().manual_seed(9)
    obs_t = [torch.randn(n, 2, cfg.obs_dim, generator=g).cuda() for _ in range(steps)]
    goal = torch.randn(n, cfg.goal_dim, generator=g).cuda()
    plain, other = policy(den, cfg, n, seed=100, multistep=s), policy(den, cfg, n, seed=100, multistep=s, candidates=cand)
    assert other.candidates == cand and other._sel is None and other._ctrl.numel() == plain._ctrl.numel()
    with pytest.raises(AttributeError, match="without candidates"):
        other.selected
    plain._lib, other._lib = _CountingLib(plain._lib), _CountingLib(other._lib)
    cnt = count_graphs(monkeypatch)
    replays, replans = [0, 0], 0
    for t in range(steps):
        outs = []
        for i, p in enumerate((plain, other)):
            if t in resets:
                p.reset(envs=resets[t], seeds=[1000 * t + b for b in resets[t]])
            before = cnt["replay"]
            outs.append(p.step({"state_images": obs_t[t]}, goal, active=active[t]))
            replays[i] += cnt["replay"] - before
        assert torch.equal(outs[0], outs[1]) and torch.equal(plain.plans, other.plans) and torch.equal(plain.draws, other.draws), t
        assert plain.replanned == other.replanned
        replans += bool(other.replanned)
    assert replans >= 5 and replays[0] == replays[1] >= replans
    assert plain._lib.calls == other._lib.calls and set(other._lib.calls) == {"mode_env_gather_noise", "mode_env_commit_emit"}
    assert [k for k, _ in plain._hooks.store.items()] == [k for k, _ in other._hooks.store.items()]


# ------------------------------------------------------------------------------------------------------------------ 5. combinations
def test_candidates_with_warm_start_cold_and_warm_chunks_in_one_step():
    cfg, m, den = build("bf16")
    n, s, N, k = 5, 4, 2, 5
    pol = policy(den, cfg, n, multistep=s, candidates=N, warm_start=k, seed=40)
    seeds = [40 + b for b in range(n)]
    img, goal = obs(cfg, n, 6)
    pol.step({"state_images": img}, goal)
    assert pol.replanned == list(range(n)) and pol.replanned_warm == [] and (pol.selected == 0).all()
    _drain(pol, img, goal, list(range(n)))
    pol.reset(envs=[1, 3])                                                                # -> cold chunk [1, 3] (bucket 2), warm chunk [0, 2, 4] (bucket 4)
    draws, prev = pol.draws.cpu().tolist(), pol.plans.clone()
    out = pol.step({"state_images": img}, goal)
    assert pol.replanned == list(range(n)) and pol.replanned_warm == [0, 2, 4]
    cold = _cand_reference(pol, den, "ddim", img, goal, seeds, draws, prev, [1, 3], [False] * n)
    warm = _cand_reference(pol, den, "ddim", img, goal, seeds, draws, prev, [0, 2, 4, 4], [True] * n, warm_k=k)
    assert torch.equal(pol.plans[[1, 3]], cold[0]) and (pol.selected[[1, 3]] == 0).all() and (pol.candidate_scores[[1, 3]] == 0).all()
    assert torch.equal(pol.plans[[0, 2, 4]], warm[0][:3]) and torch.equal(pol.selected[[0, 2, 4]], warm[1][:3])
    assert torch.equal(pol.candidate_scores[[0, 2, 4]], warm[2][:3]) and (warm[2][:3] > 0).all()
    assert torch.equal(out, pol.plans[:, 0])                                              # both kinds are emitted in the one step
    assert pol.draws.cpu().tolist() == [d + 1 for d in draws]
    assert sorted(b for _, b in pol._hooks.store) == [2 * N, 5 * N] and [b for _, b in pol._hooks_warm.store] == [4 * N]


def test_candidates_with_temporal_ensemble_ring_and_plans_receive_the_selection():
    cfg, m, den = build("bf16")
    n, s, N = 5, 4, 2
    pol = policy(den, cfg, n, multistep=s, candidates=N, temporal_ensemble=0.5, seed=60)
    seeds = [60 + b for b in range(n)]
    img, goal = obs(cfg, n, 7)
    pol.step({"state_images": img}, goal)
    first = pol.plans.clone()
    assert (pol.selected == 0).all() and torch.equal(pol.plan_ring[:, 0], first) and (pol.plan_births[:, 0] == 0).all()
    for _ in range(s - 1):
        pol.step({"state_images": img}, goal)
    assert pol.replanned == [] and torch.equal(pol.plans, first)
    draws = pol.draws.cpu().tolist()
    out = pol.step({"state_images": img}, goal)                                           # local time 4: the second plan, scored against the first
    assert pol.replanned == list(range(n))
    chosen, selected, scores = _cand_reference(pol, den, "ddim", img, goal, seeds, draws, first, list(range(n)), [True] * n)
    assert torch.equal(pol.plans, chosen) and torch.equal(pol.plan_ring[:, 1], chosen) and torch.equal(pol.plan_ring[:, 0], first)
    assert (pol.plan_births[:, :2].cpu() == torch.tensor([0, 4])).all() and (pol.local_times == s + 1).all()
    assert torch.equal(pol.selected, selected) and torch.equal(pol.candidate_scores, scores)
    wt = pol.ensemble_weight_table.double()
    want = (wt[0] * first[:, s].double() + wt[1] * chosen[:, 0].double()) / (wt[0] + wt[1])     # oldest first
    assert torch.allclose(out.double(), want, rtol=2e-6, atol=1e-6)


# ------------------------------------------------------------------------------------------------------------------ 6. raw frames
def _entry(pol, mb, warm=False):
    (ent,) = [e for (gkey, b), e in (pol._hooks_warm if warm else pol._hooks).store.items() if b == mb * pol.candidates]
    return ent


@pytest.mark.parametrize("camera", [False, True], ids=["float-frames", "uint8-cameras"])
def test_frames_with_candidates_equal_the_policy_fed_the_encoders_own_embeddings(camera):
    """The towers run once per environment (batch mb * T) and their rows are broadcast to the N candidate rows; a policy without encoders fed
    exactly those embeddings then runs the same chain on the same bits: the same plans, selections and actions, bit for bit."""
    from test_gpu_vector_env import build as build_mode
    cfg, m, den = build_mode("noise", "bf16")
    encs = encoders(cfg)
    n, s, N = 3, 2, 4
    kw = dict(act_window_size=cfg.action_seq_len, action_dim=cfg.action_dim, sigma_max=SIGMA_MAX, multistep=s, candidates=N, seed=70)
    pf = rollout.VectorEnvPolicy(den, n, static_resnet=encs[0], gripper_resnet=encs[1], camera_transforms=TRANSFORMS if camera else None, **kw)
    pe = rollout.VectorEnvPolicy(den, n, **kw)
    picked = set()
    for t, envs in enumerate(([0, 1, 2], [0, 1, 2], [0, 2], [0, 2], [1])):                # buckets 3, -, 2, -, 1
        ob, goal = u8_frames(cfg, n, 80 + t) if camera else frames(cfg, n, 80 + t)
        act = np.zeros(n, dtype=bool)
        act[envs] = True
        a = pf.step(ob, goal, active=act)
        if not pf.replanned:
            assert torch.equal(a, pe.step({"state_images": emb}, goal, active=act)) and pe.replanned == []
            continue
        mb, m_ = next(b for b in (1, 2, 3) if b >= len(pf.replanned)), len(pf.replanned)
        ent, st = _entry(pf, mb), pf._enc_store[mb]
        assert st["bufs"][0].shape == (mb, 1, 3, 64, 64) and st["bufs"][1].shape[0] == mb          # the towers' batch: mb * T, not mb * N * T
        tok = ent["img"].view(mb, N, 2, cfg.obs_dim)
        assert ent["img"].shape[0] == mb * N and all(torch.equal(tok[:, c], tok[:, 0]) for c in range(1, N))
        if not camera:                                                                    # the eager towers on the gathered rows and goals
            rows = pf.replanned + [pf.replanned[-1]] * (mb - m_)
            assert torch.equal(tok[:, 0], tokens(encs, rows_of(ob, rows), goal[rows].contiguous()))
        emb = torch.full((n, 2, cfg.obs_dim), float("nan"), device="cuda")                # rows that do not replan are not read
        emb[pf.replanned] = tok[:m_, 0]
        b = pe.step({"state_images": emb}, goal, active=act)
        assert pf.replanned == pe.replanned == envs
        assert torch.equal(a, b) and torch.equal(pf.plans, pe.plans) and torch.isfinite(pf.plans[pf.replanned]).all(), t
        assert torch.equal(pf.selected, pe.selected) and torch.equal(pf.candidate_scores, pe.candidate_scores), t
        picked |= set(pf.selected[pf.replanned].cpu().tolist())
    assert len(picked) > 1


# ------------------------------------------------------------------------------------------------------------------ 7. budget
def test_no_capture_one_replay_per_kind_no_sync_flat_memory_with_candidates(monkeypatch):
    """tests/test_gpu_vector_env_warm.py::test_no_capture_one_replay_per_kind_no_sync_flat_memory with candidates=2: after warmup, cold, warm and
    mixed replans alternating over the buckets neither capture nor synchronise, take one replay per chunk and hold no more memory."""
    cfg, m, den = build("bf16")
    n, s, k, N = 4, 2, 5, 2
    pol = policy(den, cfg, n, multistep=s, warm_start=k, candidates=N)
    img, goal = obs(cfg, n, 4)
    pol.warmup({"state_images": img}, goal)
    assert len(pol._hooks.store) == len(pol._hooks_warm.store) == len(rollout._buckets(n))
    assert sorted(b for _, b in pol._hooks.store) == [N * b for b in rollout._buckets(n)]
    assert not pol._warm.any() and not pol.draws.any() and (pol.selected == -1).all() and not pol.candidate_scores.any()   # warming up changes no state
    cnt = count_graphs(monkeypatch)
    cycle = ([0, 1, 2, 3], [], [0, 1], [0], [0, 1, 2])

    def loop(steps):
        seen = {"cold": 0, "warm": 0, "mixed": 0, "none": 0}
        for t in range(steps):
            resets = cycle[(t // s) % len(cycle)] if t % s == 0 else []
            if resets:
                pol.reset(envs=resets)
            before = cnt["replay"]
            pol.step({"state_images": img}, goal)
            if t % s:
                assert pol.replanned == [] and cnt["replay"] == before, t
                seen["none"] += 1
                continue
            warm = [b for b in range(n) if b not in resets] if t else []
            assert pol.replanned == list(range(n)) and pol.replanned_warm == warm, t
            mixed = 0 < len(warm) < n
            assert cnt["replay"] == before + (2 if mixed else 1), (t, warm)
            seen["mixed" if mixed else "warm" if warm else "cold"] += 1
        return seen
    loop(2 * s * len(cycle))
    torch.cuda.synchronize()
    mem = torch.cuda.memory_allocated()
    torch.cuda.set_sync_debug_mode("error")
    try:
        seen = loop(100)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    torch.cuda.synchronize()
    assert seen == {"cold": 10, "warm": 10, "mixed": 30, "none": 50} and cnt["capture"] == 0
    assert torch.cuda.memory_allocated() == mem
    assert (pol.selected >= 0).all() and (pol.selected < N).all()


def test_frames_with_candidates_one_encoder_replay_and_one_chain_replay_per_chunk(monkeypatch):
    from test_gpu_vector_env import build as build_mode
    cfg, m, den = build_mode("noise", "bf16")
    encs = encoders(cfg)
    n, s, N = 2, 2, 2
    pol = rollout.VectorEnvPolicy(den, n, act_window_size=cfg.action_seq_len, action_dim=cfg.action_dim, sigma_max=SIGMA_MAX, multistep=s,
                                  candidates=N, static_resnet=encs[0], gripper_resnet=encs[1])
    ob, goal = frames(cfg, n, 5)
    pol.warmup(ob, goal)
    assert sorted(pol._enc_store) == [1, 2] and (pol.selected == -1).all()
    cnt = count_graphs(monkeypatch)
    torch.cuda.set_sync_debug_mode("error")
    try:
        for r, envs in enumerate(([0, 1], [1], [0, 1], [0]) * 2):                         # buckets 2, 1, 2, 1
            act = np.zeros(n, dtype=bool)
            act[envs] = True
            for i in range(s):
                before = cnt["replay"]
                pol.step(ob, goal, active=act)
                assert pol.replanned == ([] if i else envs) and cnt["replay"] == before + (0 if i else 2), (r, i)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    assert cnt["capture"] == 0


def test_candidate_entry_points_hold_no_memory():
    """The method of tests/test_gpu_memory_soak.py (warm up, collector off, repeat, flat ``memory_allocated``) for the repeated calls this
    option adds: select_coherent, the candidate gathers through a policy's replans, and the policy's step."""
    cfg, m, den = build("bf16")
    n, N, W, A = 4, 4, cfg.action_seq_len, cfg.action_dim
    img, goal = obs(cfg, n, 8)
    pol = policy(den, cfg, n, multistep=2, candidates=N, warm_start=5)
    chunk, prev = torch.randn(n, N, W, A, device="cuda"), torch.randn(n, W, A, device="cuda")
    wt = rollout.coherence_weights(0.5, W - 2)

    def flat(fn, warm=4, reps=12, slack=1 << 20):
        for _ in range(warm):
            fn()
        torch.cuda.synchronize()
        gc.collect()
        was = gc.isenabled()
        gc.disable()
        try:
            fn()
            torch.cuda.synchronize()
            base, seen = torch.cuda.memory_allocated(), []
            for _ in range(reps):
                fn()
                torch.cuda.synchronize()
                seen.append(torch.cuda.memory_allocated())
        finally:
            if was:
                gc.enable()
        assert max(seen) <= base + slack, (base, seen)
    flat(lambda: rollout.select_coherent(chunk, prev, [True] * n, 2, wt))
    flat(lambda: pol.step({"state_images": img}, goal))
