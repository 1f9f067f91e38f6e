"""rollout.VectorEnvPolicy(candidates=N, contrast=M) on the MI355X (c1e4 weights, oracle.weights): the forward-contrast select kernel against the
fp64 restatement of tests/bid_refs.py over its case table, the (N, M) gathers against env_noise / env_warm_latents, replans against "the fused
sampler on the gathered (N + M)-row batch, then select_bidirectional" (bit for bit), the weight as a device scalar, the default path against a
policy built without the keyword, and the combinations with warm_start, temporal_ensemble and raw uint8 frames."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from mode_diffusion_policy_amd import _lib as L  # noqa: E402
from mode_diffusion_policy_amd import rollout  # noqa: E402

import bid_refs as B  # noqa: E402
import cand_refs as R  # noqa: E402
from test_gpu_vector_env_camera import TRANSFORMS, u8_frames  # noqa: E402
from test_gpu_vector_env_candidates import GUARD, ISENT, SENTINEL, U32, _CountingLib, guarded, guards_intact  # noqa: E402, F401
from test_gpu_vector_env_frames import encoders  # noqa: E402
from test_gpu_vector_env_warm import SAMPLERS, SIGMA_MAX, _drain, build, count_graphs, obs, policy  # noqa: E402

_stream = lambda: torch.cuda.current_stream().cuda_stream


# ------------------------------------------------------------------------------------------------------------------ 1. the select kernel
NUM_ENVS = B.CASE_ENVS
ROWS = [3, 0, 2, -1, NUM_ENVS, 4, 1, 1, 1]                                            # two entries out of range; padding by repetition; env 5 not listed
LISTED = sorted({r for r in ROWS if 0 <= r < NUM_ENVS})


def _select_bid(rows, cands, prev, has_prev, shift, wt, N, K, lam, count=None):
    """mode_env_select_bid on sentinel-filled outputs with guard words: cands [num_envs, N + M, W, A] (chunk row j = the candidates of rows[j],
    zeros for an out-of-range entry), prev [num_envs, W, A].  Returns (chunk [m_b, N + M, W, A], chosen [m_b, W, A], selected [num_envs],
    total [num_envs, N], bc [num_envs, N + M], fc [num_envs, N], guards intact)."""
    n, NT, W, A = cands.shape
    mb = len(rows)
    chunk = torch.stack([cands[r] if 0 <= r < n else torch.zeros_like(cands[0]) for r in rows]).contiguous()
    r = torch.tensor(rows, dtype=torch.int32, device="cuda")
    mask = torch.from_numpy(rollout._mask_words(np.asarray(has_prev, dtype=bool), (n + 31) // 32).view("<i4").copy()).cuda()
    w = torch.from_numpy(np.asarray(wt, dtype=np.float32)).cuda()
    lam_dev = torch.tensor([lam], dtype=torch.float32, device="cuda")
    cnt = None if count is None else torch.tensor([count], dtype=torch.int32, device="cuda")
    chosen, b0 = guarded(mb * W * A)
    selected, b1 = guarded(n, ISENT, torch.int32)
    total, b2 = guarded(n * N)
    bc, b3 = guarded(n * NT)
    fc, b4 = guarded(n * N)
    d = L.ModeEnvBidDesc(rows=r.data_ptr(), has_prev=mask.data_ptr(), count=None if cnt is None else cnt.data_ptr(), chunk=chunk.data_ptr(),
                         plan=prev.data_ptr(), weights=w.data_ptr(), chosen=chosen.data_ptr(), selected=selected.data_ptr(), scores=total.data_ptr(),
                         lambda_=lam_dev.data_ptr(), bc=bc.data_ptr(), fc=fc.data_ptr(), m_b=mb, num_envs=n, W=W, A=A, shift=shift, N=N, M=NT - N, K=K)
    L.check(L.load().mode_env_select_bid(C.byref(d), _stream()), "env_select_bid")
    torch.cuda.synchronize()
    ok = guards_intact(b0, mb * W * A) and guards_intact(b1, n, ISENT) and guards_intact(b2, n * N) and guards_intact(b3, n * NT) and \
        guards_intact(b4, n * N)
    return chunk, chosen.view(mb, W, A), selected, total.view(n, N), bc.view(n, NT), fc.view(n, N), ok


@pytest.mark.parametrize("W,A,shift,N,M,K", B.CASES)
def test_select_bid_matches_restatement(W, A, shift, N, M, K):
    """Over the table of bid_refs (both lambdas, with and without previous plans): bc[:N] has the bits of mode_env_select's scores; bc, fc and
    total lie within their derived bounds of fp64 (cand_refs.score_bound, bid_refs.fc_bound / total_bound); the selected candidate is strong and
    its fp64 total within the two bounds of the fp64 minimum, always, and the fp64 argmin on decisive rows; the rows that are not decisive are
    counted and stay under the table's cap (tests/test_vector_env_contrast.py holds the whole table to it)."""
    c_np, p_np, refs = B.table(W, A, shift, N, M, K)
    cands, prev = torch.from_numpy(c_np.copy()).cuda(), torch.from_numpy(p_np.copy()).cuda()
    wt = rollout.coherence_weights(B.RHO, W - shift)
    bc_rel = R.score_bound(W - shift, A)
    rows_seen = loose = 0
    worst = dict(bc=0.0, fc=0.0, total=0.0)
    for (lam, has), rows_ref in refs.items():
        chunk, chosen, selected, total, bc, fc, ok = _select_bid(ROWS, cands, prev, [has] * NUM_ENVS, shift, wt, N, K, lam)
        assert ok
        again = _select_bid(ROWS, cands, prev, [has] * NUM_ENVS, shift, wt, N, K, lam)                     # the same bits from run to run
        assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip((chosen, selected, total, bc, fc), again[1:6]))
        coh = rollout.select_coherent(cands[:, :N].contiguous(), prev, [has] * NUM_ENVS, shift, wt)[2]
        sel, tt, bb, ff = selected.cpu().numpy(), total.cpu().double().numpy(), bc.cpu().double().numpy(), fc.cpu().double().numpy()
        for r in range(NUM_ENVS):
            if r not in LISTED:                                                           # an environment nobody listed: untouched
                assert sel[r] == ISENT and (total[r] == SENTINEL).all() and (bc[r] == SENTINEL).all() and (fc[r] == SENTINEL).all(), r
        for j, r in enumerate(ROWS):
            if not 0 <= r < NUM_ENVS:
                assert (chosen[j] == SENTINEL).all(), j                                   # untouched
                continue
            ref, bt, bf, dec = rows_ref[r]
            assert torch.equal(bc[r, :N].view(torch.int32), coh[r].view(torch.int32)), (lam, has, r)
            if has:
                e = np.abs(bb[r] - ref["bc"]) / ref["bc"]
                worst["bc"] = max(worst["bc"], float(e.max() / bc_rel))
                assert np.all(e <= bc_rel), (lam, has, r, float(e.max()), bc_rel)
            else:
                assert (bc[r] == 0).all(), r
            ef, et = np.abs(ff[r] - ref["fc"]) / bf, np.abs(tt[r] - ref["total"]) / bt
            worst["fc"], worst["total"] = max(worst["fc"], float(ef.max())), max(worst["total"], float(et.max()))
            assert np.all(ef <= 1.0), (lam, has, r, float(ef.max()))
            assert np.all(et <= 1.0), (lam, has, r, float(et.max()))
            best = int(np.argmin(ref["total"]))
            assert 0 <= sel[r] < N and ref["total"][sel[r]] - ref["total"][best] <= bt[sel[r]] + bt[best], (lam, has, r)
            if ROWS.index(r) == j:                                                       # (the repeats of env 1 are the same row again)
                rows_seen += 1
                loose += not dec
            if dec:
                assert sel[r] == ref["selected"] == best, (lam, has, r)
            assert torch.equal(chosen[j].view(torch.int32), chunk[j, sel[r]].view(torch.int32)), (lam, has, r)
        solo = _select_bid([1], cands, prev, [has] * NUM_ENVS, shift, wt, N, K, lam)      # a padded call and a solo call: identical rows
        assert solo[6] and solo[2][1] == selected[1] and all(torch.equal(solo[i][1], (total, bc, fc)[i - 3][1]) for i in (3, 4, 5))
        assert all(torch.equal(solo[1][0], chosen[j]) for j in (6, 7, 8))
    print(f"select_bid W={W} A={A} shift={shift} N={N} M={M} K={K}: worst error / bound bc {worst['bc']:.3f} fc {worst['fc']:.3f} total "
          f"{worst['total']:.3f}; {loose} of {rows_seen} rows not decisive")
    assert rows_seen == 4 * len(LISTED) and loose <= (1.0 - B.DECISIVE_SHARE) * rows_seen


def test_select_bid_count_skips_the_rows_behind_it():
    """ModeEnvBidDesc.count (the control block's m): rows j >= *count are left untouched, as for mode_env_select."""
    W, A, s, N, M, K = B.CASES[1]
    c_np, p_np, _ = B.table(*B.CASES[1])
    cands, prev = torch.from_numpy(c_np[:3].copy()).cuda(), torch.from_numpy(p_np[:3].copy()).cuda()
    wt = rollout.coherence_weights(0.5, W - s)
    full = rollout.select_bidirectional(cands, prev, [True] * 3, s, wt, M, K, 1.0)
    for m in (0, 2):
        chunk, chosen, selected, total, bc, fc, ok = _select_bid([0, 1, 2], cands, prev, [True] * 3, s, wt, N, K, 1.0, count=m)
        assert ok
        for got, want in zip((chosen, selected, total, bc, fc), full):
            assert torch.equal(got[:m], want[:m]) and (got[m:] == (ISENT if got.dtype == torch.int32 else SENTINEL)).all()


def test_select_bid_constructed_cases():
    W, A, s, N, M, K = 10, 7, 4, 4, 3, 2
    rng = np.random.default_rng(5)
    prev = torch.from_numpy(rng.standard_normal((5, W, A)).astype(np.float32)).cuda()
    tail = prev[:, np.minimum(np.arange(W) + s, W - 1)]
    chunk = tail[:, None] + torch.from_numpy(rng.standard_normal((5, N + M, W, A)).astype(np.float32)).cuda()
    chunk[:, N:] += 3.0
    w = rollout.coherence_weights(0.5, W - s)
    # row 0: a weak candidate IS the previous tail (bc exactly 0, the smallest of all) -> still a strong one is selected
    # row 1: no previous plan -> bc exactly 0, S+ = {0, 1}, S- = {N, N + 1} by index
    # row 2: strong candidates 1 and 3 identical -> equal totals, the lower index if they win; made to win by sitting on the strong mean
    # row 3: candidate 0 holds a NaN in a scored element: its bc, fc and total are NaN, it ranks last and is not selected
    # row 4: every strong candidate holds a NaN -> candidate 0
    chunk[0, N + 1] = tail[0]
    chunk[2, 1] = chunk[2, 3] = tail[2] + 1e-3
    chunk[3, 0, 2, 3] = float("nan")
    chunk[4, :N, 0, 0] = float("nan")
    has = [True, False, True, True, True]
    chosen, selected, total, bc, fc = rollout.select_bidirectional(chunk, prev, has, s, w, M, K, 1.0)
    sel, c64 = selected.cpu().tolist(), chunk.cpu().double().numpy()
    assert all(0 <= v < N for v in sel)                                                  # never a weak index
    assert bc[0, N + 1] == 0 and (bc[0, :N] > 0).all() and bc[0].argmin().item() == N + 1
    ref1 = B.reference(c64[1], prev[1].cpu().numpy(), False, s, 0.5, N, K, 1.0)
    assert (bc[1] == 0).all() and list(ref1["sp"]) == [0, 1] and list(ref1["sn"]) == [N, N + 1] and sel[1] == ref1["selected"]
    assert np.allclose(fc[1].cpu().double().numpy(), ref1["fc"], rtol=0, atol=float(B.fc_bound(ref1, W, A).max()))
    assert torch.equal(total[1], fc[1])                                                  # fma(1, fc, 0)
    assert torch.equal(total[2, 1], total[2, 3]) and torch.equal(fc[2, 1], fc[2, 3]) and sel[2] == 1
    assert torch.isnan(bc[3, 0]) and torch.isnan(fc[3, 0]) and torch.isnan(total[3, 0]) and not torch.isnan(total[3, 1:]).any() and sel[3] != 0
    ref3 = B.reference(c64[3], prev[3].cpu().numpy(), True, s, 0.5, N, K, 1.0)
    assert 0 not in ref3["sp"] and sel[3] == ref3["selected"]
    assert sel[4] == 0 and torch.isnan(total[4]).all()
    for i in range(5):                                                                    # bit for bit, NaN payloads included
        assert torch.equal(chosen[i].view(torch.int32), chunk[i, sel[i]].view(torch.int32)), i
    # lambda = 0: the coherence selection of the strong candidates, total = bc bit for bit
    z = rollout.select_bidirectional(chunk[:3], prev[:3], has[:3], s, w, M, K, 0.0)
    coh = rollout.select_coherent(chunk[:3, :N].contiguous(), prev[:3], has[:3], s, w)
    assert torch.equal(z[1], coh[1]) and torch.equal(z[2], coh[2]) and torch.equal(z[3][:, :N], coh[2]) and torch.equal(z[0], coh[0])
    # K beyond both counts means all of them
    a, b = (rollout.select_bidirectional(chunk[:3], prev[:3], has[:3], s, w, M, k, 1.0) for k in (N, 64))
    assert all(torch.equal(x, y) for x, y in zip(a, b))


def test_select_bid_bad_arguments_launch_nothing():
    W, A, s, N, M, K = B.CASES[1]
    c_np, p_np, _ = B.table(*B.CASES[1])
    cands, prev = torch.from_numpy(c_np[:2].copy()).cuda(), torch.from_numpy(p_np[:2].copy()).cuda()
    wt = rollout.coherence_weights(0.5, W - s)
    for over in (dict(N=0), dict(M=0), dict(N=N + 57), dict(K=0), dict(shift=0), dict(shift=W), dict(m_b=0), dict(num_envs=0), dict(bc=None),
                 dict(fc=None), dict(lambda_=None)):
        outs = [torch.full((2, W, A), SENTINEL, device="cuda"), torch.full((2,), ISENT, dtype=torch.int32, device="cuda"),
                torch.full((2, N), SENTINEL, device="cuda"), torch.full((2, N + M), SENTINEL, device="cuda"), torch.full((2, N), SENTINEL, device="cuda")]
        rows, mask = torch.arange(2, dtype=torch.int32, device="cuda"), torch.full((1,), 3, dtype=torch.int32, device="cuda")
        lam, w = torch.ones(1, device="cuda"), torch.from_numpy(wt).cuda()
        kw = dict(rows=rows.data_ptr(), has_prev=mask.data_ptr(), count=None, chunk=cands.data_ptr(), plan=prev.data_ptr(), weights=w.data_ptr(),
                  chosen=outs[0].data_ptr(), selected=outs[1].data_ptr(), scores=outs[2].data_ptr(), lambda_=lam.data_ptr(), bc=outs[3].data_ptr(),
                  fc=outs[4].data_ptr(), m_b=2, num_envs=2, W=W, A=A, shift=s, N=N, M=M, K=K)
        d = L.ModeEnvBidDesc(**dict(kw, **over))
        assert L.load().mode_env_select_bid(C.byref(d), _stream()) == -1, over
        torch.cuda.synchronize()
        assert all((o == (ISENT if o.dtype == torch.int32 else SENTINEL)).all() for o in outs), over


# ------------------------------------------------------------------------------------------------------------------ 2. the (N, M) gathers
SEEDS, DRAWS = [0, 7, 2 ** 32 - 1, 123456789, 2 ** 20], [0, 3, 2 ** 20, 2 ** 32 - 1, 9]
G_ROWS = [3, 0, 2, -1, 5, 4, 1, 1, 1]


@pytest.mark.parametrize("W,A,N,M", [(10, 7, 2, 1), (37, 7, 3, 5), (64, 64, 32, 32)])
@pytest.mark.parametrize("warm", [False, True], ids=["noise", "warm"])
def test_bid_gathers_zero_the_weak_goal_rows_and_draw_at_draws_times_n_plus_m_plus_c(warm, W, A, N, M):
    n, mb, shift, sigma, NT = 5, len(G_ROWS), 4, 0.37, N + M
    rng = np.random.default_rng(W + NT)
    plan = torch.from_numpy(rng.standard_normal((n, W, A)).astype(np.float32)).cuda()
    img, goals = torch.from_numpy(rng.standard_normal((n, 6)).astype(np.float32)).cuda(), torch.from_numpy(rng.standard_normal((n, 5)).astype(np.float32)).cuda()
    r = torch.tensor(G_ROWS, dtype=torch.int32, device="cuda")
    s, d = rollout._u32_as_i32(SEEDS).cuda(), rollout._u32_as_i32(DRAWS).cuda()
    x0, bx = guarded(mb * NT * W * A)
    io, bi = guarded(mb * NT * 6)
    go, bg = guarded(mb * NT * 5)
    head = (r.data_ptr(), mb, n, s.data_ptr(), d.data_ptr(), img.data_ptr(), 6, goals.data_ptr(), 5, io.data_ptr(), go.data_ptr(), x0.data_ptr())
    if warm:
        L.check(L.load().mode_env_gather_warm_bid(*head, plan.data_ptr(), W, A, shift, sigma, N, M, _stream()), "env_gather_warm_bid")
    else:
        L.check(L.load().mode_env_gather_noise_bid(*head, W * A, SIGMA_MAX, N, M, _stream()), "env_gather_noise_bid")
    torch.cuda.synchronize()
    assert guards_intact(bx, mb * NT * W * A) and guards_intact(bi, mb * NT * 6) and guards_intact(bg, mb * NT * 5)
    x0, io, go = x0.view(mb, NT, W, A), io.view(mb, NT, 6), go.view(mb, NT, 5)
    for j, e in enumerate(G_ROWS):
        if not 0 <= e < n:
            assert (x0[j] == SENTINEL).all() and (io[j] == SENTINEL).all() and (go[j] == SENTINEL).all(), j       # untouched
            continue
        draws = [(DRAWS[e] * NT + c) & U32 for c in range(NT)]                            # uint32 arithmetic: DRAWS holds 2^32 - 1
        if warm:
            ref = rollout.env_warm_latents(plan[[e] * NT], [SEEDS[e]] * NT, draws, shift, sigma)
        else:
            ref = rollout.env_noise([SEEDS[e]] * NT, draws, W, A, SIGMA_MAX, "cuda")
        assert torch.equal(x0[j], ref), (j, e)
        assert torch.equal(io[j], img[e].expand(NT, -1)), (j, e)                          # every candidate sees the observation
        assert torch.equal(go[j, :N], goals[e].expand(N, -1)) and (go[j, N:].view(torch.int32) == 0).all(), (j, e)   # weak: +0.0 exactly
    assert (DRAWS[3] * NT + NT - 1) > U32                                                 # the wrap was exercised


# ------------------------------------------------------------------------------------------------------------------ 3. exact replans
def _bid_reference(pol, den, sampler, img, goal, seeds, draws, prev, rows, has_prev, warm_k=None, lam=None, full=False):
    """What a replan of ``rows`` (bucket-padded environment list) with forward contrast must produce: the fused sampler on the hand-built
    mb * (N + M) batch - N rows with the environment's goal, M with a zero goal; cold latents, or (``warm_k``) warm ones through the
    sub-schedule - then select_bidirectional against the previous plans."""
    N, M, s = pol.candidates, pol.contrast, pol.multistep
    NT, W, A = N + M, pol.act_window_size, pol.action_dim
    sched = pol._schedule(img.device)
    rc = [r for r in rows for _ in range(NT)]
    dr = [(draws[r] * NT + c) & U32 for r in rows for c in range(NT)]
    if warm_k is None:
        x0, sig = rollout.env_noise([seeds[r] for r in rc], dr, W, A, SIGMA_MAX, "cuda"), sched
    else:
        x0, sig = rollout.env_warm_latents(prev[rc], [seeds[r] for r in rc], dr, s, sched[warm_k]), sched[warm_k:].clone()
    gl = goal[rc].clone().view(len(rows), NT, -1)
    gl[:, N:] = 0
    ref = SAMPLERS[sampler](den, {"state_images": img[rc].contiguous()}, x0, gl.view(len(rc), -1).contiguous(), sig, disable=True)
    out = rollout.select_bidirectional(ref.view(len(rows), NT, W, A), prev[rows], [bool(has_prev[r]) for r in rows], s,
                                       rollout.coherence_weights(pol.coherence_decay, W - s), M, pol.contrast_topk,
                                       pol.contrast_weight if lam is None else lam)
    return out + (ref.view(len(rows), NT, W, A),) if full else out


def _entry(pol, mb, warm=False):
    (ent,) = [e for (gkey, b), e in (pol._hooks_warm if warm else pol._hooks).store.items() if b == mb * (pol.candidates + pol.contrast)]
    return ent


def _state_equals(pol, envs, ref, m_):
    chosen, selected, total, bc, fc = ref[:5]
    return (torch.equal(pol.plans[envs], chosen[:m_]) and torch.equal(pol.selected[envs], selected[:m_]) and
            torch.equal(pol.candidate_scores[envs], total[:m_]) and torch.equal(pol.coherence_scores[envs], bc[:m_]) and
            torch.equal(pol.contrast_scores[envs], fc[:m_]))


@pytest.mark.parametrize("sampler,w", [("ddim", None), ("dpmpp_2m", None), ("ddim", 2.5)])
def test_replans_equal_fused_sampler_on_the_strong_and_weak_batch_then_selection(sampler, w):
    cfg, m, den = build("bf16")
    den.guidance_scale = w
    n, s, N, M = 8, 4, 3, 2
    pol = policy(den, cfg, n, sampler_type=sampler, multistep=s, candidates=N, contrast=M)
    assert pol.contrast == M and pol.contrast_topk == 2 and pol.contrast_weight == 1.0 and (pol.selected == -1).all()
    assert pol.candidate_scores.shape == (n, N) and pol.coherence_scores.shape == (n, N + M) and pol.contrast_scores.shape == (n, N)
    img, goal = obs(cfg, n, 1)
    seeds = [11, 12, 13, 14, 15, 16, 17, 18]
    pol.reset(seeds=seeds)
    zero = torch.zeros_like(pol.plans)
    out = pol.step({"state_images": img}, goal)                                           # cold: no previous plan, the contrast term alone decides
    ref = _bid_reference(pol, den, sampler, img, goal, seeds, [0] * n, zero, list(range(n)), [False] * n)
    assert pol.replanned == list(range(n)) and _state_equals(pol, list(range(n)), ref, n) and torch.equal(out, ref[0][:, 0])
    assert (pol.coherence_scores == 0).all() and torch.equal(pol.candidate_scores, pol.contrast_scores)
    assert len(set(pol.selected.cpu().tolist())) > 1                                      # a cold replan no longer keeps the first
    for step, envs in enumerate(([1, 4, 6], [0, 2, 3, 5, 7], [4])):                      # m = 3 (bucket 4), 5 (bucket 8), 1
        _drain(pol, img, goal, envs)
        act = np.zeros(n, dtype=bool)
        act[envs] = True
        draws, prev, psel, psc = pol.draws.cpu().tolist(), pol.plans.clone(), pol.selected.clone(), pol.candidate_scores.clone()
        out = pol.step({"state_images": img}, goal, active=act)
        assert pol.replanned == envs
        mb, m_ = next(b for b in (1, 2, 4, 8) if b >= len(envs)), len(envs)
        rows = envs + [envs[-1]] * (mb - m_)
        ref = _bid_reference(pol, den, sampler, img, goal, seeds, draws, prev, rows, [True] * n)
        assert _state_equals(pol, envs, ref, m_), (sampler, step)
        assert torch.equal(out[envs], ref[0][:m_, 0]) and not out[~torch.from_numpy(act).cuda()].any()
        assert (ref[3][:m_] > 0).all() and (pol.selected[envs] < N).all()
        assert pol.draws.cpu().tolist() == [d + (i in envs) for i, d in enumerate(draws)]
        others = [b for b in range(n) if b not in envs]
        assert torch.equal(pol.plans[others], prev[others]) and torch.equal(pol.selected[others], psel[others])
        assert torch.equal(pol.candidate_scores[others], psc[others])
    assert sorted(b for _, b in pol._hooks.store) == [(N + M) * b for b in (1, 4, 8)]


def test_weak_rows_do_not_depend_on_the_goal():
    """Two policies with the same seeds and observations and different goals: the weak candidates' plans are bit-identical (their goal row is
    zero), the strong ones differ."""
    cfg, m, den = build("bf16")
    n, N, M = 4, 2, 2
    img, goal = obs(cfg, n, 2)
    chunks = []
    for g in (goal, goal + 1.0):
        pol = policy(den, cfg, n, multistep=4, candidates=N, contrast=M, seed=30)
        pol.step({"state_images": img}, g)
        torch.cuda.synchronize()
        ent = _entry(pol, n)
        assert torch.equal(ent["goals"].view(n, N + M, -1)[:, :N], g[:, None].expand(n, N, -1)) and not ent["goals"].view(n, N + M, -1)[:, N:].any()
        chunks.append(ent["bufs"][0].view(n, N + M, cfg.action_seq_len, cfg.action_dim).clone())
    a, b = chunks
    assert torch.equal(a[:, N:], b[:, N:]) and torch.isfinite(a).all()
    assert all(not torch.equal(a[i, c], b[i, c]) for i in range(n) for c in range(N))


def test_contrast_weight_is_a_device_scalar_no_recapture(monkeypatch):
    cfg, m, den = build("bf16")
    n, s, N, M = 8, 4, 4, 4
    pol = policy(den, cfg, n, multistep=s, candidates=N, contrast=M, contrast_weight=0.0, seed=50)
    seeds = [50 + b for b in range(n)]
    img, goal = obs(cfg, n, 3)
    pol.step({"state_images": img}, goal)
    assert torch.equal(pol.candidate_scores, pol.coherence_scores[:, :N]) and (pol.selected == 0).all()     # lambda = 0, cold: all totals 0
    keys = list(pol._hooks.store)
    cnt = count_graphs(monkeypatch)
    picks = []
    for lam in (0.0, 1000.0):
        _drain(pol, img, goal, list(range(n)))
        pol.contrast_weight = lam
        assert pol.contrast_weight == lam
        draws, prev, before = pol.draws.cpu().tolist(), pol.plans.clone(), dict(cnt)
        pol.step({"state_images": img}, goal)
        assert cnt["capture"] == before["capture"] and cnt["replay"] == before["replay"] + 1, lam     # the graph captured at weight 0.0
        ref = _bid_reference(pol, den, "ddim", img, goal, seeds, draws, prev, list(range(n)), [True] * n, full=True)
        assert _state_equals(pol, list(range(n)), ref, n), lam
        other = rollout.select_bidirectional(ref[5], prev, [True] * n, s, rollout.coherence_weights(0.5, cfg.action_seq_len - s), M, pol.contrast_topk,
                                             1000.0 - lam)
        picks.append((ref[1].cpu().tolist(), other[1].cpu().tolist()))
    assert any(a != b for a, b in picks)                                                  # the weight decides: the other value selects differently
    assert list(pol._hooks.store) == keys                                                 # (no graph key holds the weight)
    with pytest.raises(ValueError, match="finite float >= 0"):
        pol.contrast_weight = -1.0
    assert pol.contrast_weight == 1000.0


# ------------------------------------------------------------------------------------------------------------------ 4. defaults
def test_contrast_none_is_the_policy_without_the_keyword(monkeypatch):
    cfg, m, den = build("bf16")
    n, steps, s, N = 5, 9, 4, 3
    rng = np.random.default_rng(6)
    active = rng.random((steps, n)) > 0.2
    g = torch.Generator().manual_seed(10)
    obs_t = [torch.randn(n, 2, cfg.obs_dim, generator=g).cuda() for _ in range(steps)]
    goal = torch.randn(n, cfg.goal_dim, generator=g).cuda()
    plain = policy(den, cfg, n, seed=100, multistep=s, candidates=N)
    other = policy(den, cfg, n, seed=100, multistep=s, candidates=N, contrast=None)
    assert other.contrast is None and other.contrast_weight is None and other.contrast_topk is None
    assert type(other._sel) is L.ModeEnvSelectDesc and other._ctrl.numel() == plain._ctrl.numel()
    with pytest.raises(AttributeError, match="without contrast"):
        other.coherence_scores
    with pytest.raises(AttributeError, match="without contrast"):
        other.contrast_weight = 1.0
    plain._lib, other._lib = _CountingLib(plain._lib), _CountingLib(other._lib)
    cnt = count_graphs(monkeypatch)
    graphs = []
    for p in (plain, other):
        before = dict(cnt)
        for t in range(steps):
            if t == 5:
                p.reset(envs=[1, 3], seeds=[501, 503])
            p.step({"state_images": obs_t[t]}, goal, active=active[t])
        graphs.append({k: cnt[k] - before[k] for k in cnt})
    assert torch.equal(plain.plans, other.plans) and torch.equal(plain.draws, other.draws) and torch.equal(plain.selected, other.selected)
    assert torch.equal(plain.candidate_scores, other.candidate_scores)
    assert graphs[0] == graphs[1] and graphs[0]["replay"] >= 2                              # the same captures, the same replays
    assert plain._lib.calls == other._lib.calls and set(other._lib.calls) == {"mode_env_gather_noise_cand", "mode_env_select", "mode_env_commit_emit"}
    assert [k for k, _ in plain._hooks.store.items()] == [k for k, _ in other._hooks.store.items()]


# ------------------------------------------------------------------------------------------------------------------ 5. combinations
def test_contrast_with_warm_start_cold_and_warm_chunks_in_one_step():
    cfg, m, den = build("bf16")
    n, s, N, M, k = 5, 4, 2, 2, 5
    pol = policy(den, cfg, n, multistep=s, candidates=N, contrast=M, warm_start=k, seed=40)
    seeds = [40 + b for b in range(n)]
    img, goal = obs(cfg, n, 6)
    pol.step({"state_images": img}, goal)
    assert pol.replanned == list(range(n)) and pol.replanned_warm == []
    _drain(pol, img, goal, list(range(n)))
    pol.reset(envs=[1, 3])                                                                # -> cold chunk [1, 3] (bucket 2), warm chunk [0, 2, 4] (bucket 4)
    draws, prev = pol.draws.cpu().tolist(), pol.plans.clone()
    out = pol.step({"state_images": img}, goal)
    assert pol.replanned == list(range(n)) and pol.replanned_warm == [0, 2, 4]
    cold = _bid_reference(pol, den, "ddim", img, goal, seeds, draws, prev, [1, 3], [False] * n)
    warm = _bid_reference(pol, den, "ddim", img, goal, seeds, draws, prev, [0, 2, 4, 4], [True] * n, warm_k=k)   # weak rows warm-started alike
    assert _state_equals(pol, [1, 3], cold, 2) and (pol.coherence_scores[[1, 3]] == 0).all()
    assert _state_equals(pol, [0, 2, 4], warm, 3) and (warm[3][:3] > 0).all()
    assert torch.equal(out, pol.plans[:, 0]) and pol.draws.cpu().tolist() == [d + 1 for d in draws]
    assert sorted(b for _, b in pol._hooks.store) == [2 * (N + M), 5 * (N + M)] and [b for _, b in pol._hooks_warm.store] == [4 * (N + M)]


def test_contrast_with_temporal_ensemble_ring_and_plans_receive_the_selection():
    cfg, m, den = build("bf16")
    n, s, N, M = 5, 4, 2, 2
    pol = policy(den, cfg, n, multistep=s, candidates=N, contrast=M, temporal_ensemble=0.5, seed=60)
    seeds = [60 + b for b in range(n)]
    img, goal = obs(cfg, n, 7)
    pol.step({"state_images": img}, goal)
    first = pol.plans.clone()
    assert torch.equal(pol.plan_ring[:, 0], first) and (pol.plan_births[:, 0] == 0).all()
    for _ in range(s - 1):
        pol.step({"state_images": img}, goal)
    draws = pol.draws.cpu().tolist()
    out = pol.step({"state_images": img}, goal)                                           # local time 4: the second plan, scored against the first
    ref = _bid_reference(pol, den, "ddim", img, goal, seeds, draws, first, list(range(n)), [True] * n)
    assert _state_equals(pol, list(range(n)), ref, n) and torch.equal(pol.plan_ring[:, 1], ref[0]) and torch.equal(pol.plan_ring[:, 0], first)
    wt = pol.ensemble_weight_table.double()
    want = (wt[0] * first[:, s].double() + wt[1] * ref[0][:, 0].double()) / (wt[0] + wt[1])     # oldest first
    assert torch.allclose(out.double(), want, rtol=2e-6, atol=1e-6)


def test_uint8_frames_with_contrast_equal_the_policy_fed_the_encoders_own_embeddings():
    """The towers run once per environment (batch mb * T), FiLM on the environment's goal - the first, strong row -, and their rows are
    broadcast to all N + M candidate rows: the weak candidates share the observation embeddings, only the denoiser's goal row is zero.  A policy
    without encoders fed exactly those embeddings then runs the same chain on the same bits."""
    from test_gpu_vector_env import build as build_mode
    cfg, m, den = build_mode("noise", "bf16")
    encs = encoders(cfg)
    n, s, N, M = 3, 2, 2, 2
    kw = dict(act_window_size=cfg.action_seq_len, action_dim=cfg.action_dim, sigma_max=SIGMA_MAX, multistep=s, candidates=N, contrast=M, seed=70)
    pf = rollout.VectorEnvPolicy(den, n, static_resnet=encs[0], gripper_resnet=encs[1], camera_transforms=TRANSFORMS, **kw)
    pe = rollout.VectorEnvPolicy(den, n, **kw)
    for t, envs in enumerate(([0, 1, 2], [0, 1, 2], [0, 2])):                            # buckets 3, -, 2
        ob, goal = u8_frames(cfg, n, 90 + t)
        act = np.zeros(n, dtype=bool)
        act[envs] = True
        a = pf.step(ob, goal, active=act)
        if not pf.replanned:
            assert torch.equal(a, pe.step({"state_images": emb}, goal, active=act)) and pe.replanned == []
            continue
        mb, m_ = next(b for b in (1, 2, 3) if b >= len(pf.replanned)), len(pf.replanned)
        ent, st = _entry(pf, mb), pf._enc_store[mb]
        assert st["bufs"][0].shape[0] == mb and st["bufs"][1].shape[0] == mb              # the towers' batch: mb * T, not mb * (N + M) * T
        tok = ent["img"].view(mb, N + M, 2, cfg.obs_dim)
        assert ent["img"].shape[0] == mb * (N + M) and all(torch.equal(tok[:, c], tok[:, 0]) for c in range(1, N + M))
        gl = ent["goals"].view(mb, N + M, -1)
        assert torch.equal(gl[:m_, 0], goal[pf.replanned].reshape(m_, -1).float()) and not gl[:, N:].any()
        emb = torch.full((n, 2, cfg.obs_dim), float("nan"), device="cuda")                # rows that do not replan are not read
        emb[pf.replanned] = tok[:m_, 0]
        b = pe.step({"state_images": emb}, goal, active=act)
        assert pf.replanned == pe.replanned == envs
        assert torch.equal(a, b) and torch.equal(pf.plans, pe.plans) and torch.isfinite(pf.plans[pf.replanned]).all(), t
        assert torch.equal(pf.selected, pe.selected) and torch.equal(pf.candidate_scores, pe.candidate_scores), t
        assert torch.equal(pf.coherence_scores, pe.coherence_scores) and torch.equal(pf.contrast_scores, pe.contrast_scores), t
