"""Bit-level digest of what the vector-environment kernels (csrc/env_pool.hip) and ``rollout.VectorEnvPolicy`` compute: made to be run on two
commits and compared line by line (the precedent: scripts/optim_state_digest.py).  A change of ``rollout.py`` or of ``env_pool.hip`` that keeps
the launches, their arguments and the kernels' arithmetic keeps every digest.  Only names of the public API, of ``_lib`` and of the library's
exports are used, so the identical file runs on an older checkout (``--root``).

Tier (a), the kernels alone on seeded inputs, one SHA-256 per case over the raw bytes of every output buffer, guard words included:
  gather   env_noise / env_warm_latents at (W, A) in {(1, 1), (10, 7), (64, 64)}, shift 1 and W - 1, seeds and draws up to 2**32 - 1; every
           gather export (plain, _cand at N in {1, 2, 64}, _bid at (N, M) in {(1, 1), (4, 4), (32, 32)}, cold and warm) with observation and goal
           rows, a padding row, a repeated row and two row indices outside [0, num_envs)
  select   select_coherent at N in {1, 2, 64} with (W - shift) * A in {1, 63, 65, 4095}, 33 rows (two mask words) with mixed has_prev, a NaN
           candidate, an all-NaN row and an exact tie; select_bidirectional at (N, M, K) in {(1, 1, 1), (4, 4, 4), (8, 3, 64), (32, 32, 2)}, lambda
           0 and 1, the same rows
  commit   mode_env_commit_emit and mode_env_commit_emit_ens (K in {1, 2, 9, 10}, ring slots reset to -1) in the control-block form with
           m in {0, 1, num_envs} and in the descriptor form, num_envs in {1, 33}, inactive rows
  frames   mode_env_gather_frames fp32 -> fp32, fp32 -> bf16, bf16 -> bf16 at row lengths 7, 8 and 8 * 256 * 4 + 3, even and odd source pitch
Tier (b), the policy on the c1e4 model of the tests (bf16), 5 environments, 12 steps with the tests' staggered resets and active masks, per
configuration one SHA-256 over every step's output and the final plans, draws, selected, candidate_scores, plan_ring and plan_births.

Every group runs in a fresh child process under its own time limit; the driver stops at the first child that does not exit 0.

    python scripts/vector_env_digest.py [--root TREE] [--out FILE] [--only group,group]
    python scripts/vector_env_digest.py --compare A.txt [B.txt] [--skip name,name]   (one file: against a run of this tree) -> exit status 1 on
    any difference"""
import ctypes as C
import hashlib
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNEL_GROUPS = ["gather", "select", "commit", "frames"]
POLICY_GROUPS = ["plain", "ensemble", "warm", "cand", "contrast", "all", "frames-f32", "frames-u8"]
CHILD_LIMIT = 300                                                                     # seconds per group (a group takes a few)
SENTINEL, GUARD = -777.0, 64


def child(group, root):
    sys.path.insert(0, root)
    import numpy as np
    import torch
    import mode_diffusion_policy_amd as M
    from mode_diffusion_policy_amd import _lib as L
    from mode_diffusion_policy_amd import rollout

    lib = L.load()
    stream = lambda: torch.cuda.current_stream().cuda_stream                          # noqa: E731
    U32 = 2 ** 32 - 1

    def emit(name, *tensors):
        torch.cuda.synchronize()
        h = hashlib.sha256()
        for t in tensors:
            t = t.detach().contiguous().cpu()
            h.update(t.view(torch.uint8).numpy().tobytes())
        print(f"DIGEST {name} {h.hexdigest()}", flush=True)

    def guarded(n, dtype=torch.float32, fill=SENTINEL):
        """(the n payload elements as a view, the whole buffer with GUARD sentinel elements on either side)"""
        buf = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device="cuda")
        return buf[GUARD:GUARD + n], buf

    def randn(seed, *shape):
        return torch.from_numpy(np.random.default_rng(seed).standard_normal(shape).astype(np.float32)).cuda()

    def i32(values):
        return rollout._u32_as_i32(values).cuda()

    # ------------------------------------------------------------------------------------------------------------------ tier (a)
    def gathers():
        seeds, draws = [0, 1, U32, 12345, U32], [0, U32, U32, 7, 1]
        for W, A in ((1, 1), (10, 7), (64, 64)):
            emit(f"env_noise-{W}x{A}", rollout.env_noise(seeds, draws, W, A, 80.0))
            for shift in [sh for sh in sorted({1, W - 1}) if 1 <= sh < W]:            # (W = 1 has no legal shift)
                emit(f"env_warm_latents-{W}x{A}-shift{shift}", rollout.env_warm_latents(randn(W * A + shift, 5, W, A), seeds, draws, shift, 2.5))
        n, W, A, shift, IMG, G = 5, 10, 7, 4, 6, 3
        rows = [3, 0, -1, n, 4, 1, 1, 1]                                              # two entries out of range; padding by repetition
        r, s, d = torch.tensor(rows, dtype=torch.int32, device="cuda"), i32(seeds), i32(draws)
        img, goals, plan = randn(1, n, IMG), randn(2, n, G), randn(3, n, W, A)
        kinds = [("", 1, 0)] + [("_cand", N, 0) for N in (1, 2, 64)] + [("_bid", N, Mw) for N, Mw in ((1, 1), (4, 4), (32, 32))]
        for kind, N, Mw in kinds:
            per = {"": (), "_cand": (N,), "_bid": (N, Mw)}[kind]
            B = len(rows) * (N + Mw)
            for warm in (False, True):
                (x, xb), (io, iob), (go, gob) = guarded(B * W * A), guarded(B * IMG), guarded(B * G)
                head = (r.data_ptr(), len(rows), n, s.data_ptr(), d.data_ptr(), img.data_ptr(), IMG, goals.data_ptr(), G, io.data_ptr(), go.data_ptr(),
                        x.data_ptr())
                if warm:
                    L.check(getattr(lib, "mode_env_gather_warm" + kind)(*head, plan.data_ptr(), W, A, shift, 2.5, *per, stream()), "gather_warm" + kind)
                else:
                    L.check(getattr(lib, "mode_env_gather_noise" + kind)(*head, W * A, 80.0, *per, stream()), "gather_noise" + kind)
                emit(f"gather{kind}-{'warm' if warm else 'noise'}-N{N}-M{Mw}", xb, iob, gob)

    def selection_rows(seed, n, NT, N, W, A):
        """Seeded candidates around the previous plans' tails; row 1: a NaN in candidate 0, row 2: a NaN in every candidate, row 3: candidates 0
        and 1 (of N >= 2) identical."""
        prev = randn(seed, n, W, A)
        chunk = 0.5 * randn(seed + 1, n, NT, W, A) + prev[:, None]
        chunk[1, 0, 0, 0] = float("nan")                                              # (element 0 is scored at every shift)
        chunk[2, :, 0, 0] = float("nan")
        if N >= 2:
            chunk[3, 1] = chunk[3, 0]
        has = np.arange(n) % 3 != 0
        has[1:4] = True
        return chunk, prev, has

    def selects():
        n = 33
        for N in (1, 2, 64):
            for W, A, shift in ((2, 1, 1), (10, 7, 1), (14, 5, 1), (4096, 1, 1)):   # (W - shift) * A = 1, 63, 65, 4095
                chunk, prev, has = selection_rows(N + W, n, N, N, W, A)
                emit(f"select_coherent-N{N}-{W}x{A}-shift{shift}", *rollout.select_coherent(chunk, prev, has, shift, rollout.coherence_weights(0.99, W - shift)))
        W, A, shift = 10, 7, 4
        for N, Mw, K in ((1, 1, 1), (4, 4, 4), (8, 3, 64), (32, 32, 2)):
            chunk, prev, has = selection_rows(100 + N, n, N + Mw, N, W, A)
            for lam in (0.0, 1.0):
                emit(f"select_bidirectional-N{N}-M{Mw}-K{K}-lambda{lam:g}",
                     *rollout.select_bidirectional(chunk, prev, has, shift, rollout.coherence_weights(0.99, W - shift), Mw, K, lam))

    def commits():
        A = 7
        for ens, W, s in [(False, 10, 4)] + [(True, Wk, sk) for Wk, sk in ((10, 10), (10, 5), (9, 1), (10, 1))]:
            K = -(-W // s)
            for n in (1, 33):
                nw = (n + 31) // 32
                rng = np.random.default_rng(1000 * W + 10 * s + n)
                for m in sorted({0, 1, n}) + [None]:                                   # None: the descriptor form (no control block)
                    plan, (out, outb) = randn(n + W, n, W, A), guarded(n * A)
                    t_np = rng.integers(0, 3 * W, n)
                    counter = torch.from_numpy((t_np % s).astype(np.int32)).cuda()
                    draws = i32(rng.integers(0, 2 ** 32, n).tolist())
                    active = rng.random(n) > 0.3
                    words = rollout._mask_words(active, nw)
                    d = L.ModeEnvPoolDesc(num_envs=n, W=W, A=A, multistep=s, plan=plan.data_ptr(), counter=counter.data_ptr(), draws=draws.data_ptr())
                    keep = []
                    if m is None:
                        d.out = out.data_ptr()
                        C.memmove(d.active, words.ctypes.data, 4 * nw)
                    else:
                        mb = max(m, 1)
                        rows = rng.permutation(n)[:m].astype(np.int32)
                        rows = np.concatenate([rows, np.full(mb - m, rows[-1] if m else 0, dtype=np.int32)])
                        ctrl = np.zeros(4 + nw + n, dtype=np.int32)
                        ctrl[0] = m
                        ctrl[2:4] = np.array([out.data_ptr()], dtype="<u8").view("<i4")
                        ctrl[4:4 + nw] = words.view("<i4")
                        ctrl[4 + nw:4 + nw + mb] = rows
                        keep = [torch.from_numpy(ctrl).cuda(), randn(n + W + 1, mb, W, A)]
                        d.ctrl, d.chunk = keep[0].data_ptr(), keep[1].data_ptr()
                    name = f"commit{'_ens' if ens else ''}-W{W}-s{s}-n{n}-{'desc' if m is None else 'ctrl-m%d' % m}"
                    if not ens:
                        L.check(lib.mode_env_commit_emit(C.byref(d), stream()), name)
                        emit(name, outb, plan, counter, draws)
                        continue
                    # a ring consistent with the local times: the plan of age i born at tn - i * s in its slot, some slots reset to -1
                    birth_np = np.full((n, K), -1, dtype=np.int32)
                    for b in range(n):
                        t = int(t_np[b])
                        tn, q = t - t % s, (t // s) % K
                        for i in range(K):
                            if tn - i * s >= 0 and rng.random() > 0.3:
                                birth_np[b, (q + K - i) % K] = tn - i * s
                    ring, birth = randn(n + W + 2, n, K, W, A), torch.from_numpy(birth_np).cuda()
                    tt = torch.from_numpy(t_np.astype(np.int32)).cuda()
                    wts = torch.from_numpy(rollout.ensemble_weights(0.1, K)).cuda()
                    e = L.ModeEnvEnsDesc(ring=ring.data_ptr(), birth=birth.data_ptr(), t=tt.data_ptr(), weights=wts.data_ptr(), K=K)
                    e.pool = d
                    L.check(lib.mode_env_commit_emit_ens(C.byref(e), stream()), name)
                    emit(name, outb, plan, counter, draws, ring, birth, tt)

    def frame_gathers():
        n, rows = 7, [5, 2, 2, 9, -1, 0, 5]
        r = torch.tensor(rows, dtype=torch.int32, device="cuda")
        dt = {torch.float32: L.MODE_F32, torch.bfloat16: L.MODE_BF16}
        for src_dt, dst_dt in ((torch.float32, torch.float32), (torch.float32, torch.bfloat16), (torch.bfloat16, torch.bfloat16)):
            for row in (7, 8, 8 * 256 * 4 + 3):
                for pitch in (row, row + 2 + (row % 2 == 0)):                         # the second one odd
                    src = randn(row + pitch, n, pitch).to(src_dt)
                    src[5, :3] = torch.tensor([float("nan"), 1.00390625, -3.0e38]).to(src_dt)
                    other = randn(row + pitch + 1, n, 75)
                    (dst, dstb), (dst2, dst2b) = guarded(len(rows) * row, dst_dt), guarded(len(rows) * 75)
                    d = L.ModeEnvFramesDesc(rows=r.data_ptr(), m_b=len(rows), num_envs=n)
                    d.cam[0] = L.ModeEnvFramesCam(src=src.data_ptr(), src_stride=pitch, row_elems=row, dst=dst.data_ptr(), src_dtype=dt[src_dt],
                                                  dst_dtype=dt[dst_dt])
                    d.cam[1] = L.ModeEnvFramesCam(src=other.data_ptr(), src_stride=75, row_elems=75, dst=dst2.data_ptr(), src_dtype=L.MODE_F32,
                                                  dst_dtype=L.MODE_F32)
                    L.check(lib.mode_env_gather_frames(C.byref(d), stream()), "gather_frames")
                    emit(f"gather_frames-{str(src_dt)[6:]}-{str(dst_dt)[6:]}-row{row}-pitch{pitch}", dstb, dst2b)

    # ------------------------------------------------------------------------------------------------------------------ tier (b)
    def policy_run(config):
        import dataclasses
        from oracle.weights import get_config, make_state_dict
        cfg = dataclasses.replace(get_config("c1e4"))
        m = M.MoDeDiT(obs_dim=cfg.obs_dim, goal_dim=cfg.goal_dim, device="cuda", goal_conditioned=True, action_dim=cfg.action_dim,
                      embed_dim=cfg.embed_dim, embed_pdrob=0, attn_pdrop=0.3, n_layers=cfg.n_layers, n_heads=cfg.n_heads, goal_seq_len=1,
                      obs_seq_len=1, action_seq_len=cfg.action_seq_len, num_experts=cfg.num_experts, top_k=cfg.top_k, compute_dtype="bf16")
        m.load_state_dict(make_state_dict(cfg, 210))
        den = M.GCDenoiser(m.to("cuda").eval(), 0.5).eval()
        n, steps, s = 5, 12, 4
        kw = {"plain": {}, "ensemble": dict(temporal_ensemble=0.1), "warm": dict(warm_start=3), "cand": dict(candidates=4),
              "contrast": dict(candidates=4, contrast=2), "all": dict(candidates=4, contrast=2, warm_start=3, temporal_ensemble=0.1),
              "frames-f32": {}, "frames-u8": {}}[config]
        g = torch.Generator().manual_seed(9)
        if config.startswith("frames"):
            from oracle import resnet_oracle as R
            encs = []
            for seed in (1, 2):
                e = M.FiLMResNet18Policy(cfg.goal_dim).cuda().eval()
                e.load_state_dict({k: v.cuda() for k, v in R.fill_encoder_state_dict(e.state_dict(), seed).items()})
                encs.append(e)
            kw.update(static_resnet=encs[0], gripper_resnet=encs[1])
            if config == "frames-u8":
                kw.update(camera_transforms={"rgb_static": M.CameraTransform((64, 64)),
                                             "rgb_gripper": M.CameraTransform((64, 64), mean=(0.5, 0.4, 0.3), std=(0.2, 0.25, 0.3))})
                obs_t = [{"rgb_obs": {"rgb_static": torch.randint(0, 256, (n, 1, 48, 40, 3), dtype=torch.uint8, generator=g).cuda(),
                                      "rgb_gripper": torch.randint(0, 256, (n, 1, 20, 20, 3), dtype=torch.uint8, generator=g).cuda()}}
                         for _ in range(steps)]
            else:
                obs_t = [{"rgb_obs": {"rgb_static": torch.randn(n, 1, 3, 64, 64, generator=g).cuda(),
                                      "rgb_gripper": torch.randn(n, 1, 3, 64, 64, generator=g).cuda()}} for _ in range(steps)]
        else:
            obs_t = [{"state_images": torch.randn(n, 2, cfg.obs_dim, generator=g).cuda()} for _ in range(steps)]
        goal = torch.randn(n, cfg.goal_dim, generator=g).cuda()
        rng = np.random.default_rng(5)
        resets = {t: sorted(rng.choice(n, size=int(rng.integers(1, 3)), replace=False).tolist()) for t in (2, 5, 9)}
        active = rng.random((steps, n)) > 0.2
        pol = rollout.VectorEnvPolicy(den, n, seed=100, multistep=s, act_window_size=cfg.action_seq_len, action_dim=cfg.action_dim, sigma_max=80.0, **kw)
        outs = []
        for t in range(steps):
            if t in resets:
                pol.reset(envs=resets[t], seeds=[1000 * t + b for b in resets[t]])
            outs.append(pol.step(obs_t[t], goal, active=active[t]).clone())
        state = [pol.plans, pol.draws]
        if kw.get("candidates"):
            state += [pol.selected, pol.candidate_scores]
        if kw.get("temporal_ensemble") is not None:
            state += [pol.plan_ring, pol.plan_births]
        emit(f"policy-{config}", *outs, *state)

    kernels = dict(gather=gathers, select=selects, commit=commits, frames=frame_gathers)
    with torch.no_grad():
        kernels[group]() if group in kernels else policy_run(group[len("policy-"):])


def drive(root, out, only):
    groups = KERNEL_GROUPS + ["policy-" + g for g in POLICY_GROUPS]
    lines = []
    for group in [g for g in groups if not only or g in only]:
        cmd = [sys.executable, os.path.abspath(__file__), "--child", group, "--root", root]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=CHILD_LIMIT)
        except subprocess.TimeoutExpired:
            print(f"{group}: no result within {CHILD_LIMIT} s - stopping", flush=True)
            return 1
        got = [ln.split() for ln in r.stdout.splitlines() if ln.startswith("DIGEST ")]
        if r.returncode != 0 or not got:
            print(f"{group}: exit status {r.returncode} - stopping\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}", flush=True)
            return 1
        for _, name, digest in got:
            lines.append(f"{name:<56} {digest}")
            print(lines[-1], flush=True)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


def compare(a_path, b_path, skip):
    a, b = (dict(ln.split() for ln in open(p) if ln.strip()) for p in (a_path, b_path))
    bad = [k for k in sorted(set(a) | set(b)) if k not in skip and a.get(k) != b.get(k)]
    print(f"{len((set(a) | set(b)) - set(skip))} digests compared, {len(bad)} differ" + (f": {', '.join(bad)}" if bad else ""))
    return 1 if bad else 0


if __name__ == "__main__":
    args = sys.argv[1:]
    opt = lambda k, d=None: args[args.index(k) + 1] if k in args else d              # noqa: E731
    root = os.path.abspath(opt("--root", HERE))
    skip = [s for s in (opt("--skip") or "").split(",") if s]
    if "--child" in args:
        child(opt("--child"), root)
    elif args[:1] == ["--compare"]:
        files = [a for a in args[1:3] if not a.startswith("--")]
        if len(files) == 1:                                                            # against a run of this tree
            with tempfile.TemporaryDirectory() as tmp:
                now = os.path.join(tmp, "now.txt")
                sys.exit(drive(root, now, None) or compare(files[0], now, skip))
        sys.exit(compare(files[0], files[1], skip))
    else:
        sys.exit(drive(root, opt("--out"), [g for g in (opt("--only") or "").split(",") if g]))
