"""Bit-level digest of what the optimizers leave behind: made to be run on two commits and compared line by line.  A host-side change of
``optim.py`` (or of the AdamW entry points of the library) that keeps the launches and their arguments keeps every digest.

The tiny model of the optimizer tests (2 layers, embed_dim 128, 4 heads, 4 experts top-2, B = 8, bf16 compute, seeded weights and inputs).  Per mode:
three optimizer steps, then ONE SHA-256 over the bytes of ``arena.flat``, ``arena.lp``, ``exp_avg``, ``exp_avg_sq`` and the EMA buffer (where the
mode has one); the ``FlatAdamW`` modes hash every parameter and both moments of a handful of small fp32 tensors, one of them left without a gradient.
Only the public API is used (constructors, ``step(...)`` keywords, ``state_dict()``), so the identical file runs on an older checkout.  The modes
``serial`` and ``flat-*`` overwrite the gradients with seeded values and cannot depend on the backward; every other mode takes its gradients from
the real backward chain (so run a commit twice before trusting a comparison of those).

Every mode runs in a fresh child process under its own time limit; the driver stops at the first child that does not exit 0.

    python scripts/optim_state_digest.py [--root TREE] [--out FILE]     (TREE: another checkout to import the package and the oracle from)
    python scripts/optim_state_digest.py --compare A.txt B.txt [--skip mode,mode]   -> exit status 1 on any difference"""
import hashlib
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = ["serial", "overlap", "frozen-router", "ema", "clip-serial", "clip-overlap", "skip-nonfinite", "bf16-serial", "bf16-overlap",
         "fuse-registered-ema", "fuse-step-ema", "flat-fp32", "flat-clipped", "flat-bf16", "flat-joint-clip"]
CHILD_LIMIT = 180                                                                     # seconds per mode (a mode takes a few)
KW = dict(lr=1e-3, betas=(0.9, 0.95), weight_decay=0.05)
GROUPS = [[(5,), (1000,), (7,), (8, 4, 3, 3), (3,)], [(1,), (130,)]]                  # group 0, tensor 2 never gets a gradient
NO_GRAD = (0, 2)


def child(mode, root):
    sys.path.insert(0, root)
    import torch
    import mode_diffusion_policy_amd as M
    from mode_diffusion_policy_amd.optim import ArenaEMA, FlatAdamW, FusedAdamW, GradClip
    from oracle import mode_oracle as O
    from oracle.weights import make_inputs, make_state_dict

    h = hashlib.sha256()

    def feed(*tensors):
        torch.cuda.synchronize()
        for t in tensors:
            t = t.detach().contiguous()
            h.update(t.view(torch.int32 if t.element_size() == 4 else torch.int16).cpu().numpy().tobytes())

    def setup(seed):
        cfg = O.DiTConfig(obs_dim=64, goal_dim=32, action_dim=7, embed_dim=128, n_layers=2, n_heads=4, action_seq_len=10, num_experts=4, top_k=2)
        m = M.MoDeDiT(obs_dim=cfg.obs_dim, goal_dim=cfg.goal_dim, device="cuda", goal_conditioned=True, action_dim=7, embed_dim=cfg.embed_dim,
                      embed_pdrob=0, attn_pdrop=0.0, n_layers=cfg.n_layers, n_heads=cfg.n_heads, goal_seq_len=1, obs_seq_len=1, action_seq_len=10,
                      mlp_pdrop=0.0, goal_drop=0.0, num_experts=cfg.num_experts, top_k=cfg.top_k, use_argmax=True, compute_dtype="bf16")
        m.load_state_dict(make_state_dict(cfg, seed))
        m = m.to("cuda").train()
        inp = {k: v.cuda() for k, v in make_inputs(cfg, 8, 3).items()}
        den = M.GCDenoiser(m, 0.5).train()
        sig = torch.full((8,), 0.9, device="cuda")

        def backward():
            loss, _ = den.loss({"state_images": inp["state_images"]}, inp["actions"], inp["goals"], inp["noise"], sig)
            loss.backward()
        return m, backward

    def seeded_arena_grad(m, step):
        g = m.engine.arena.grad
        g.copy_((torch.randn(g.numel(), generator=torch.Generator().manual_seed(2000 + step)) * 1e-2).to(g.device))

    def flat_groups(seed):
        gen = torch.Generator().manual_seed(seed)
        groups = []
        for gi, shapes in enumerate(GROUPS):
            ps = []
            for s in shapes:
                t = torch.randn(s, generator=gen).cuda()
                ps.append(torch.nn.Parameter(t.contiguous(memory_format=torch.channels_last) if len(s) == 4 else t))
            groups.append(dict(params=ps, weight_decay=0.05 if gi == 0 else 0.0))
        return groups

    def set_flat_grads(groups, step, scale=1.0):
        gen = torch.Generator().manual_seed(1000 + step)
        for gi, shapes in enumerate(GROUPS):
            for pi, s in enumerate(shapes):
                g = (torch.randn(s, generator=gen) * scale).cuda()
                g = g.contiguous(memory_format=torch.channels_last) if len(s) == 4 else g
                groups[gi]["params"][pi].grad = None if (gi, pi) == NO_GRAD else g

    def feed_fused(m, opt, ema=None):
        ar, sd = m.engine.arena, opt.state_dict()
        feed(ar.flat, ar.lp, sd["exp_avg"], sd["exp_avg_sq"], *([] if ema is None else [ema.flat]))

    def feed_flat(groups, opt):
        sd = opt.state_dict()
        feed(*[p for g in groups for p in g["params"]], *sd["exp_avg"], *sd["exp_avg_sq"])

    if mode.startswith("flat-"):
        groups = flat_groups(5)
        m = fused = None
        if mode == "flat-fp32":
            opt = FlatAdamW(groups, lr=1e-2)
        elif mode == "flat-clipped":
            opt = FlatAdamW(groups, lr=1e-2, clip=GradClip(max_norm=0.05))
        elif mode == "flat-bf16":
            opt = FlatAdamW(groups, lr=1e-2, moment_dtype="bf16", round_seed=77)
        else:                                                                         # joint clip: the denoiser's FusedAdamW and a FlatAdamW under one norm
            clip = GradClip(max_norm=0.05)
            m, backward = setup(61)
            fused, opt = FusedAdamW(m, clip=clip, **KW), FlatAdamW(groups, lr=1e-2, clip=clip)
        for step in range(1, 4):
            set_flat_grads(groups, step, scale=1e-2 if fused is not None else 1.0)
            if fused is not None:
                backward()
                seeded_arena_grad(m, step)                                            # after the backward: the mode does not depend on its bits
                clip.measure()
                fused.step()
                opt.step()
            else:
                opt.step(grad_scale=0.5)
        feed_flat(groups, opt)
        if fused is not None:
            feed_fused(m, fused)
    else:
        m, backward = setup(11)
        ema, step_kw, inf_at = None, {}, None
        if mode == "serial":
            opt = FusedAdamW(m, **KW)
        elif mode == "overlap":
            opt, step_kw = FusedAdamW(m, **KW), dict(overlap=True)
        elif mode == "frozen-router":
            m.freeze_router()
            opt = FusedAdamW(m, **KW)
        elif mode == "ema":
            opt, ema = FusedAdamW(m, **KW), ArenaEMA(m, decay=0.99, min_value=0.5)
            step_kw = dict(ema=ema)
        elif mode in ("clip-serial", "clip-overlap", "skip-nonfinite"):
            opt = FusedAdamW(m, clip=GradClip(max_norm=0.05, skip_nonfinite=True), **KW)
            step_kw = dict(overlap=mode == "clip-overlap")
            inf_at = 2 if mode == "skip-nonfinite" else None
        elif mode in ("bf16-serial", "bf16-overlap"):
            opt = FusedAdamW(m, moment_dtype="bf16", round_seed=0xC0FFEE, **KW)
            step_kw = dict(overlap=mode == "bf16-overlap")
        elif mode in ("fuse-registered-ema", "fuse-step-ema"):
            opt, ema = FusedAdamW(m, fuse_expert_step=True, **KW), ArenaEMA(m, decay=0.99, min_value=0.5)
            if mode == "fuse-registered-ema":
                opt.fused_ema = ema
            else:
                ema.ensure(m.engine.arena)                                            # exists before the first backward: averaged from the pre-update weights
                step_kw = dict(ema=ema)
        else:
            raise SystemExit(f"unknown mode {mode}")
        for step in range(1, 4):
            backward()
            if mode == "serial":
                seeded_arena_grad(m, step)
            if step == inf_at:
                ar = m.engine.arena
                ar.grad[ar.offset("l0.w1") + 1234] = float("inf")
            opt.step(**step_kw)
        assert opt.step_count == 3
        if inf_at is not None:
            assert int(opt.clip.skipped) == 1
        feed_fused(m, opt, ema)
    print(f"DIGEST {mode} {h.hexdigest()}", flush=True)


def drive(root, out):
    lines = []
    for mode in MODES:
        cmd = [sys.executable, os.path.abspath(__file__), "--child", mode, "--root", root]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=CHILD_LIMIT)
        except subprocess.TimeoutExpired:
            print(f"{mode}: no result within {CHILD_LIMIT} s - stopping", flush=True)
            return 1
        got = [ln for ln in r.stdout.splitlines() if ln.startswith("DIGEST ")]
        if r.returncode != 0 or len(got) != 1:
            print(f"{mode}: exit status {r.returncode} - stopping\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}", flush=True)
            return 1
        _, name, digest = got[0].split()
        lines.append(f"{name:<22}{digest}")
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
    if args[:1] == ["--compare"]:
        sys.exit(compare(args[1], args[2], [s for s in (opt("--skip") or "").split(",") if s]))
    root = os.path.abspath(opt("--root", HERE))
    if "--child" in args:
        child(opt("--child"), root)
    else:
        sys.exit(drive(root, opt("--out")))
