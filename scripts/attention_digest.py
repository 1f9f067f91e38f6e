"""Bit-level digest of what the attention kernels (csrc/attn.hip, attn_long.hip, attn_core.h, qkv_attn.hip) compute: made to be run on two builds
of the library and compared line by line (the precedents: scripts/optim_state_digest.py, scripts/vector_env_digest.py).  A change of those files that
keeps the kernels' arithmetic keeps every digest.  The library is chosen with MODE_HIP_LIB; the Python side is this tree's.

One SHA-256 per case over the status and the raw bytes of every output buffer, canary rows included.  Seeded inputs from tests/attn_refs.py:
  kernels  mode_attn_block_fwd at every case of fwd_cases at every T of FWD_SHORT_T + FWD_LONG_T, both dtypes, p = 0 and 0.3; mode_attn_block_bwd at
           every case of bwd_cases at every T of BWD_SHORT_T + BWD_LONG_T, both dtypes, with "attn_bwd_mfma" 1 and (T <= 16, head_dim % 16 == 0) 0
  fused    mode_qkv_attn_fwd at FUSED_T x FUSED_B with the padded leading dimensions and the four geometries of tests/test_gpu_attention_edges.py
  train    the gradients of the packed QKV bias and of the qk-norm gains after one training backward (they reach the per-sample bias partial of the
           attention backward) at a 10-step and a 20-step action chunk (T = 14 and T = 24), fp32 and bf16: the smallest training configuration of
           tests/test_gpu_long_chunk_model.py
Every group runs in a fresh child process under its own time limit; the driver stops at the first child that does not exit 0.

    python scripts/attention_digest.py [--out FILE] [--only group,group]
    python scripts/attention_digest.py --compare A.txt B.txt [C.txt]     three files: A and B are two runs of one build - the digests that differ
                                                                         between them are named and left out - and C is the other build
                                                                         -> exit status 1 on any difference
    python scripts/attention_digest.py --perf N       N launches per kernel and shape after 20 warm-up launches, at the shapes users run (B = 128,
                                                      H = 8, head_dim 128, p = 0.3, T = 14 / 24 / 64, both dtypes, forward and backward, T = 14 in both
                                                      forms of the backward): the workload for `rocprofv3 --kernel-trace --stats -- python ...`"""
import hashlib
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GROUPS = ["kernels", "fused", "train"]
CHILD_LIMIT = 600                                                                     # seconds per group (a group takes well under a minute)
SEED = 1234


def child(group):
    sys.path[:0] = [HERE, os.path.join(HERE, "tests")]
    import torch
    import attn_refs as R
    import hip_helpers as H
    from mode_diffusion_policy_amd import _lib as L

    lib = L.load()
    dev = lambda t: t.to("cuda")                                                      # noqa: E731
    dname = {torch.bfloat16: "bf16", torch.float32: "fp32"}

    def emit(name, rc, *tensors):
        torch.cuda.synchronize()
        h = hashlib.sha256(str(rc).encode())
        for t in tensors:
            h.update(t.detach().contiguous().cpu().view(torch.uint8).numpy().tobytes())
        print(f"DIGEST {name} {h.hexdigest()}", flush=True)

    if group == "kernels":
        for dtype in (R.BF16, R.F32):
            for T in R.FWD_SHORT_T + R.FWD_LONG_T:
                for B, Hh, hd, fam in R.fwd_cases(dtype, T):
                    inp = R.make_inputs(fam, B, T, Hh, hd, dtype)
                    for p in (0.0, 0.3):
                        y = H.Guarded(B * T, Hh * hd, dtype)
                        rc = H.attn(dev(inp.qkv), dev(inp.qg), dev(inp.kg), B, T, Hh, hd, seed=SEED, p_drop=p, out=y)
                        emit(f"fwd/{dname[dtype]}/T{T}/B{B}/H{Hh}/hd{hd}/{fam}/p{p}", rc, y.buf)
            for T in R.BWD_SHORT_T + R.BWD_LONG_T:
                for B, Hh, hd, fam, p in R.bwd_cases(dtype, T):
                    inp = R.make_inputs(fam, B, T, Hh, hd, dtype)
                    for mfma in (1, 0) if T <= 16 and hd % 16 == 0 else (1,):
                        assert lib.mode_set_option(b"attn_bwd_mfma", mfma) == 0
                        try:
                            rc, dqkv, pq, pk = H.attn_bwd(dev(inp.qkv), dev(inp.qg), dev(inp.kg), dev(inp.dy), B, T, Hh, hd, seed=SEED, p_drop=p)
                        finally:
                            lib.mode_set_option(b"attn_bwd_mfma", 1)
                        emit(f"bwd/{dname[dtype]}/T{T}/B{B}/H{Hh}/hd{hd}/{fam}/p{p}/mfma{mfma}", rc, dqkv.buf, pq.buf, pk.buf)
    elif group == "fused":
        Hh, hd = 2, 128
        D = Hh * hd
        for T in R.FUSED_T:
            for B in R.FUSED_B:
                for r in range(3):
                    ph, pw, py = (R.FUSED_PAD[(r + k) % 3] for k in range(3))
                    s = 100 * T + 10 * B + r
                    hbuf = R.rnd(B * T, D + ph, seed=s).to(R.BF16)
                    hbuf[(B * T) // 2] = 0
                    wbuf = (R.rnd(3 * D, D + pw, seed=s + 1) * D ** -0.5).to(R.BF16)
                    qg, kg = dev((3 + 0.1 * R.rnd(hd, seed=s + 2)).float()), dev((3 + 0.1 * R.rnd(hd, seed=s + 3)).float())
                    h, w, bias = dev(hbuf)[:, :D], dev(wbuf)[:, :D], torch.zeros(3 * D, device="cuda")
                    try:
                        for waves, w3 in ((8, 1), (8, 0), (4, 1), (4, 0)):
                            assert lib.mode_set_option(b"qkv_attn_waves", waves) == 0 and lib.mode_set_option(b"qkv_attn_w3", w3) == 0
                            out = H.Guarded(B * T, D + py, R.BF16)
                            rc, _ = H.qkv_attn(h, w, bias, qg, kg, B, T, Hh, D=D, out=out)
                            emit(f"fused/T{T}/B{B}/pad{ph}-{pw}-{py}/waves{waves}/w3{w3}", rc, out.buf)
                    finally:
                        lib.mode_set_option(b"qkv_attn_waves", 8); lib.mode_set_option(b"qkv_attn_w3", 1)
    elif group == "train":
        import mode_diffusion_policy_amd as M
        from oracle import mode_oracle as O
        from oracle.weights import make_inputs, make_state_dict

        for A_len in (10, 20):
            for dtype in ("fp32", "bf16"):
                cfg = O.DiTConfig(obs_dim=64, goal_dim=32, action_dim=14, embed_dim=256, n_layers=2, n_heads=4, action_seq_len=A_len, num_experts=4, top_k=2)
                m = M.MoDeDiT(obs_dim=cfg.obs_dim, goal_dim=cfg.goal_dim, device="cuda", goal_conditioned=True, action_dim=cfg.action_dim,
                              embed_dim=cfg.embed_dim, embed_pdrob=0, n_layers=cfg.n_layers, n_heads=cfg.n_heads, goal_seq_len=1, obs_seq_len=1,
                              action_seq_len=A_len, state_dim=None, num_experts=cfg.num_experts, top_k=cfg.top_k, compute_dtype=dtype, attn_pdrop=0.0,
                              mlp_pdrop=0.0, goal_drop=0.0, use_argmax=True)
                m.load_state_dict(make_state_dict(cfg, 300 + A_len))
                m = m.to("cuda").train()
                c = {k: v.cuda() for k, v in make_inputs(cfg, 6, 301 + A_len).items()}
                sig = torch.linspace(0.2, 2.0, 6, device="cuda")
                loss, _ = M.GCDenoiser(m, 0.5).train().loss({"state_images": c["state_images"]}, c["actions"], c["goals"], c["noise"], sig)
                loss.backward()
                grads = [p.grad for n, p in sorted(m.named_parameters()) if ".attn." in n and (n.endswith(".bias") or n.endswith("_norm.g"))]
                assert len(grads) == 5 * cfg.n_layers and all(g is not None for g in grads)
                emit(f"train/{dtype}/T{A_len + 4}/dbqkv+dgains", 0, *grads)
    else:
        raise SystemExit(f"unknown group {group}")


def perf(n, warm=20):
    sys.path[:0] = [HERE, os.path.join(HERE, "tests")]
    import torch
    import hip_helpers as H
    from mode_diffusion_policy_amd import _lib as L

    lib = L.load()
    B, Hh, hd, p = 128, 8, 128, 0.3
    D = Hh * hd
    torch.manual_seed(0)
    for T in (14, 24, 64):
        for dtype in (torch.bfloat16, torch.float32):
            qkv, dy = torch.randn(B * T, 3 * D, device="cuda").to(dtype), torch.randn(B * T, D, device="cuda").to(dtype)
            qg, kg = 1 + 0.1 * torch.randn(hd, device="cuda"), 1 + 0.1 * torch.randn(hd, device="cuda")
            y, dqkv = torch.empty(B * T, D, device="cuda", dtype=dtype), torch.empty(B * T, 3 * D, device="cuda", dtype=dtype)
            pq, pk = torch.empty(B * Hh, hd, device="cuda"), torch.empty(B * Hh, hd, device="cuda")
            a = (H.p(qkv), H.p(qg), H.p(kg))
            for _ in range(warm + n):
                L.check(lib.mode_attn_block_fwd(*a, H.p(y), H.dt_of(qkv), B, T, Hh, hd, 1e-6, SEED, p, H.stream()), "attn")
            for mfma in (1, 0) if T <= 16 else (1,):
                assert lib.mode_set_option(b"attn_bwd_mfma", mfma) == 0
                for _ in range(warm + n):
                    L.check(lib.mode_attn_block_bwd(*a, H.p(dy), H.p(dqkv), H.p(pq), H.p(pk), H.dt_of(qkv), B, T, Hh, hd, 1e-6, SEED, p, H.stream()), "attn_bwd")
                lib.mode_set_option(b"attn_bwd_mfma", 1)
            torch.cuda.synchronize()
    print(f"PERF done: {n} launches per kernel and shape after {warm} warm-up launches", flush=True)


def drive(out, only):
    lines = []
    for group in only or GROUPS:
        cmd = [sys.executable, os.path.abspath(__file__), "--child", group]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=CHILD_LIMIT)
        except subprocess.TimeoutExpired:
            print(f"{group}: no result within {CHILD_LIMIT} s - stopping", flush=True)
            return 1
        got = [ln.split() for ln in r.stdout.splitlines() if ln.startswith("DIGEST ")]
        if r.returncode != 0 or not got:
            print(f"{group}: exit status {r.returncode} - stopping\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}", flush=True)
            return 1
        lines += [f"{name} {digest}" for _, name, digest in got]
        print(f"{group}: {len(got)} digests", flush=True)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write("\n".join(lines) + "\n")
    else:
        print("\n".join(lines))
    return 0


def compare(paths):
    runs = [dict(ln.split() for ln in open(p) if ln.strip()) for p in paths]
    names = sorted(set().union(*runs))
    unstable = [k for k in names if len(runs) == 3 and runs[0].get(k) != runs[1].get(k)]
    bad = [k for k in names if k not in unstable and runs[0].get(k) != runs[-1].get(k)]
    for k in unstable:
        print(f"does not repeat between {paths[0]} and {paths[1]}, left out: {k}")
    print(f"{len(names) - len(unstable)} digests compared, {len(bad)} differ" + (":\n  " + "\n  ".join(bad) if bad else ""))
    return 1 if bad else 0


if __name__ == "__main__":
    args = sys.argv[1:]
    opt = lambda k, d=None: args[args.index(k) + 1] if k in args else d              # noqa: E731
    if args[:1] == ["--compare"]:
        sys.exit(compare(args[1:]))
    if "--child" in args:
        child(opt("--child"))
    elif "--perf" in args:
        perf(int(opt("--perf")))
    else:
        sys.exit(drive(opt("--out"), [g for g in (opt("--only") or "").split(",") if g]))
