#!/usr/bin/env python3
"""What does it cost a layer kernel that its weights come from HBM instead of the Infinity Cache?  (LABNOTES.md, "weight run-ahead".)

The five kernels of one transformer block at the benchmark shape (B = 128: 1792 tokens, 3584 sorted rows, D = 1024, 4 experts top-2, one routing row),
each timed the way bench.layer_kernel_breakdown does - a hipGraph of back-to-back launches between two events - in three arms of ONE process:

  cold   the weight matrix cycles over enough copies that their ACTIVE bytes exceed the 256-MiB Infinity Cache several times over between two uses
         (Wqkv 6.3 MB x 48, Wo 2.1 MB x 144, W1 / W2 33.6 / 16.8 MB active x 12 / 24 - about 300 - 400 MB each), as in the chain, where one denoise step
         touches 767 MB of weights;
  mall   the copies of the cycle add up to 75 - 100 MB: more than the eight XCDs' L2s hold together (32 MiB), well inside the Infinity Cache - what a
         consumer sees when a run-ahead has pulled its matrix in from HBM;
  warm   one copy, reused by every launch (small matrices then also sit in L2: an upper bound no prefetch into the Infinity Cache reaches).

Activations, outputs and everything else are the same buffers in every arm.  Arms alternate, three rounds; a round's figure is the median of three
replays.  A kernel whose cold - mall gap is below the spread (max - min over rounds) of either arm has nothing a prefetch could win.  The combine
kernel reads no weight matrix (two gain vectors): its arms are the same launch and show what the method resolves.

    python scripts/weight_residency_probe.py [--out FILE] [--reps 144] [--rounds 3]
Nothing imports this file."""
import argparse
import ctypes as C
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=144)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    import bench
    from mode_diffusion_policy_amd import _lib as L
    from mode_diffusion_policy_amd.engine import capture_graph
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    _, den = bench.build_model(dev, "bf16")
    eng = den.inner_model.engine
    lib = L.load()
    D, E, k, T, H, B = 1024, 4, 2, 14, 8, 128
    N, NK, S = B * T, B * T * 2, 4
    bf = torch.bfloat16
    idx = torch.tensor([[1, 2]], dtype=torch.int32, device=dev); w = torch.tensor([[0.6, 0.4]], dtype=torch.float32, device=dev)
    meta = eng.dispatch(idx, w, 1, 1, N, N); ml = eng.meta_layout(N); mp = meta.data_ptr()
    g = torch.Generator(device="cpu").manual_seed(0)

    def rnd(*shape, scale=1.0, dtype=torch.float32):
        return (torch.randn(*shape, generator=g) * scale).to(dtype).to(dev)

    h = rnd(N, D, dtype=bf); yat = rnd(N, D, dtype=bf); x = rnd(N, D); xo = torch.empty(N, D, device=dev); h2 = torch.empty(N, D, dtype=bf, device=dev)
    ss = torch.rand(N, D // 64, generator=g).to(dev) + 0.5
    Hb = rnd(NK, 4 * D, scale=0.1, dtype=bf); Hout = torch.empty(NK, 4 * D, dtype=bf, device=dev)
    Y = torch.empty(S, NK, D, dtype=bf, device=dev)
    cond = rnd(1, D); gain = (1 + 0.1 * torch.randn(2, D, generator=g)).to(dev); qg = torch.ones(D // H, device=dev); kg = torch.ones(D // H, device=dev)
    bqkv = rnd(3 * D, scale=0.1); b1 = rnd(E, 8 * D, scale=0.1)

    def copies(n, *shape):
        """n copies of one random bf16 matrix: [n, *shape]"""
        base = rnd(*shape, scale=shape[-1] ** -0.5, dtype=bf)
        return base.unsqueeze(0).repeat(n, *([1] * len(shape))).contiguous()
    wqkv = copies(48, 3 * D, D); wo = copies(144, D, D); w1 = copies(12, E, 8 * D, D); w2 = copies(24, E, D, 4 * D)

    def gd(**kw):
        base = dict(dtype=L.MODE_BF16, epilogue=L.EPI_NONE, out_dtype=L.MODE_BF16, M=N, N=D, K=D, A=h.data_ptr(), lda=D, W=None, ldw=D, C=None, ldc=D)
        base.update(kw)
        return L.ModeGemmDesc(**base)
    cpr = [gd(epilogue=L.EPI_RESIDUAL_NORM, out_dtype=L.MODE_F32, A=yat.data_ptr(), W=wo[i].data_ptr(), resid=x.data_ptr(), ldr=D, C=xo.data_ptr(), C2=h2.data_ptr(),
              ldc2=D, gain=gain[0].data_ptr(), row_ss_out=ss.data_ptr()) for i in range(wo.shape[0])]
    up = [gd(epilogue=L.EPI_SWIGLU, M=NK, N=4 * D, W=w1[i].data_ptr(), w_expert_stride=8 * D * D, bias=b1.data_ptr(), bias_expert_stride=8 * D, C=Hout.data_ptr(),
             ldc=4 * D, a_rows=mp + 4 * ml.perm, expert_offsets=mp + 4 * ml.offsets, num_experts=E, row_ss=ss.data_ptr(), row_ss_n=D // 64, row_eps=1e-6,
             flags=L.GEMM_UNIFORM_GROUPS | L.GEMM_IDENTITY_ROWS) for i in range(w1.shape[0])]
    dn = [gd(M=NK, N=D, K=4 * D, A=Hb.data_ptr(), lda=4 * D, W=w2[i].data_ptr(), ldw=4 * D, w_expert_stride=4 * D * D, C=Y.data_ptr(), expert_offsets=mp + 4 * ml.offsets,
             num_experts=E, split_k=S, split_stride=NK * D, flags=L.GEMM_UNIFORM_GROUPS) for i in range(w2.shape[0])]
    qa = [L.ModeQkvAttnDesc(dtype=L.MODE_BF16, B=B, T=T, H=H, D=D, h=h.data_ptr(), ldh=D, wqkv=wqkv[i].data_ptr(), ldw=D, bqkv=bqkv.data_ptr(), q_gain=qg.data_ptr(),
                            k_gain=kg.data_ptr(), eps=1e-6, y=yat.data_ptr(), ldy=D) for i in range(wqkv.shape[0])]

    def gemm(ds):
        return len(ds), lambda i, st: L.check(lib.mode_gemm(C.byref(ds[i]), st))

    def comb(i, st):
        L.check(lib.mode_moe_combine_norm_fused_fwd(xo.data_ptr(), ss.data_ptr(), D // 64, gain[0].data_ptr(), Y.data_ptr(), L.MODE_BF16, S, NK * D, mp + 4 * ml.pos,
                                                    mp + 4 * ml.posw, N, D, k, gain[1].data_ptr(), cond.data_ptr(), N, 1e-6, x.data_ptr(), h.data_ptr(), L.MODE_BF16, st))
    items = [("qkv+attention", (len(qa), lambda i, st: L.check(lib.mode_qkv_attn_fwd(C.byref(qa[i]), st))), 12, "Wqkv 6.3 MB x 48 / x 12"),
             ("c_proj+resid+ln2", gemm(cpr), 36, "Wo 2.1 MB x 144 / x 36"),
             ("up+swiglu", gemm(up), 3, "W1 33.6 MB active x 12 / x 3"),
             ("down_4slabs", gemm(dn), 6, "W2 16.8 MB active x 24 / x 6"),
             ("combine+ln1", (1, comb), 1, "no weight matrix: all arms are the same launch")]
    cur = lambda: torch.cuda.current_stream().cuda_stream
    lines = [f"weight residency probe: {torch.cuda.get_device_name(dev)}, {args.reps} launches per graph, {args.rounds} alternating rounds, us per launch (median of 3 replays)",
             f"{'kernel':<18} {'arm':<5} " + " ".join(f"round{r + 1:>2}" for r in range(args.rounds)) + "   median  spread   | cold - mall   verdict"]
    ARMS = ("cold", "mall", "warm")
    for name, (ncopies, fn), nmall, what in items:
        graphs = {}
        for arm in ARMS:
            pick = {"cold": lambda i: i % ncopies, "mall": lambda i: i % nmall, "warm": lambda i: 0}[arm]
            for i in range(min(ncopies, 16)):
                fn(pick(i), cur())
            torch.cuda.synchronize()
            gr = torch.cuda.CUDAGraph()
            with capture_graph(gr):
                st = cur()
                for i in range(args.reps):
                    fn(pick(i), st)
            gr.replay(); torch.cuda.synchronize()
            graphs[arm] = gr
        res = {a: [] for a in ARMS}
        for _ in range(args.rounds):
            for arm in ARMS:
                gr = graphs[arm]
                gr.replay(); torch.cuda.synchronize()                       # the arm's own cache state before it is timed
                ts = []
                for _ in range(3):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(); gr.replay(); e1.record(); torch.cuda.synchronize()
                    ts.append(e0.elapsed_time(e1) * 1e3 / args.reps)
                res[arm].append(statistics.median(ts))
        med = {a: statistics.median(v) for a, v in res.items()}
        spread = {a: max(v) - min(v) for a, v in res.items()}
        gap = med["cold"] - med["mall"]
        verdict = "kept in the plan" if gap > max(spread["cold"], spread["mall"]) else "DROPPED: gap below the spread of its own rounds"
        if ncopies == 1:
            verdict = "(noise floor)"
        for arm in ARMS:
            tail = f"   | {gap:+7.2f} us    {verdict}   [{what}]" if arm == "cold" else ""
            lines.append(f"{name:<18} {arm:<5} " + " ".join(f"{v:7.2f}" for v in res[arm]) + f"  {med[arm]:7.2f} {spread[arm]:7.2f}{tail}")
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
