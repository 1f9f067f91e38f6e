"""Cost of a 10-step DDIM chunk per routing mode on the benchmarked model (C2 geometry, bf16): the default conditioning-row routing on sigma,
goal routing (use_goal_in_routing=True: router input emb_t + goal_emb(goal)) and token routing (cond_router=False), each as the captured chunk
(one hipGraph replay) and on the per-step path (MODE_HIP_GRAPH=0).  Prints ms per chunk at B = 1, 32, 128 and the kernel launches of one
chunk: for the captured chunk the kernels the graph holds (its launch chain issued eagerly once under the profiler) plus what runs around
the replay; for the per-step path every kernel of the call.

    python scripts/routing_variants_probe.py [B ...]   -> profiles/routing_variants.txt"""
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
import mode_diffusion_policy_amd as M  # noqa: E402

MODES = {"default": {}, "goal": dict(use_goal_in_routing=True), "token": dict(cond_router=False)}


def build(dev, over):
    torch.manual_seed(0)
    C2 = bench.C2
    m = M.MoDeDiT(obs_dim=C2["obs_dim"], goal_dim=C2["goal_dim"], device=str(dev), goal_conditioned=True, action_dim=7, embed_dim=C2["embed_dim"],
                  embed_pdrob=0, attn_pdrop=0.3, n_layers=C2["n_layers"], n_heads=C2["n_heads"], goal_seq_len=1, obs_seq_len=1, action_seq_len=10,
                  mlp_pdrop=0.1, goal_drop=0.1, num_experts=C2["num_experts"], top_k=C2["top_k"], compute_dtype="bf16", **over)
    return M.GCDenoiser(m.to(dev).eval(), bench.SIGMA_DATA).eval()


def kernels(fn):
    """Device kernels issued by fn() (torch profiler, eager launches only)."""
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    try:
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
    except RuntimeError:                                             # no device tracer in this build: report -1
        return -1
    return sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA)


def captured_chain(den, img, goal, x0, sig):
    """The launch chain the ddim graph holds, issued eagerly on the graph's own state (same launches as the capture)."""
    m = den.inner_model
    ent = m._route_cache["graph"]
    eng = m.engine
    bufs = [ent["bufs"][0].clone()] + ent["bufs"][1:]                # (plain DDIM never touches buffers 1 and 2)
    with eng.pinned_workspace(ent["ws"]):
        m._chunk_steps(eng, ent["img"], ent["goals"], bufs, ent["sched"], ent["evals"], tok=ent["tok"])


def main():
    dev = torch.device("cuda:0")
    sig = M.get_sigmas_exponential(10, 1e-3, 80.0).to(dev)
    batches = [int(a) for a in sys.argv[1:]] or [1, 32, 128]
    print(f"10-step DDIM chunk, C2 geometry (D {bench.C2['embed_dim']}, {bench.C2['n_layers']} layers, {bench.C2['num_experts']} experts, top-{bench.C2['top_k']}), bf16; "
          f"ms per chunk = mean of 20 calls after 3 warm-up calls")
    print(f"{'mode':8s} {'B':>4s} {'graphed ms':>11s} {'per-step ms':>12s} {'gain':>6s}   {'graph kernels':>13s} {'+ around replay':>15s} {'per-step kernels':>16s}")
    for mode, over in MODES.items():
        den = build(dev, over)
        for B in batches:
            img, goal, x0 = bench.synthetic_inputs(dev, B)
            fn = lambda: M.sample_ddim(den, {"state_images": img}, x0, goal, sig, disable=True)
            res = {}
            for path in ("1", "0"):
                os.environ["MODE_HIP_GRAPH"] = path
                for _ in range(3):
                    fn()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(20):
                    fn()
                torch.cuda.synchronize()
                res[path] = (time.perf_counter() - t0) / 20 * 1e3
                if path == "1":
                    res["around"] = kernels(fn)                      # the replay itself is not an eager kernel: copies, counters, the output clone
                    res["graph"] = kernels(lambda: captured_chain(den, img, goal, x0, sig))
                else:
                    res["step"] = kernels(fn)
            os.environ.pop("MODE_HIP_GRAPH", None)
            print(f"{mode:8s} {B:4d} {res['1']:11.3f} {res['0']:12.3f} {res['0'] / res['1']:5.2f}x   {res['graph']:13d} {res['around']:15d} {res['step']:16d}",
                  flush=True)
        del den
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
