"""Bit-level digest of every host path that drives the denoiser chain: what the calls return, the experts they record and the usage counters
they keep, written to one .npz - made to be run on two commits and compared key by key (``numpy.array_equal``).  A host-side change that keeps
the launches and their arguments keeps every key.

Smallest test configuration (c1e4, seeded weights and inputs), B = 3 (odd, no bucket size: padding rows and the guided 2B halves), a 4-step
exponential schedule ending in sigma = 0 (Euler fallback / plain last step), for the three routing modes x guidance_scale in {None, 1.5} x
{bf16, fp32}.  Per configuration, with ``torch.manual_seed`` set right before each call: ``GCDenoiser.forward``; ``denoise_uniform`` twice on the
same observation tensors, then on new ones; the five deterministic fused samplers, graphed and with MODE_HIP_GRAPH=0; two replanning steps of a
``ChunkedRolloutPolicy`` (euler_ancestral); three steps of a ``VectorEnvPolicy`` (3 environments, multistep 2, one inactive at the second step).
After each call: the result, ``_last_topk``, every block's usage counters and token count, and the default generators' states.

    python scripts/sampler_paths_digest.py OUT.npz [--root TREE]     (TREE: another checkout to import the package and the oracle from)
    python scripts/sampler_paths_digest.py --compare A.npz B.npz     -> number of keys compared; exit status 1 on any difference"""
import dataclasses
import os
import sys

import numpy as np


def compare(a_path, b_path) -> int:
    a, b = np.load(a_path), np.load(b_path)
    bad = sorted(set(a.files) ^ set(b.files))
    bad += [k for k in a.files if k in b.files and not np.array_equal(a[k], b[k])]
    print(f"{len(set(a.files) | set(b.files))} keys compared, {len(bad)} differ")
    for k in bad[:40]:
        print("  differs:", k)
    return 1 if bad else 0


MODES = {"default": (310, {}), "goal": (311, dict(use_goal_in_routing=True)), "token": (312, dict(cond_router=False))}
B, STEPS = 3, 4


def main(out_path, root):
    sys.path.insert(0, root)
    import torch
    import mode_diffusion_policy_amd as M
    from mode_diffusion_policy_amd import gc_sampling as gs, rollout
    from oracle.weights import get_config, make_inputs, make_state_dict

    print("package:", os.path.dirname(M.__file__))
    dev = torch.device("cuda:0")
    rec = {}

    def record(tag, m, result):
        """The observable state after one call."""
        rec[tag + "/result"] = result.detach().float().cpu().numpy()
        topk = getattr(m, "_last_topk", None)
        if topk is not None:
            rec[tag + "/topk"] = topk.cpu().numpy()
        m.sync_expert_usage()
        rec[tag + "/usage"] = torch.stack([blk.inference_expert_usage for blk in m.blocks]).numpy().copy()
        rec[tag + "/tokens"] = np.asarray([blk.total_tokens_processed for blk in m.blocks], dtype=np.int64)
        rec[tag + "/rng_host"] = torch.get_rng_state().numpy()
        rec[tag + "/rng_dev"] = torch.cuda.get_rng_state(dev).numpy()

    def call(tag, m, fn):
        torch.manual_seed(1234)
        record(tag, m, fn())

    for mode, (seed, over) in MODES.items():
        for dtype in ("bf16", "fp32"):
            for w in (None, 1.5):
                cfg = dataclasses.replace(get_config("c1e4"), **over)
                m = M.MoDeDiT(obs_dim=cfg.obs_dim, goal_dim=cfg.goal_dim, device="cuda", goal_conditioned=True, action_dim=cfg.action_dim,
                              embed_dim=cfg.embed_dim, embed_pdrob=0, attn_pdrop=0.3, n_layers=cfg.n_layers, n_heads=cfg.n_heads, goal_seq_len=1,
                              obs_seq_len=1, action_seq_len=cfg.action_seq_len, num_experts=cfg.num_experts, top_k=cfg.top_k, compute_dtype=dtype,
                              **over)
                m.load_state_dict(make_state_dict(cfg, seed))
                m = m.to(dev).eval()
                den = M.GCDenoiser(m, 0.5, guidance_scale=w).eval()
                inp = {k: v.to(dev) for k, v in make_inputs(cfg, B, seed + 100).items()}
                state, goals, x0 = {"state_images": inp["state_images"]}, inp["goals"], inp["x0"]
                sig = M.get_sigmas_exponential(STEPS, 1e-3, 80.0).to(dev)
                pre = f"{mode}/{dtype}/w{w}"
                with torch.no_grad():
                    call(pre + "/forward", m, lambda: den(state, inp["actions"], goals, sig[:B].clone()))
                    for i in range(2):
                        call(pre + f"/denoise_uniform{i}", m, lambda: den.denoise_uniform(state, x0, goals, sig[1]))
                    state2, goals2 = {"state_images": inp["state_images"].flip(0).contiguous()}, goals.flip(0).contiguous()
                    call(pre + "/denoise_uniform_new_obs", m, lambda: den.denoise_uniform(state2, x0, goals2, sig[2]))
                    samplers = dict(ddim=gs.sample_ddim, dpmpp_2m=gs.sample_dpmpp_2m, heun=gs.sample_heun, dpm_2=gs.sample_dpm_2, dpmpp_2s=gs.sample_dpmpp_2s)
                    for graph in ("1", "0"):
                        os.environ["MODE_HIP_GRAPH"] = graph
                        for name, fn in samplers.items():
                            call(pre + f"/graph{graph}/{name}", m, lambda: fn(den, state, x0, goals, sig, disable=True))
                    os.environ.pop("MODE_HIP_GRAPH")
                    pol = rollout.ChunkedRolloutPolicy(den, num_sampling_steps=STEPS, sigma_min=1e-3, sigma_max=80.0, sampler_type="euler_ancestral",
                                                       act_window_size=cfg.action_seq_len, multistep=1, action_dim=cfg.action_dim)
                    for i in range(2):
                        call(pre + f"/chunked_step{i}", m, lambda: pol.step(state, goals))
                    vec = rollout.VectorEnvPolicy(den, 3, num_sampling_steps=STEPS, sigma_min=1e-3, sigma_max=80.0, multistep=2,
                                                  act_window_size=cfg.action_seq_len, action_dim=cfg.action_dim)
                    for i, active in enumerate((None, np.array([True, False, True]), None)):
                        call(pre + f"/vector_step{i}", m, lambda: vec.step(state, goals, active=active))
                        rec[pre + f"/vector_step{i}/plans"] = vec.plans.cpu().numpy()
                        rec[pre + f"/vector_step{i}/draws"] = vec.draws.cpu().numpy()
                print(pre, "done", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    np.savez(out_path, **rec)
    print(f"{len(rec)} keys -> {out_path}")


if __name__ == "__main__":
    args = sys.argv[1:]
    if args[:1] == ["--compare"]:
        sys.exit(compare(args[1], args[2]))
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    main(args[0], os.path.abspath(args[args.index("--root") + 1]) if "--root" in args else here)
