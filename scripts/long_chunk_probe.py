"""Long action chunks at the benchmark model size (12 layers, d 1024, 8 heads, 4 experts top-2, bf16): ms per 10-step DDIM chunk (fused sampler,
device events, after warm-up) for action_seq_len in {10, 20, 32} x action_dim in {7, 14}, at B = 128 and B = 1.  Also the attention kernel alone
at each chunk length (B = 128, the chain's own launch), with the bytes it moves (qkv read + y write) and the achieved rate.

    python scripts/long_chunk_probe.py                      # the whole table
    python scripts/long_chunk_probe.py --only 128:20:7      # one (B, A_len, A_dim) point, e.g. under rocprofv3 --kernel-trace --stats

Never imported by the package or by bench.py."""
import argparse
import ctypes as C
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import mode_diffusion_policy_amd as M  # noqa: E402
from mode_diffusion_policy_amd import _lib as L  # noqa: E402
from oracle import mode_oracle as O  # noqa: E402
from oracle.weights import make_inputs, make_state_dict  # noqa: E402


def timed(fn, warmup, iters):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    st, en = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ts = []
    for _ in range(iters):
        st.record(); fn(); en.record(); en.synchronize()
        ts.append(st.elapsed_time(en))
    ts.sort()
    return ts[len(ts) // 2]


def chunk_ms(sd_cache, B, A_len, A_dim, warmup, iters):
    cfg = O.DiTConfig(action_seq_len=A_len, action_dim=A_dim)          # 12 L, d 1024, 8 heads, 4 experts top-2, obs 2048, goal 512
    key = (A_len, A_dim)
    if key not in sd_cache:
        sd_cache[key] = make_state_dict(cfg, 7)
    m = M.MoDeDiT(obs_dim=cfg.obs_dim, goal_dim=cfg.goal_dim, device="cuda", goal_conditioned=True, action_dim=A_dim, embed_dim=cfg.embed_dim,
                  embed_pdrob=0, attn_pdrop=0.3, n_layers=cfg.n_layers, n_heads=cfg.n_heads, goal_seq_len=1, obs_seq_len=1,
                  action_seq_len=A_len, num_experts=cfg.num_experts, top_k=cfg.top_k, compute_dtype="bf16")
    m.load_state_dict(sd_cache[key])
    m = m.cuda().eval()
    den = M.GCDenoiser(m, 0.5).eval()
    inp = {k: v.cuda() for k, v in make_inputs(cfg, B, 8).items()}
    state = {"state_images": inp["state_images"]}
    sig = M.get_sigmas_exponential(10, 1e-3, 80.0).cuda()
    with torch.no_grad():
        ms = timed(lambda: M.sample_ddim(den, state, inp["x0"], inp["goals"], sig, disable=True), warmup, iters)
    return ms, cfg.seq_len


def attn_us(B, T, H=8, hd=128, warmup=20, iters=200):
    lib = L.load()
    D = H * hd
    qkv = torch.randn(B * T, 3 * D, device="cuda").to(torch.bfloat16)
    g = torch.ones(hd, device="cuda")
    y = torch.empty(B * T, D, device="cuda", dtype=torch.bfloat16)
    s = torch.cuda.current_stream().cuda_stream

    def run():
        L.check(lib.mode_attn_block_fwd(qkv.data_ptr(), g.data_ptr(), g.data_ptr(), y.data_ptr(), L.MODE_BF16, B, T, H, hd, 1e-6, 0, 0.0, C.c_void_p(s)), "attn")
    us = timed(run, warmup, iters) * 1e3
    nbytes = (B * T * 3 * D + B * T * D) * 2
    return us, nbytes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", help="B:A_len:A_dim")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10)
    a = ap.parse_args()
    assert torch.cuda.is_available()
    sd_cache = {}
    if a.only:
        B, A_len, A_dim = (int(x) for x in a.only.split(":"))
        ms, T = chunk_ms(sd_cache, B, A_len, A_dim, a.warmup, a.iters)
        print(json.dumps(dict(B=B, A_len=A_len, A_dim=A_dim, T=T, chunk_ms=round(ms, 3))), flush=True)
        return
    for B in (128, 1):
        for A_len in (10, 20, 32):
            for A_dim in (7, 14):
                ms, T = chunk_ms(sd_cache, B, A_len, A_dim, a.warmup, a.iters)
                print(json.dumps(dict(B=B, A_len=A_len, A_dim=A_dim, T=T, chunk_ms=round(ms, 3))), flush=True)
    for A_len in (10, 20, 32):
        T = 4 + A_len
        us, nb = attn_us(128, T)
        print(json.dumps(dict(kernel="mode_attn_block_fwd", B=128, T=T, H=8, hd=128, us=round(us, 2), mbytes=round(nb / 1e6, 2),
                              gbps=round(nb / us / 1e3, 1))), flush=True)


if __name__ == "__main__":
    main()
