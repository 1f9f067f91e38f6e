"""Causal attention for 16 < T <= 64 tokens per sample (attn_long.hip, taken by mode_attn_block_fwd / mode_attn_block_bwd when T > 16) against
torch: forward in bf16 and fp32, the causality property, the hash dropout mask (oracle.mode_oracle.attn_keep_scale), the backward (dqkv and the
qk-norm gain partials) against autograd with and without dropout, and a ragged batch."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

import hip_helpers as H  # noqa: E402
from mode_diffusion_policy_amd import _lib as L  # noqa: E402
from oracle import mode_oracle as O  # noqa: E402

DT = {torch.bfloat16: L.MODE_BF16, torch.float32: L.MODE_F32}


def dev():
    return torch.device("cuda")


def rel(a, b):
    a = torch.as_tensor(a).double().cpu(); b = torch.as_tensor(b).double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def rnd(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def _ref(qkv, qg, kg, B, T, Hh, hd, keep=None):
    D = Hh * hd
    q, k, v = (t.view(B, T, Hh, hd).transpose(1, 2) for t in qkv.split(D, dim=-1))
    q = O.rmsnorm(q, qg); k = O.rmsnorm(k, kg)
    att = (q @ k.transpose(-2, -1)) / math.sqrt(hd)
    att = att.masked_fill(~torch.ones(T, T, dtype=torch.bool).tril(), float("-inf")).softmax(-1)
    if keep is not None:
        att = att * keep
    return (att @ v).transpose(1, 2).reshape(B * T, D)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("hd", [32, 64, 128])
@pytest.mark.parametrize("T", [17, 24, 33, 48, 64])
def test_attention_long(T, hd, dtype):
    B, Hh = 5, 3
    D = Hh * hd
    qkv = rnd(B * T, 3 * D, seed=41 + T).to(dtype)
    qg = 1 + 0.1 * rnd(hd, seed=42); kg = 1 + 0.1 * rnd(hd, seed=43)
    y = H.attn(qkv.to(dev()), qg.to(dev()), kg.to(dev()), B, T, Hh, hd)
    ref = _ref(qkv.float(), qg, kg, B, T, Hh, hd)
    assert not torch.isnan(y.float()).any()
    assert rel(y.float(), ref) < (1.2e-2 if dtype == torch.bfloat16 else 1e-5)
    # causality: token 0 attends only to itself -> its output is its own v
    y0 = y.float().cpu().view(B, T, D)[:, 0]
    v0 = qkv.float().view(B, T, 3 * D)[:, 0, 2 * D:]
    assert rel(y0, v0) < (8e-3 if dtype == torch.bfloat16 else 1e-6)
    # a later token does not see the future: changing the last token leaves every earlier output unchanged
    qkv2 = qkv.clone().view(B, T, 3 * D)
    qkv2[:, -1] = rnd(B, 3 * D, seed=7).to(dtype)
    y2 = H.attn(qkv2.view(B * T, 3 * D).to(dev()), qg.to(dev()), kg.to(dev()), B, T, Hh, hd)
    assert torch.equal(y2.view(B, T, D)[:, :-1], y.view(B, T, D)[:, :-1])


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("B,T,Hh,hd", [(37, 24, 4, 64), (3, 64, 2, 128), (6, 40, 8, 32)])
def test_attention_long_dropout_and_ragged_batch(dtype, B, T, Hh, hd):
    D = Hh * hd
    p, seed = 0.3, 1234
    qkv = rnd(B * T, 3 * D, seed=51).to(dtype)
    qg = 1 + 0.1 * rnd(hd, seed=52); kg = 1 + 0.1 * rnd(hd, seed=53)
    y = H.attn(qkv.to(dev()), qg.to(dev()), kg.to(dev()), B, T, Hh, hd, seed=seed, p_drop=p)
    keep = O.attn_keep_scale(seed, B, Hh, T, p)
    ref = _ref(qkv.float(), qg, kg, B, T, Hh, hd, keep)
    assert rel(y.float(), ref) < (1.2e-2 if dtype == torch.bfloat16 else 1e-5)
    # a sample's result does not depend on the batch around it (ragged B: last workgroups of the grid)
    y1 = H.attn(qkv.view(B, T, 3 * D)[:1].reshape(T, 3 * D).to(dev()), qg.to(dev()), kg.to(dev()), 1, T, Hh, hd)
    y_all = H.attn(qkv.to(dev()), qg.to(dev()), kg.to(dev()), B, T, Hh, hd)
    assert torch.equal(y1, y_all[:T])


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("B,T,Hh,hd,p", [(3, 24, 4, 32, 0.0), (4, 64, 8, 128, 0.0), (5, 33, 2, 64, 0.3), (37, 20, 2, 64, 0.0), (2, 48, 2, 128, 0.3)])
def test_attention_long_backward(dtype, B, T, Hh, hd, p):
    lib = L.load()
    D = Hh * hd
    qkv = rnd(B * T, 3 * D, seed=21).to(dtype)
    qg = 1 + 0.1 * rnd(hd, seed=22); kg = 1 + 0.1 * rnd(hd, seed=23)
    dy = rnd(B * T, D, seed=24).to(dtype)
    seed = 777
    keep = O.attn_keep_scale(seed, B, Hh, T, p) if p > 0 else None
    qd, qgd, kgd, dyd = qkv.to(dev()), qg.to(dev()), kg.to(dev()), dy.to(dev())
    dqkv = torch.full((B * T, 3 * D), float("nan"), dtype=dtype, device=dev())
    pq = torch.empty(B * Hh, hd, device=dev()); pk = torch.empty(B * Hh, hd, device=dev())
    L.check(lib.mode_attn_block_bwd(qd.data_ptr(), qgd.data_ptr(), kgd.data_ptr(), dyd.data_ptr(), dqkv.data_ptr(), pq.data_ptr(), pk.data_ptr(),
                                    DT[dtype], B, T, Hh, hd, 1e-6, seed, p, H.stream()))
    x = qkv.float().requires_grad_(True); a = qg.clone().requires_grad_(True); c = kg.clone().requires_grad_(True)
    y = _ref(x, a, c, B, T, Hh, hd, keep)
    y.backward(dy.float())
    tol = 2e-2 if dtype == torch.bfloat16 else 2e-5
    assert not torch.isnan(dqkv.float()).any()
    assert rel(dqkv.float(), x.grad) < tol
    assert rel(pq.sum(0), a.grad) < tol and rel(pk.sum(0), c.grad) < tol
    # "attn_bwd_mfma" keeps its meaning for T <= 16 only: the long-T kernel gives the same bits either way
    dq2 = torch.full_like(dqkv, float("nan"))
    lib.mode_set_option(b"attn_bwd_mfma", 0)
    try:
        L.check(lib.mode_attn_block_bwd(qd.data_ptr(), qgd.data_ptr(), kgd.data_ptr(), dyd.data_ptr(), dq2.data_ptr(), pq.data_ptr(), pk.data_ptr(),
                                        DT[dtype], B, T, Hh, hd, 1e-6, seed, p, H.stream()))
    finally:
        lib.mode_set_option(b"attn_bwd_mfma", 1)
    assert torch.equal(dq2, dqkv)


def test_attention_beyond_64_tokens_is_refused():
    lib = L.load()
    B, T, Hh, hd = 2, 65, 2, 64
    D = Hh * hd
    qkv = torch.zeros(B * T, 3 * D, dtype=torch.bfloat16, device=dev())
    g = torch.ones(hd, device=dev())
    y = torch.empty(B * T, D, dtype=torch.bfloat16, device=dev())
    assert lib.mode_attn_block_fwd(qkv.data_ptr(), g.data_ptr(), g.data_ptr(), y.data_ptr(), L.MODE_BF16, B, T, Hh, hd, 1e-6, 0, 0.0, H.stream()) != 0
