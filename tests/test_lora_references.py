"""CPU: the fp64 references of tests/lora_refs.py are the chain rule of y = x (W + s B A)^T (torch autograd, fp64), an fp32 emulation of the
kernels' stated arithmetic sits inside the derived bounds, and every deliberately wrong reference sits outside them on the shapes the GPU tests use."""
import ctypes as C
import os
import re

import pytest
import torch

import lora_refs as R
from mode_diffusion_policy_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [(G, rows, cols, r) for (rows, cols) in R.GRAD_SHAPES for r in R.RANKS for G in R.GROUPS]


@pytest.mark.parametrize("G,rows,cols,r", [(1, 7, 64, 3), (3, 65, 192, 16), (1, 129, 64, 64)])
def test_projection_is_the_chain_rule_of_the_merged_weight(G, rows, cols, r):
    """dA and dB from autograd through y = x (W + s B A)^T equal s B^T dW and s dW A^T, with dW the gradient of the merged weight."""
    d = R.inputs(G, rows, cols, r)
    g = torch.Generator().manual_seed(5)
    W, A, B = (R.f64(d[k]) for k in ("W", "A", "B"))
    A.requires_grad_(True); B.requires_grad_(True)
    x = torch.randn(G, 11, cols, generator=g, dtype=torch.float64)
    up = torch.randn(G, 11, rows, generator=g, dtype=torch.float64)
    Weff = W + R.SCALE * (B @ A)
    Weff.retain_grad()
    ((x @ Weff.transpose(1, 2)) * up).sum().backward()
    (dA, dB), _ = R.grad_ref(Weff.grad, A, B, R.SCALE)
    assert torch.allclose(A.grad, dA, rtol=1e-12, atol=1e-12) and torch.allclose(B.grad, dB, rtol=1e-12, atol=1e-12)
    ref, _ = R.merge_ref(W, A, B, R.SCALE)
    assert torch.allclose(ref, Weff.detach(), rtol=1e-14, atol=1e-14)
    # accumulate: the previous value is one more term
    (dA2, dB2), _ = R.grad_ref(Weff.grad, A, B, R.SCALE, d["dA0"], d["dB0"])
    assert torch.allclose(dA2, dA + d["dA0"].double()) and torch.allclose(dB2, dB + d["dB0"].double())


@pytest.mark.parametrize("G,rows,cols,r", [(1, 1, 64, 1), (3, 65, 192, 3), (1, 129, 64, 16), (3, 7, 64, 64)])
def test_fp32_emulation_of_the_stated_arithmetic_is_inside_the_bounds(G, rows, cols, r):
    """The kernels' arithmetic restated with torch fp32 ops (sequential accumulation in the stated order; the products rounded separately, which is
    no better than an fma) stays inside the derived bounds - the bounds are not tighter than the format allows."""
    d = R.inputs(G, rows, cols, r)
    W, A, B, dW = d["W"], d["A"], d["B"], d["dW"]
    s = torch.tensor(R.SCALE, dtype=torch.float32)
    acc = torch.zeros_like(W)
    for k in range(r):
        acc = acc + B[:, :, k:k + 1] * A[:, k:k + 1, :]
    ref, S = R.merge_ref(W, A, B, float(s))
    got = W + s * acc
    assert R.worst(got, ref, R.merge_bound(ref, S, False)) <= 1.0
    assert R.worst(got.bfloat16().float(), ref, R.merge_bound(ref, S, True)) <= 1.0
    (dA, dB), (bA, bB) = R.grad_ref(dW, A, B, float(s))
    parts = []
    for r0 in range(0, rows, R.ROW_BLOCK):
        p = torch.zeros(G, r, cols)
        for i in range(r0, min(rows, r0 + R.ROW_BLOCK)):
            p = p + B[:, i, :, None] * dW[:, i, None, :]
        parts.append(p)
    tot = parts[0]
    for p in parts[1:]:
        tot = tot + p
    accB = torch.zeros(G, rows, r)
    for j in range(cols):
        accB = accB + dW[:, :, j, None] * A[:, None, :, j]
    assert R.worst(s * tot, dA, bA) <= 1.0 and R.worst(s * accB, dB, bB) <= 1.0


@pytest.mark.parametrize("G,rows,cols,r", CASES)
def test_wrong_references_are_outside_the_bounds(G, rows, cols, r):
    d = R.inputs(G, rows, cols, r)
    (dA, dB), (bA, bB) = R.grad_ref(d["dW"], d["A"], d["B"], R.SCALE)
    wrong = R.wrong_grads(d["dW"], d["A"], d["B"], R.SCALE)
    assert {"scale dropped", "last row block dropped"} <= set(wrong) and ("experts swapped" in wrong) == (G > 1) and ("dW transposed" in wrong) == (rows > 1)
    for name, (wA, wB) in wrong.items():
        assert R.worst(wA, dA, bA) > 10 and R.worst(wB, dB, bB) > 10, (name, R.worst(wA, dA, bA), R.worst(wB, dB, bB))
    if (rows, cols) in R.MERGE_SHAPES:
        ref, S = R.merge_ref(d["W"], d["A"], d["B"], R.SCALE)
        wm = R.wrong_merges(d["W"], d["A"], d["B"], R.SCALE)
        assert ("experts swapped" in wm) == (G > 1)
        for name, w in wm.items():
            for bf16 in (True, False):
                assert R.worst(w, ref, R.merge_bound(ref, S, bf16)) > 10, (name, bf16)


def test_entry_points_refuse_bad_shapes_without_a_device():
    """Rank 0 / 65 and cols % 8 != 0 are refused on the host before any pointer is looked at (the GPU test repeats this over canaried outputs);
    the workspace query is 0 for them and G * ceil(rows / 64) * r * cols floats otherwise."""
    lib = L.load()
    hdr = open(os.path.join(ROOT, "include", "mode_hip.h")).read()
    assert int(re.search(r"#define\s+MODE_LORA_MAX_RANK\s+(\d+)", hdr).group(1)) == L.MODE_LORA_MAX_RANK == max(R.RANKS)
    for r, cols in ((0, 64), (65, 64), (16, 68), (16, 4)):
        d = L.ModeLoraDesc(G=1, rows=8, cols=cols, r=r, w_stride=8 * cols)
        assert lib.mode_lora_merge(C.byref(d), None) == -2 and lib.mode_lora_grad(C.byref(d), None, 0, None) == -2
        assert lib.mode_lora_grad_workspace_bytes(C.byref(d)) == 0
    d = L.ModeLoraDesc(G=3, rows=129, cols=64, r=16, w_stride=129 * 64 + 64)
    assert lib.mode_lora_grad_workspace_bytes(C.byref(d)) == 3 * 3 * 16 * 64 * 4
    assert lib.mode_lora_merge(C.byref(d), None) == -1 and lib.mode_lora_grad(C.byref(d), None, 0, None) == -1       # null pointers
    d.w_stride = 129 * 64 + 4
    assert lib.mode_lora_merge(C.byref(d), None) == -1                                                                 # stride not a multiple of 8
    assert lib.mode_lora_merge(None, None) == -1


def test_adapter_module_surface_on_the_host():
    """LoraAdapter on a CPU model: shapes, initialisation, scale, state_dict round trip and its refusals; the model's parameter and state_dict
    layout are untouched by attach() (the adapter is no submodule)."""
    import mode_diffusion_policy_amd as M
    kw = dict(obs_dim=32, goal_dim=16, device="cpu", goal_conditioned=True, action_dim=7, embed_dim=64, embed_pdrob=0, attn_pdrop=0.0, n_layers=2,
              n_heads=4, goal_seq_len=1, obs_seq_len=1, action_seq_len=10, num_experts=4, top_k=2)
    m = M.MoDeDiT(**kw)
    names, keys = [n for n, _ in m.named_parameters()], list(m.state_dict())
    m.freeze_router()
    flags = [p.requires_grad for p in m.parameters()]
    ad = M.LoraAdapter(m, rank=4, alpha=6.0, seed=3)
    assert ad.scale == 1.5 and ad.targets == ("wqkv", "wo", "w1", "w2")
    assert tuple(ad.A_w1.shape) == (2, 4, 4, 64) and tuple(ad.B_w1.shape) == (2, 4, 512, 4) and tuple(ad.B_wqkv.shape) == (2, 1, 192, 4)
    assert tuple(ad.A_w2.shape) == (2, 4, 4, 256) and tuple(ad.B_w2.shape) == (2, 4, 64, 4)
    assert all(float(b.detach().abs().max()) == 0 for _, _, b in ad.pairs()) and abs(float(ad.A_w1.detach().std()) - 0.5) < 0.05
    assert torch.equal(M.LoraAdapter(m, rank=4, seed=3).A_wo, ad.A_wo) and not torch.equal(M.LoraAdapter(m, rank=4, seed=4).A_wo, ad.A_wo)
    ad.attach()
    assert m._lora is ad and not any(p.requires_grad for p in m.parameters()) and all(p.requires_grad for p in ad.parameters())
    assert [n for n, _ in m.named_parameters()] == names and list(m.state_dict()) == keys and not any("lora" in n.lower() for n, _ in m.named_modules())
    other = M.LoraAdapter(m, rank=4, targets=("w1",)).attach()                   # replaces the first; the remembered flags pass on
    assert m._lora is other and other.targets == ("w1",)
    other.detach()
    assert getattr(m, "_lora", None) is None and [p.requires_grad for p in m.parameters()] == flags
    sd = ad.state_dict()
    assert sd["_extra_state"] == dict(rank=4, alpha=6.0, targets=["wqkv", "wo", "w1", "w2"], embed_dim=64, num_layers=2, num_experts=4)
    twin = M.LoraAdapter(m, rank=4, seed=9)
    twin.load_state_dict(sd)
    assert twin.alpha == 6.0 and all(torch.equal(a, b) for a, b in zip(twin.parameters(), ad.parameters()))
    before = [p.clone() for p in twin.parameters()]
    for bad in (M.LoraAdapter(m, rank=8), M.LoraAdapter(m, rank=4, targets=("wo", "w2")), M.LoraAdapter(M.MoDeDiT(**dict(kw, n_layers=1)), rank=4)):
        with pytest.raises(ValueError, match="another adapter or model"):
            bad.load_state_dict(sd)
    with pytest.raises(ValueError, match="not a LoraAdapter"):
        twin.load_state_dict({k: v for k, v in sd.items() if k != "_extra_state"})
    assert all(torch.equal(a, b) for a, b in zip(twin.parameters(), before))
    for kwargs in (dict(rank=0), dict(rank=65), dict(targets=("wq",)), dict(targets=())):
        with pytest.raises(ValueError):
            M.LoraAdapter(m, **kwargs)
    with pytest.raises(ValueError, match="bf16"):
        M.LoraAdapter(M.MoDeDiT(**dict(kw, compute_dtype="fp32")), rank=4).attach()
