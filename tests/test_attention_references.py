"""The fp64 restatements of tests/attn_refs.py, validated without a GPU: against the oracle's causal_attention, against torch's
scaled_dot_product_attention, the backward against central differences, each wrong reference against the bound the GPU test applies, and the
reference-alone gaps (fp32 torch and the bf16 rounding-point model against fp64) of every case of tests/test_gpu_attention_edges.py's matrix.  A
mismatch between a HIP kernel and attn_refs on the GPU is then the kernel's, not the reference's."""
import math

import pytest
import torch
import torch.nn.functional as F

from oracle import mode_oracle as O

import attn_refs as R
from attn_refs import BF16, F32


def rel(a, b):
    a, b = R.f64(a), R.f64(b)
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def oracle_sd(D, hd, qg, kg, wqkv=None):
    eye = torch.eye(D, dtype=torch.float64)
    wq, wk, wv = (eye, eye, eye) if wqkv is None else wqkv.split(D, 0)
    p = "blocks.0.attn."
    z = torch.zeros(D, dtype=torch.float64)
    return {p + "query.weight": wq, p + "key.weight": wk, p + "value.weight": wv, p + "query.bias": z, p + "key.bias": z, p + "value.bias": z,
            p + "q_norm.g": qg.double(), p + "k_norm.g": kg.double(), p + "c_proj.weight": eye}


@pytest.mark.parametrize("B,T,H,hd", [(1, 1, 1, 4), (3, 5, 2, 8), (2, 16, 3, 20), (2, 33, 2, 16)])
@pytest.mark.parametrize("p", [0.0, 0.3])
def test_attn_ref_is_the_oracles_causal_attention(B, T, H, hd, p):
    D = H * hd
    h = R.rnd(B, T, D, seed=T)
    h[0, 0, :hd] = 0                                                                   # one clamped row on the way
    qg, kg = 3 + 0.1 * R.rnd(hd, seed=1), 1 + 0.1 * R.rnd(hd, seed=2)
    keep = O.attn_keep_scale(5, B, H, T, p).double() if p else None
    for w in (None, R.rnd(3 * D, D, seed=3) * D ** -0.5):
        ref = O.causal_attention(oracle_sd(D, hd, qg, kg, w), 0, h, H, keep_scale=keep)
        qkv = torch.cat([h, h, h], -1) if w is None else h @ w.t()
        got = R.attn_ref(qkv.reshape(B * T, 3 * D), qg, kg, B, T, H, hd, keep=keep)
        assert rel(got, ref.reshape(B * T, D)) < 1e-12


@pytest.mark.parametrize("B,T,H,hd", [(2, 1, 2, 4), (3, 7, 2, 12), (1, 16, 3, 128), (2, 40, 1, 24)])
def test_attn_ref_is_torch_sdpa_after_the_oracles_rmsnorm(B, T, H, hd):
    inp = R.make_inputs("peaked", B, T, H, hd, F32)
    q, k, v = R.split_qkv(inp.qkv.double(), B, T, H, hd)
    ref = F.scaled_dot_product_attention(O.rmsnorm(q, inp.qg.double()), O.rmsnorm(k, inp.kg.double()), v, is_causal=True)
    assert rel(R.attn_ref(inp.qkv, inp.qg, inp.kg, B, T, H, hd), R.merge(ref)) < 1e-12


def test_backward_reference_against_central_differences():
    """B = 1, H = 2, T = 3, hd = 4 with the `clamped` family's rows: a zero q row, a zero k row, a tiny q row and a tiny k row.  Inside the clamp the
    forward is linear in the row (x / eps * g), so central differences with a step far below eps hold there too; the zero rows' gradients are also
    checked for being finite and of the clamp form g * dxh / eps (no projection term: scaling the row scales nothing else)."""
    B, T, H, hd = 1, 3, 2, 4
    inp = R.make_inputs("clamped", B, T, H, hd, F32)
    assert len(inp.clamped["q"]) == 2 and len(inp.clamped["k"]) == 2
    qkv, qg, kg, dy = inp.qkv.double(), inp.qg.double().expand(B, H, hd).clone(), inp.kg.double().expand(B, H, hd).clone(), inp.dy.double()
    ref = R.attn_bwd_ref(qkv, inp.qg, inp.kg, dy, B, T, H, hd)
    assert all(bool(torch.isfinite(t).all()) for t in ref.values())
    loss = lambda x, a, b: float((R.merge(torch.matmul(*R.attn_parts(x, a, b, B, T, H, hd)[3:1:-1])) * dy).sum())
    assert abs(loss(qkv, qg, kg) - float((ref["y"] * dy).sum())) < 1e-12

    def fd(t, which):
        g = torch.zeros_like(t)
        flat, gf = t.view(-1), g.view(-1)
        for i in range(flat.numel()):
            step = 1e-10 if abs(float(flat[i])) < 1e-6 and which == 0 else 1e-6
            old = float(flat[i])
            vals = []
            for sgn in (1, -1):
                flat[i] = old + sgn * step
                vals.append(loss(qkv, qg, kg))                                     # t is one of the three, stepped in place
            flat[i] = old
            gf[i] = (vals[0] - vals[1]) / (2 * step)
        return g
    # rows inside the clamp carry gradients ~1e6 times the others: compare per block and per clamped row, not over the tensor
    errs = R.block_errors(ref["dqkv"], fd(qkv, 0), None, B, T, H, hd, ("dq", "dk", "dv"), inp.clamped)
    errs += R.row_errors(ref["dgq"], fd(qg, 1).reshape(B * H, hd), None, "dgq") + R.row_errors(ref["dgk"], fd(kg, 2).reshape(B * H, hd), None, "dgk")
    w, where = R.worst(errs)
    print(f"autograd against central differences: worst block {w:.2e} at {where}")
    assert w < 1e-5
    # clamp form of the clamped q rows: dq = qg * d q_hat / eps, d q_hat = (dS k_hat) from an autograd of its own on q_hat
    q, k, v = R.split_qkv(qkv, B, T, H, hd)
    qh = (q / R.qk_rms(q, R.EPS) * R.gain4(qg, B, H, hd)).detach().requires_grad_(True)
    kh = k / R.qk_rms(k, R.EPS) * R.gain4(kg, B, H, hd)
    att = ((qh @ kh.transpose(-2, -1)) / math.sqrt(hd)).masked_fill(~R.causal_mask(T), float("-inf")).softmax(-1)
    (R.merge(att @ v) * dy).sum().backward()
    dq = R.blocks(ref["dqkv"], B, T, H, hd)[0]
    for b, h, t in inp.clamped["q"]:
        want = qg[b, h] * qh.grad[b, h, t] / R.EPS
        assert float((dq[b, h, t] - want).norm()) <= 1e-12 * float(want.norm())


# ------------------------------------------------------------------------------------------------------------------ wrong references
@pytest.mark.parametrize("path,dtype,B,T,H,hd,family,p", R.SENSITIVITY)
def test_each_wrong_reference_moves_far_outside_the_gpu_bound(path, dtype, B, T, H, hd, family, p):
    inp = R.make_inputs(family, B, T, H, hd, dtype)
    keep = O.attn_keep_scale(R.SEED, B, H, T, p) if p else None
    case = R.fwd_case(inp, keep) if path == "fwd" else R.bwd_case(inp, keep)
    wrongs = R.applicable_wrongs(path, dtype, T, hd, family, p, B, H)
    assert wrongs
    for wrong in wrongs:
        moved, where = R.worst(R.wrong_errors(path, wrong, inp, case, keep, got=case["ref"]))
        print(f"{path} {dtype} {family} T={T} hd={hd} p={p}: {wrong} moves the reference by {moved:.2e} ({moved / case['rtol']:.0f} x the bound) at {where}")
        margin = R.PADDED_BF16_MARGIN if (wrong, dtype) == ("padded_hd", BF16) else 10
        assert moved > margin * case["rtol"], wrong


def test_every_wrong_reference_has_a_case():
    seen = set()
    for path, dtype, B, T, H, hd, family, p in R.SENSITIVITY:
        seen |= set(R.applicable_wrongs(path, dtype, T, hd, family, p, B, H))
    assert seen == set(R.WRONGS)


# ------------------------------------------------------------------------------------------------------------------ the gap tables
def _gap_table(path, dtype, Ts, cases_of):
    worst_gap, rule, dominated, blocks_n = {}, [], {f: 0 for f in R.FAMILIES}, {f: 0 for f in R.FAMILIES}
    for T in Ts:
        for cs in cases_of(dtype, T):
            B, H, hd, family = cs[:4]
            p = cs[4] if len(cs) > 4 else 0.0
            inp = R.make_inputs(family, B, T, H, hd, dtype)
            keep = O.attn_keep_scale(R.SEED, B, H, T, p) if p else None
            case = R.fwd_case(inp, keep) if path == "fwd" else R.bwd_case(inp, keep)
            assert math.isfinite(case["gap"]), (T, cs, case["gap_at"])
            assert case["gap"] <= case["rtol"] / 4, (T, cs)                              # the reference alone stays inside before a GPU is involved
            if case["rtol"] > case["start"]:
                rule.append((T, B, H, hd, family, p, case["gap"]))
            worst_gap[family] = max(worst_gap.get(family, (0.0,)), (case["gap"], T, hd, p, case["gap_at"]))
            # how often the floor term exceeds the relative term (measured with the floor for every family; `soft` is then held without it)
            a = (inp.qkv, inp.qg, inp.kg) + ((inp.dy,) if path == "bwd" else ()) + (B, T, H, hd)
            if path == "fwd":
                errs = R.block_errors(case["ref"], case["ref"], R.attn_floor_fwd(*a, keep=keep), B, T, H, hd, ("y",))
            else:
                errs = R.bwd_errors(case["ref"]["dqkv"], case["ref"]["dgq"], case["ref"]["dgk"], dict(ref=case["ref"], floor=R.attn_bwd_floor(*a, keep=keep)), inp)
            dominated[family] += R.floor_dominates(errs); blocks_n[family] += len(errs)
            assert (case["floor"] is None) == (family != "peaked")                     # zero uses of the floor term for `soft` (and `clamped`)
    for f in R.FAMILIES:
        g = worst_gap[f]
        print(f"{path} {dtype} {f}: worst reference-alone gap {g[0]:.2e} (T={g[1]} hd={g[2]} p={g[3]} {g[4]}), starting value {R.START[path, dtype]:.1e}; "
              f"floor above the relative term in {dominated[f]} of {blocks_n[f]} blocks, used in {blocks_n[f] if R.use_floor(f) else 0}")
    for r in rule:
        print(f"  4x rule: {path} {dtype} T={r[0]} B={r[1]} H={r[2]} hd={r[3]} {r[4]} p={r[5]}: gap {r[6]:.2e} -> bound {4 * r[6]:.2e}")
    return rule


@pytest.mark.parametrize("dtype", [BF16, F32])
@pytest.mark.parametrize("span", ["short", "long"])
def test_forward_gap_table(span, dtype):
    _gap_table("fwd", dtype, R.FWD_SHORT_T if span == "short" else R.FWD_LONG_T, R.fwd_cases)


@pytest.mark.parametrize("dtype", [BF16, F32])
@pytest.mark.parametrize("span", ["short", "long"])
def test_backward_gap_table(span, dtype):
    _gap_table("bwd", dtype, R.BWD_SHORT_T if span == "short" else R.BWD_LONG_T, R.bwd_cases)
