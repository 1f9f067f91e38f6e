"""tests/gemm_refs.py without a GPU: (a) the fp64 reference of mode_gemm agrees with the same operation written a second way (per-row Python loops,
torch.nn.functional activations on the assembled pre-activation); (b) the bound has power: an fp32 torch stand-in for a correct kernel stays inside it
for every case of the GPU test's table, and every deliberate defect of the stand-in leaves it at one shape per epilogue; (c) every case of the table
is taken by the kernel it names, by the launchers' acceptance conditions restated in gemm_refs.py."""
import pytest
import torch
import torch.nn.functional as F

import gemm_refs as R
from gemm_refs import BF16, F32, NONE, BIAS, BIAS_GELU, RESIDUAL, SWIGLU, RESIDUAL_NORM
from mode_diffusion_policy_amd import _lib as L

CASES = R.all_cases()
UNIQUE = list(dict.fromkeys(c._replace(kernel="", cfg=0, flags=c.flags & (R.SMALL_ROWS | R.IDENTITY_ROWS)) for c in CASES))   # data and output dtype


def test_constants_are_the_bindings():
    assert (NONE, BIAS, BIAS_GELU, RESIDUAL, SWIGLU, RESIDUAL_NORM) == (L.EPI_NONE, L.EPI_BIAS, L.EPI_BIAS_GELU, L.EPI_RESIDUAL, L.EPI_SWIGLU,
                                                                         L.EPI_RESIDUAL_NORM)
    assert (R.SKINNY_OK, R.UNIFORM_GROUPS, R.SMALL_ROWS, R.IDENTITY_ROWS) == (L.GEMM_SKINNY_OK, L.GEMM_UNIFORM_GROUPS, L.GEMM_SMALL_ROWS,
                                                                              L.GEMM_IDENTITY_ROWS)


# ------------------------------------------------------------------------------------------------------------------ (a) the reference, a second way
def second_way(c, inp):
    """Row by row: one matrix-vector product per sorted row with its expert's matrix, then the activations of torch.nn.functional."""
    A, W, b = inp.A.double(), inp.W.double(), inp.bias.double()
    segs = [(0, c.M)] if c.counts is None else list(zip(inp.offsets[:-1].tolist(), inp.offsets[1:].tolist()))
    pre, mag = torch.empty(c.M, c.Nw, dtype=torch.float64), torch.empty(c.M, c.Nw, dtype=torch.float64)
    slabs = torch.empty(c.split_k, c.M, c.Nw, dtype=torch.float64)
    for e, (r0, r1) in enumerate(segs):
        for m in range(r0, r1):
            tok = int(inp.a_rows[m]) if c.gather else m
            acc, s = (W[e] * A[tok]).sum(1), (W[e] * A[tok]).abs().sum(1)
            for z in range(c.split_k):
                k0, k1 = z * c.K // c.split_k, (z + 1) * c.K // c.split_k
                slabs[z, m] = torch.mv(W[e][:, k0:k1], A[tok, k0:k1])
            if c.ss_n:
                norm = max(float(inp.row_ss[tok].double().sum()) ** 0.5 / c.K ** 0.5, inp.row_eps)
                acc, s = acc / norm, s / norm
            if c.epi in (BIAS, BIAS_GELU, SWIGLU):
                acc, s = acc + b[e, :c.Nw], s + b[e, :c.Nw].abs()
            if c.epi in (RESIDUAL, RESIDUAL_NORM):
                acc, s = acc + inp.resid[m].double(), s + inp.resid[m].double().abs()
            pre[m], mag[m] = acc, s
    out = dict(S_pre=mag)
    out["C"] = F.gelu(pre) if c.epi == BIAS_GELU else pre[:, :c.N] * F.silu(pre[:, c.N:]) if c.epi == SWIGLU else pre
    if c.epi == RESIDUAL_NORM:
        out["C2"] = pre * inp.gain.double()
        out["row_ss_out"] = torch.stack([pre[:, g0:g0 + c.group].square().sum(1) for g0 in range(0, c.N, c.group)], 1)
    if c.split_k > 1:
        out["slab"] = slabs
    return out


def _kind(c):
    return (c.epi, c.family, bool(c.counts), c.gather, c.split_k > 1, bool(c.ss_n), c.dtype, c.group)


SECOND_WAY = list({_kind(c): c for c in sorted(UNIQUE, key=lambda c: c.M * c.Nw * c.K) if c.M * c.Nw * c.K <= 2 ** 22}.values())


@pytest.mark.parametrize("c", SECOND_WAY, ids=lambda c: c.tag.replace(" ", "_"))
def test_reference_agrees_with_a_second_formulation(c):
    ref, _, _ = R.reference(c)
    other = second_way(c, R.inputs(c))
    for name, t in other.items():
        assert torch.allclose(ref[name], t, rtol=1e-12, atol=1e-12), (name, float((ref[name] - t).abs().max()))
    if c.split_k > 1:
        assert torch.allclose(ref["slab"].sum(0), ref["C"], rtol=1e-12, atol=1e-12)


def test_families_reach_what_they_are_for():
    """tails: pre-activations beyond +-6 and +-11 in one case and both signs in every 16 x 16 block; clamp: the clamped rows take the eps branch."""
    c = R.case("ring", 1, BIAS_GELU, F32, 65, 68, 128, family="tails")
    pre = R.reference(c)[0]["pre"]
    assert float(pre.min()) < -11 and float(pre.max()) > 11
    blocks = pre[:64, :64].reshape(4, 16, 4, 16).permute(0, 2, 1, 3).reshape(16, 256)
    assert bool((blocks.min(1).values < -6).all()) and bool((blocks.max(1).values > 6).all())
    c = R.case("ring", 1, SWIGLU, BF16, 0, 68, 128, family="clamp", counts=(0, 1, 128, 129), gather=True, ss_n=16)
    inp, ref = R.inputs(c), R.reference(c)[0]
    rows = [m for m in range(c.M) if int(inp.a_rows[m]) in inp.clamped]
    assert len(rows) >= 3 and all(float(ref["rfac"][m]) == 1 / R.CLAMP_EPS for m in rows)
    assert sum(float(ref["rfac"][m]) != 1 / R.CLAMP_EPS for m in range(c.M)) == c.M - len(rows)


# ------------------------------------------------------------------------------------------------------------------ (b) the bound has power
DEFECTS = ("k_drop", "bias_shift", "truncate", "resid_row", "no_gain", "ss_60", "slab_range", "swap_halves", "no_eps", "next_expert")


def to_bf16(t, truncate):
    if truncate:
        return (t.float().contiguous().view(torch.int32) & -65536).view(torch.float32).to(BF16)
    return t.to(BF16)


def standin(c, inp, defect=None):
    """A correct kernel's stand-in: fp32 torch matmul on the CPU, the epilogue in fp32, rounded to the output dtype with .to(torch.bfloat16) - or the
    same with one deliberate defect.  Returns the dict of outputs the GPU test reads back."""
    A, W, bias = inp.A.float(), inp.W.float(), inp.bias[:, :c.Nw].clone()
    M, N, K, Nw = c.M, c.N, c.K, c.Nw
    rows = torch.arange(M) if not c.gather else inp.a_rows.long()
    eid = torch.zeros(M, dtype=torch.long) if c.counts is None else torch.bucketize(torch.arange(M), inp.offsets.long()[1:], right=True)
    if defect == "next_expert":
        m = int(inp.offsets[-2]) - 1                                     # the last row before the last expert's segment
        assert eid[m] + 1 < c.E
        eid = eid.clone(); eid[m] += 1
    Ag = A[rows]

    def product(k0, k1):
        acc = torch.zeros(M, Nw)
        for e in range(c.E):
            sel = eid == e
            if bool(sel.any()):
                acc[sel] = Ag[sel, k0:k1] @ W[e, :, k0:k1].t()
        return acc

    acc = product(0, K)
    if defect == "k_drop":
        acc[:16, :16] = product(0, K - 32)[:16, :16]
    got = {}
    tr = defect == "truncate"
    if c.split_k > 1:
        ks = K // c.split_k
        slabs = [product(z * ks, (z + 1) * ks) for z in range(c.split_k)]
        if defect == "slab_range":
            slabs[1] = slabs[0].clone()
        if defect == "k_drop":
            slabs[0][:16, :16] = product(0, ks - 32)[:16, :16]
        got["slab"] = torch.stack([to_bf16(s, tr) if c.out == BF16 else s for s in slabs])
        return got
    if c.ss_n:
        ss = inp.row_ss[rows].sum(1)
        eps = torch.full((M,), inp.row_eps)
        if defect == "no_eps":
            eps[[m for m in range(M) if int(rows[m]) == inp.clamped[0]]] = 0.0
        acc = acc * (1.0 / torch.maximum(ss.sqrt() * torch.tensor(float(K)).rsqrt(), eps))[:, None]
    if c.epi in (BIAS, BIAS_GELU, SWIGLU):
        b = bias[eid]
        if defect == "bias_shift":
            b[:, N - 4:N] = bias[eid][:, N - 8:N - 4]
        acc = acc + b
    if c.epi in (RESIDUAL, RESIDUAL_NORM):
        r = inp.resid.clone()
        if defect == "resid_row":
            r[1] = inp.resid[0]
        acc = acc + r
    if c.epi == BIAS_GELU:
        out = F.gelu(acc)
    elif c.epi == SWIGLU:
        v, g = (acc[:, N:], acc[:, :N]) if defect == "swap_halves" else (acc[:, :N], acc[:, N:])
        out = v * F.silu(g)
    else:
        out = acc
    got["C"] = to_bf16(out, tr) if c.out == BF16 else out
    if c.epi == RESIDUAL_NORM:
        got["C2"] = to_bf16(out if defect == "no_gain" else out * inp.gain, tr)
        sq = out * out
        if defect == "ss_60":
            sq[:, c.group - 4:c.group] = 0
        got["row_ss_out"] = sq.reshape(M, N // c.group, c.group).sum(2)
    return got


def clamped_rows(c, inp):
    return [m for m in range(c.M) if (int(inp.a_rows[m]) if c.gather else m) in inp.clamped]


def worst_ratio(c, defect=None):
    inp = R.inputs(c)
    ref, b, _ = R.reference(c)
    rs = R.ratios(standin(c, inp, defect), ref, b, clamped_rows(c, inp))
    return max(rs, key=lambda r: r[1])


@pytest.mark.parametrize("epi", range(6), ids=R.EPI_NAME)
def test_correct_standin_is_inside_the_bound_for_every_case(epi):
    worst = (None, 0.0, None)
    for c in (c for c in UNIQUE if c.epi == epi):
        name, q, idx = worst_ratio(c)
        assert q <= 1.0, f"{c.tag}: {name}{list(idx)} err / bound = {q:.3g}"
        if q > worst[1]:
            worst = (name, q, c.tag)
    print(f"{R.EPI_NAME[epi]}: worst err / bound of the stand-in {worst[1]:.3g} ({worst[2]} {worst[0]})")


def _applies(defect, c):
    grouped_next = bool(c.counts) and c.counts[-1] > 0 and c.counts[-2] > 0
    return {
        "k_drop": c.K >= 64 and c.M >= 16,
        "bias_shift": c.epi in (BIAS, BIAS_GELU, SWIGLU) and c.N >= 8,
        # (K <= 256: at K = 1024 the accumulation term (K + 2) u S reaches the bf16 half unit itself, and a truncating store then leaves the bound on
        # a tenth of the elements instead of half)
        "truncate": (c.out == BF16 or c.epi == RESIDUAL_NORM) and c.M * c.N >= 1024 and c.K <= 256,
        "resid_row": c.epi in (RESIDUAL, RESIDUAL_NORM) and c.M >= 2,
        "no_gain": c.epi == RESIDUAL_NORM,
        "ss_60": c.epi == RESIDUAL_NORM and c.group == 64,
        "slab_range": c.split_k > 1,
        "swap_halves": c.epi == SWIGLU,
        "no_eps": c.epi == SWIGLU and c.family == "clamp",
        "next_expert": grouped_next and c.split_k == 1,
    }[defect]


def defect_cases():
    """(defect, case): the first case of the table each defect applies to, per epilogue."""
    out = []
    for defect in DEFECTS:
        for epi in range(6):
            c = next((c for c in UNIQUE if c.epi == epi and c.dtype == BF16 and _applies(defect, c)), None)
            if c is not None:
                out.append((defect, c))
    return out


DEFECT_CASES = defect_cases()


def test_every_defect_has_a_case_at_every_epilogue_it_can_touch():
    have = {(d, c.epi) for d, c in DEFECT_CASES}
    every = set(range(6))
    want = {"k_drop": every, "bias_shift": {BIAS, BIAS_GELU, SWIGLU}, "truncate": every - {RESIDUAL}, "resid_row": {RESIDUAL, RESIDUAL_NORM},
            "no_gain": {RESIDUAL_NORM}, "ss_60": {RESIDUAL_NORM}, "slab_range": {NONE}, "swap_halves": {SWIGLU}, "no_eps": {SWIGLU},
            "next_expert": {NONE, BIAS, SWIGLU}}
    for d, epis in want.items():
        assert {(d, e) for e in epis} <= have, d


@pytest.mark.parametrize("defect,c", DEFECT_CASES, ids=lambda v: v if isinstance(v, str) else v.tag.replace(" ", "_"))
def test_each_defect_leaves_the_bound(defect, c):
    name, q, idx = worst_ratio(c, defect)
    print(f"{defect} at {c.tag}: err / bound = {q:.3g} at {name}{list(idx)}")
    assert q > 1.0, f"a kernel with {defect} would pass {c.tag}"
    if defect == "truncate":                                             # "on about half of the elements"
        inp = R.inputs(c)
        ref, b, _ = R.reference(c)
        name = "C2" if c.epi == RESIDUAL_NORM else "slab" if c.split_k > 1 else "C"
        g = standin(c, inp, defect)[name]
        frac = float(((g.double() - ref[name]).abs() > b[name]).double().mean())
        assert 0.3 < frac < 0.7, frac


# ------------------------------------------------------------------------------------------------------------------ (c) the kernel a case names
def test_every_case_is_taken_by_the_kernel_it_names():
    assert len(CASES) > 1000
    for c in CASES:
        assert R.kernel_of(c) == c.kernel, c.tag
        if c.kernel == "ring" and c.cfg:
            assert R.ring_accepts(c), c.tag
    for kernel in ("ring", "pp", "stream", "mid", "f32"):
        assert any(c.kernel == kernel for c in CASES)
    assert {R.f32_kernel(c) for c in CASES if c.dtype == F32} == {"f32-dot", "f32-gemv", "f32-mfma"}


def test_refused_descriptors_are_refused_by_the_predicates_too():
    ok = R.case("ring", 1, NONE, F32, 65, 68, 128)
    assert R.ring_accepts(ok)
    for bad in (ok._replace(K=96), ok._replace(N=66), ok._replace(pad=(4, 8, 8, 0)), ok._replace(epi=BIAS, split_k=2),
                ok._replace(flags=R.SMALL_ROWS)):
        assert not R.ring_accepts(bad), bad.tag
    assert R.kernel_of(R.case("stream", 1, NONE, F32, 17, 20, 128, flags=R.SMALL_ROWS)) == "refused"
