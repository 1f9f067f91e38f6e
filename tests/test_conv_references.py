"""tests/conv_refs.py without a GPU: (a) the table-level fp64 reference of the implicit-GEMM convolution equals the convolution-level one (F.conv2d
and its autograd) through index tables written as plain loops, and perceptual_encoders._tap_table builds those same tables in both orientations;
(b) the bound has power: an fp32 torch stand-in for a correct kernel stays inside it for every case of the GPU test's table, and each deliberate defect
of the stand-in (the ones a tile kernel can have) leaves it; (c) the dispatch predicates send the case table to all twelve kernels of
csrc/conv_gemm.hip; (d) the BatchNorm fold's reference is nn.BatchNorm2d's."""
import pytest
import torch
import torch.nn.functional as F

import conv_refs as R
from conv_refs import BF16
from mode_diffusion_policy_amd import _lib as L

CASES = R.all_cases()
UNIQUE = list(dict.fromkeys(c.data_key for c in CASES))
SMALL = [c for c in UNIQUE if c.M * c.N <= 2 ** 20]
LARGE = [c for c in UNIQUE if c.M * c.N > 2 ** 20]


def test_constants_and_descriptor_fields_are_the_bindings():
    assert R.W_KN == L.GEMM_W_KN and L.EPI_NONE == 0 and L.MODE_BF16 == 0
    gemm = [f[0] for f in L.ModeGemmDesc._fields_]
    assert {"a_rows", "a_tap_cols", "a_rows_tap_stride", "flags", "split_k", "k_group_offsets"} <= set(gemm)
    assert gemm.index("a_rows_tap_stride") == gemm.index("a_tap_cols") + 1
    assert [f[0] for f in L.ModeConvBnDesc._fields_] == [
        "x", "ldx", "idx", "idx_tap_stride", "taps", "w", "ldw", "y", "ldy", "M", "Cin", "Cout", "bn_mean", "bn_var", "bn_weight", "bn_bias", "bn_eps",
        "residual", "ldr", "relu", "pre_gamma", "pre_beta", "post_gamma", "post_beta", "rows_per_sample", "stat_sum", "stat_sq"]


# ------------------------------------------------------------------------------------------------------------------ (a) two levels, one operation
@pytest.mark.parametrize("cv", R.CONVS, ids=lambda cv: cv.tag.replace(" ", "_"))
def test_table_level_reference_is_the_convolution(cv):
    """Forward: A = X rows, the channels_last weight read K-contiguously; data gradient: A = dY rows, the same weight memory read as [k = (t, cout)][cin]
    (MODE_GEMM_W_KN: ldw = taps * cin, N = cin).  Both against F.conv2d / its autograd in fp64, magnitude sums included."""
    ref = R.conv_reference(cv)
    fwd, tr = R.tap_tables_by_loop(cv)
    X, Wf, dY, Wkn = R.conv_as_tables(cv)
    y, Sy = R.table_product(X, fwd, Wf, cv.rows_out, cv.cout, cv.cin, cv.taps, False)
    dx, Sdx = R.table_product(dY, tr, Wkn, cv.rows_in, cv.cin, cv.cout, cv.taps, True)
    for got, want in ((y, ref["y"]), (Sy, ref["S_y"]), (dx, ref["dx"]), (Sdx, ref["S_dx"])):
        assert got.shape == want.shape and torch.allclose(got, want, rtol=1e-12, atol=1e-12), float((got - want).abs().max())


@pytest.mark.parametrize("cv", R.CONVS, ids=lambda cv: cv.tag.replace(" ", "_"))
def test_tap_table_builds_the_loops_tables_in_both_orientations(cv):
    from mode_diffusion_policy_amd import perceptual_encoders as E
    fwd, tr = R.tap_tables_by_loop(cv)
    args = (cv.n, cv.H, cv.W, cv.ho, cv.wo, cv.kh, cv.kw, cv.sh, cv.sw, cv.ph, cv.pw, torch.device("cpu"))
    assert torch.equal(E._tap_table(*args).long(), fwd)
    assert torch.equal(E._tap_table(*args, transposed=True).long(), tr)


def test_the_convolutions_hold_the_edges_they_are_for():
    fwd = {cv: R.tap_tables_by_loop(cv)[0] for cv in R.CONVS}
    assert any(bool((t < 0).all(0).any()) for t in fwd.values())                   # an output pixel no tap of which meets the image
    assert any(cv.H < cv.kh for cv in R.CONVS) and any(cv.n == 1 for cv in R.CONVS) and any(cv.kh != cv.kw and cv.sh != cv.sw for cv in R.CONVS)
    assert any(cv.rows_out < 128 for cv in R.CONVS) and any(cv.rows_out > 384 for cv in R.CONVS)
    assert {64, 128} <= {cv.cin for cv in R.CONVS} and {64, 128} <= {cv.cout for cv in R.CONVS}


# ------------------------------------------------------------------------------------------------------------------ (b) the bound has power
DEFECTS = ("film_row0", "zero_row", "k_drop", "truncate", "resid_row")


def standin(c, inp, defect=None):
    """A correct kernel's stand-in: per-tap fp32 torch matmuls on the CPU, the epilogue in fp32 in the kernel's order, rounded with .to(bfloat16) - or the
    same with one deliberate defect.  Returns y [M, N] bf16."""
    M, N, tk = c.M, c.N, c.tap_k
    A, W = inp.A.float(), inp.W.float()
    A = torch.where(torch.isnan(A), torch.full_like(A, 1e30), A)          # a read of a never-read element shows (NaN itself would spoil 0 * NaN)
    acc = torch.zeros(M, N)
    for t in range(c.taps):
        if inp.idx is None:
            At = A[:M]
        else:
            it = inp.idx[t].long()
            At = torch.where((it >= 0)[:, None], A[it.clamp_min(0)], torch.zeros(()))
            if defect == "zero_row" and t == c.taps - 1:
                At = A[it.clamp_min(0)]                                    # row 0 in place of the zero row
        Wt = W[:, t * N:(t + 1) * N] if c.layout == "w_kn" else W[:, t * tk:(t + 1) * tk].t()
        if defect == "k_drop" and t == c.taps - 1:
            At, Wt = At[:, :tk - 64], Wt[:tk - 64]                         # the last K-step of 64
        acc += At @ Wt
    v = acc
    sample = torch.arange(M) // max(c.rps, 1)
    if defect == "film_row0":
        sample = (torch.arange(M) // 128 * 128) // max(c.rps, 1)
    if "bn" in c.terms:
        sc, sh = R.scale_shift(inp.bn_mean, inp.bn_var, inp.bn_w if "bn_w" in c.terms else None, inp.bn_b if "bn_b" in c.terms else None, R.BN_EPS,
                               torch.float32)
        v = v * sc + sh
    if "pre" in c.terms:
        v = inp.pre_g[sample] * v + inp.pre_b[sample]
    if "res" in c.terms:
        r = inp.res.float()
        if defect == "resid_row":
            r = r.roll(1, 0)
        v = v + r
    if "relu" in c.terms:
        v = v.clamp_min(0)
    if "post" in c.terms:
        v = (1 + inp.post_g[sample]) * v + inp.post_b[sample]
    if defect == "truncate":
        return (v.contiguous().view(torch.int32) & -65536).view(torch.float32).to(BF16)
    return v.to(BF16)


def worst_ratio(c, defect=None):
    ref, b, _ = R.reference(c)
    return max(R.ratios(dict(C=standin(c, R.inputs(c), defect)), ref, b), key=lambda r: r[1])


@pytest.mark.parametrize("part", range(8))
def test_correct_standin_is_inside_the_bound_for_every_small_case(part):
    worst = (0.0, "")
    for c in SMALL[part::8]:
        name, q, idx = worst_ratio(c)
        assert q <= 1.0, f"{c.tag}: {name}{list(idx)} err / bound = {q:.3g}"
        worst = max(worst, (q, c.tag))
        inp = R.inputs(c)
        if inp.zero_row is not None and c.kind == "gemm":
            assert bool((R.reference(c)[0]["C"][inp.zero_row] == 0).all()) and bool((R.reference(c)[1]["C"][inp.zero_row] == 0).all())
    print(f"worst err / bound of the stand-in {worst[0]:.3g} ({worst[1]})")


@pytest.mark.parametrize("c", LARGE, ids=lambda c: c.tag.replace(" ", "_"))
def test_correct_standin_is_inside_the_bound_for_the_wide_cases(c):
    name, q, idx = worst_ratio(c)
    assert q <= 1.0, f"{c.tag}: {name}{list(idx)} err / bound = {q:.3g}"


def _applies(defect, c):
    return {"film_row0": ("pre" in c.terms or "post" in c.terms) and c.rps < 128 and c.M > c.rps,
            "zero_row": not c.direct and c.M >= 16, "k_drop": c.M >= 16, "truncate": c.M * c.N >= 1024 and c.K <= 256,
            "resid_row": "res" in c.terms and c.M >= 2}[defect]


DEFECT_CASES = [(d, next(c for c in SMALL if c.kind == kind and _applies(d, c))) for d in DEFECTS for kind in ("gemm", "fused")
                if any(c.kind == kind and _applies(d, c) for c in SMALL)]


@pytest.mark.parametrize("defect,c", DEFECT_CASES, ids=lambda v: v if isinstance(v, str) else v.tag.replace(" ", "_"))
def test_each_defect_leaves_the_bound(defect, c):
    name, q, idx = worst_ratio(c, defect)
    print(f"{defect} at {c.tag}: err / bound = {q:.3g} at {name}{list(idx)}")
    assert q > 1.0, f"a kernel with {defect} would pass {c.tag}"


def test_every_defect_has_its_cases():
    have = {(d, c.kind) for d, c in DEFECT_CASES}
    assert {("film_row0", "fused"), ("resid_row", "fused")} <= have
    assert {(d, k) for d in ("zero_row", "k_drop", "truncate") for k in ("gemm", "fused")} <= have


def test_families_reach_what_they_are_for():
    """ReLU clips about half of the elements in every family; the poison family holds NaN exactly where the contract says nothing is read, and its
    reference is finite; every table has its all-(-1) tap and row."""
    for c in (c for c in SMALL if "relu" in c.terms):
        assert 0.3 < R.reference(c)[0]["clipped"] < 0.7, c.tag
    for c in (c for c in SMALL if c.family == "poison"):
        inp = R.inputs(c)
        assert bool(torch.isnan(inp.A_buf[inp.dead]).all()) and bool(torch.isnan(inp.A_buf[:, c.tap_k:]).all()) and bool(torch.isnan(inp.W_buf[:, c.wrow:]).all())
        assert bool(torch.isnan(inp.res_buf[:, c.N:]).all()) and not bool(torch.isnan(inp.A).all(1)[[i for i in range(inp.A.shape[0]) if i not in set(inp.dead.tolist())]].any())
        assert bool(torch.isfinite(R.reference(c)[0]["C"]).all())
        if inp.idx is not None:
            named = set(inp.idx_buf.tolist()) - {-1}
            slack = set(inp.idx_buf.view(c.taps, c.idx_stride)[:, c.M:].reshape(-1).tolist())
            assert slack <= set(inp.dead.tolist()) and not (set(inp.idx.reshape(-1).tolist()) & set(inp.dead.tolist())) and max(named) < inp.A_buf.shape[0]
    for c in (c for c in SMALL if not c.direct):
        inp = R.inputs(c)
        live = [t for t in range(c.taps) if t != inp.zero_tap]           # drawn with p = 0.15 .. 0.30 (+ the zero row): 3 sigma of 256 draws is 0.09
        frac = float((inp.idx[live] < 0).double().mean())
        assert (c.taps < 2 or bool((inp.idx[inp.zero_tap] == -1).all())) and (c.M < 2 or bool((inp.idx[:, inp.zero_row] == -1).all()))
        assert c.M * len(live) < 256 or 0.05 < frac < 0.42, (c.tag, frac)
        assert inp.zero_tap is None or inp.zero_tap < c.taps - 1


def test_stat_bound_takes_an_fp32_sum_and_not_a_sum_that_skips_rows():
    c = R.stat_cases()[0]
    y = standin(c, R.inputs(c))
    tiles = [y[t * 128:(t + 1) * 128].float() for t in range(c.m_tiles)]
    s, q = torch.stack([t.sum(0) for t in tiles]), torch.stack([(t * t).sum(0) for t in tiles])
    assert all(r[1] <= 1.0 for r in R.stat_ratios(y, s, q, c.M))
    s2 = torch.stack([t[:8].sum(0) + t[16:].sum(0) for t in tiles])              # the partner rows of one shuffle missing
    assert any(r[1] > 1.0 for r in R.stat_ratios(y, s2, q, c.M))


# ------------------------------------------------------------------------------------------------------------------ (c) the kernel a case reaches
def test_the_case_table_reaches_all_twelve_kernels():
    reached = {c.kernel for c in CASES}
    assert reached == set(R.ALL_KERNELS) and len(R.ALL_KERNELS) == 12, sorted(set(R.ALL_KERNELS) - reached)
    for k in R.ALL_KERNELS:
        print(k, sum(c.kernel == k for c in CASES), "launches")
    at, below = R.WIDE[0], R.NARROW_NEIGHBOUR
    t128 = lambda M, N: -(-M // 128) * -(-N // 128)
    assert t128(*at[:2]) == 384 and R.takes_wide(*at[:2]) and t128(*below[:2]) < 384 and not R.takes_wide(*below[:2]) and at[1] == below[1]
    assert t128(*R.WIDE[2][:2]) == 384 and R.takes_wide(*R.WIDE[2][:2]) and not R.takes_wide(128 * 384, 72) and not R.takes_wide(128 * 383, 128)
    # the automatic ring depth (conv_launch): two slots from 2 x 256 workgroups on
    assert R.ring_depth(128 * 511, 64, False) == 3 and R.ring_depth(128 * 512, 64, False) == 2 and R.ring_depth(128 * 256, 72, False) == 2
    assert R.ring_depth(128 * 48, 1024, True) == 3 and R.ring_depth(128 * 64, 1024, True) == 2 and R.ring_depth(1, 8, False, 2) == 2
    assert all(not R.takes_wide(c.M, c.N) for c in SMALL)                      # what the suite launched before: three of the twelve
    # the training shapes the issue names: ResNet-50 at 224 x 224, batch 64: layer1's 3 x 3 (1568 tiles: two slots), layer2's 3 x 3 at 28 x 28 (BN = 128)
    assert R.ring_depth(64 * 56 * 56, 64, R.takes_wide(64 * 56 * 56, 64)) == 2 and R.takes_wide(64 * 28 * 28, 128)


# ------------------------------------------------------------------------------------------------------------------ (d) the BatchNorm fold
@pytest.mark.parametrize("momentum", (0.1, -1.0))
def test_bn_partials_reference_is_batch_norm(momentum):
    g = torch.Generator().manual_seed(5)
    x = torch.randn(157 * 4, 72, generator=g, dtype=torch.float64) * 2 + 0.5
    w, b = torch.randn(72, generator=g).float(), torch.randn(72, generator=g).float()
    rm, rv = torch.randn(72, generator=g).float(), (0.5 + torch.rand(72, generator=g)).float()
    psum, psq = x.reshape(157, 4, 72).sum(1), x.reshape(157, 4, 72).square().sum(1)
    ref, bound = R.bn_partials_ref(psum, psq, float(x.shape[0]), w, b, 1e-5, momentum, rm, rv, 3)
    rm2, rv2 = rm.double(), rv.double()
    y = F.batch_norm(x, rm2, rv2, w.double(), b.double(), True, 0.1 if momentum >= 0 else 0.25, float(torch.tensor(1e-5)))
    assert torch.allclose(x * ref["scale"] + ref["shift"], y, rtol=1e-9, atol=1e-9)
    assert torch.allclose(ref["running_mean"], rm2, rtol=1e-7, atol=1e-7) and torch.allclose(ref["running_var"], rv2, rtol=1e-7, atol=1e-7)
    assert torch.allclose(ref["mean"], x.mean(0)) and torch.allclose(ref["var"], x.var(0, unbiased=False)) and all(bool((v >= 0).all()) for v in bound.values())
