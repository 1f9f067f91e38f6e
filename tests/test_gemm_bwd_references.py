"""tests/gemm_bwd_refs.py without a GPU: (a) the fp64 reference of the backward layouts agrees with the same descriptor read a second way (one
reduction row at a time); (b) the bound has power: an fp32 torch stand-in for a correct kernel stays inside it at every distinct (data, output dtype)
case of the GPU test's table, and every wrong reading of the descriptor leaves it at every case it can be stated for; (c) every case is taken by the
kernel, geometry and path it names, by the launchers' conditions restated in gemm_bwd_refs.py; (d) the poison families' reference is finite."""
import pytest
import torch

import gemm_bwd_refs as B
from gemm_bwd_refs import BF16, F32
from mode_diffusion_policy_amd import _lib as L

CASES = B.all_cases()
UNIQUE = list(dict.fromkeys(c._replace(kernel="", cfg=0, path=None) for c in CASES))      # data and output dtype
DATA = list(dict.fromkeys(c.data_key for c in CASES))


def test_constants_are_the_bindings():
    assert (B.W_KN, B.A_KM, B.NONE) == (L.GEMM_W_KN, L.GEMM_A_KM, L.EPI_NONE)
    assert torch.tensor(B.BF16_MAX).to(BF16).double().item() == B.BF16_MAX and torch.isinf(torch.tensor(B.BF16_MAX * 1.01).to(BF16))


# ------------------------------------------------------------------------------------------------------------------ (a) the reference, a second way
def second_way(c, inp):
    """One reduction row at a time, straight from the descriptor's words: C_z[m, n] += A-element * W-element, a rank-one update per row."""
    A, Z = inp.A.double(), c.Z
    out = torch.zeros(Z, c.M, c.N, dtype=torch.float64)
    if c.a_km:
        for z, (kb, ke) in enumerate(c.ranges):
            for r in range(kb, ke):
                if c.layout == "f32 lay 1":
                    w = inp.W[:, r].double()
                elif inp.idx is None:
                    w = inp.W[r, :c.N].double()
                else:
                    w = torch.zeros(c.N, dtype=torch.float64)
                    width = c.tap_cols or c.N
                    for t in range(c.taps):
                        i = int(inp.idx.reshape(-1)[t * c.tap_stride + r])
                        if i >= 0:
                            w[t * width:(t + 1) * width] = inp.W[i, :width].double()
                out[z] += torch.outer(A[r, :c.M], w)
    else:
        W = inp.W.double() if c.layout == "dgrad" else inp.W.double()[None]
        seg = inp.seg.tolist() if c.counts else [0, c.M]
        ksz = c.K // c.split_k
        for m in range(c.M):
            e = next(e for e in range(c.E) if seg[e] <= m < seg[e + 1])
            for z in range(c.split_k):
                out[z, m] = torch.einsum("k,kn->n", A[m, z * ksz:(z + 1) * ksz], W[e, z * ksz:(z + 1) * ksz, :c.N])
    return out


def _kind(c):
    return (c.layout, c.family, bool(c.counts), bool(c.kranges), c.split_k > 1, c.w_rows, c.taps > 1, c.pad[3] > 0)


SECOND_WAY = list({_kind(c): c for c in sorted(DATA, key=lambda c: -c.M * c.N * c.K)}.values())      # the smallest case of every kind


@pytest.mark.parametrize("c", SECOND_WAY, ids=lambda c: c.tag.replace(" ", "_"))
def test_reference_agrees_with_a_second_formulation(c):
    ref, _ = B.reference(c)
    other = second_way(c, B.inputs(c))
    assert torch.allclose(ref.C, other, rtol=1e-12, atol=1e-12), float((ref.C - other).abs().max())
    if c.split_k > 1:
        assert torch.allclose(ref.C.sum(0), ref.total, rtol=1e-12, atol=1e-12)
    for z, k in enumerate(ref.k):                                        # an empty range: exactly +0.0, and a bound of 0
        if k == 0:
            assert bool((ref.C[z] == 0).all()) and not bool(torch.signbit(ref.C[z]).any())


def test_families_reach_what_they_are_for():
    """spiky: both scalings present in both operands; poison: NaN in every pad column, in every row of A outside the groups and in every W row outside
    them (poison_max: the largest finite bf16 there), an index table that names a poisoned row outside the groups."""
    c = B.case("wgrad", "ring", 1, F32, 136, 72, kranges=B.RING_KG, family="spiky")
    inp = B.inputs(c)
    for t, scale in ((inp.A, 1.0), (inp.W, max(c.kranges[1]) ** -0.5)):
        a = t.double().abs() / scale
        assert 0.002 < float((a > 16).double().mean()) < 0.02 and 0.05 < float((a < 2.0 ** -7).double().mean()) < 0.2
    for fam in ("poison", "poison_max"):
        c = B.case("wgrad", "pptr", 6, F32, 256, 256, kranges=(67, B.PPTR_KG, 5), family=fam)
        inp, lo, hi = B.inputs(c), c.offsets[0], c.offsets[-1]
        assert lo == 67 and hi == c.K - 5 and c.ranges[0] == (67, 67)
        assert bool(torch.isnan(inp.A[:lo]).all()) and bool(torch.isnan(inp.A[hi:]).all()) and bool(torch.isfinite(inp.A[lo:hi]).all())
        assert bool(torch.isnan(inp.A_buf[:, c.M:]).all()) and bool(torch.isnan(inp.W_buf[:, c.N:]).all())
        out = torch.cat([inp.W[:lo], inp.W[hi:]]).double()
        assert bool(torch.isnan(out).all()) if fam == "poison" else bool((out == B.BF16_MAX).all())
    c = B.case("wgrad", "ring", 4, F32, 136, 0, kranges=B.TAP_KG, w_rows="taps", taps=9, tap_cols=64, family="poison")
    inp, lo, hi = B.inputs(c), c.offsets[0], c.offsets[-1]
    assert bool((inp.idx[:, :lo] == c.Rw - 1).all()) and bool(torch.isnan(inp.W[c.Rw - 1]).all()) and int(inp.idx[:, lo:hi].max()) < c.Rw - 1
    assert 0.1 < float((inp.idx[:, lo:hi] < 0).double().mean()) < 0.2 and c.tap_stride > c.K


@pytest.mark.parametrize("c", [c for c in DATA if c.family.startswith("poison")], ids=lambda c: c.tag.replace(" ", "_"))
def test_poison_reference_is_finite(c):
    ref, b = B.reference(c)
    assert bool(torch.isfinite(ref.C).all()) and bool(torch.isfinite(ref.S).all()) and bool(torch.isfinite(b).all())


# ------------------------------------------------------------------------------------------------------------------ (b) the bound has power
def standin(c):
    """A correct kernel's stand-in: an fp32 torch matmul on the CPU of the same operand values (gathered and masked as the descriptor says), rounded to
    bf16 for bf16 output.  [Z, M, N]."""
    inp = B.inputs(c)
    A = inp.A.float()
    parts = []
    if c.a_km:
        for kb, ke in c.ranges:
            parts.append(A[kb:ke, :c.M].t() @ B._w_rows_of(c, inp, kb, ke, None).float())
    else:
        W = inp.W.float() if c.layout == "dgrad" else inp.W.float()[None]
        seg = inp.seg.tolist() if c.counts else [0, c.M]
        ksz = c.K // c.split_k
        for z in range(c.split_k):
            parts.append(torch.cat([A[seg[e]:seg[e + 1], z * ksz:(z + 1) * ksz] @ W[e, z * ksz:(z + 1) * ksz, :c.N] for e in range(c.E)]))
    return torch.stack([B.to_out(p, c.out) for p in parts])


@pytest.mark.parametrize("layout", B.LAYOUTS, ids=lambda s: s.replace(" ", "_"))
def test_correct_standin_is_inside_the_bound_for_every_case(layout):
    worst = (0.0, None)
    for c in (c for c in UNIQUE if c.layout == layout):
        ref, b = B.reference(c)
        rs = B.part_ratios(standin(c), ref.C, b, ref.total)
        name, q, idx = max(rs, key=lambda r: r[1])
        assert q <= 1.0, f"{c.tag}: {name}{list(idx)} err / bound = {q:.3g}"
        if q > worst[0]:
            worst = (q, f"{c.tag} {name}")
    print(f"{layout}: worst err / bound of the stand-in {worst[0]:.3g} ({worst[1]})")


DEFECT_CASES = [(d, c) for d in B.DEFECTS for c in UNIQUE if B.applies(d, c)]


def test_every_defect_has_cases_on_every_kernel_it_can_touch():
    have = {(d, c.layout) for d, c in DEFECT_CASES}
    every = set(B.LAYOUTS)
    want = {"k_late": every, "k_drop_last": every, "k_past": {"dgrad", "wgrad", "f32 lay 1", "f32 lay 3"}, "prev_group": {"wgrad", "f32 lay 1", "f32 lay 3"},
            "neg_as_row0": {"wgrad"}, "tap0_table": {"wgrad"}, "tap_swap": {"wgrad"}, "slab_range": {"dgrad"}, "next_expert": {"dgrad"},
            "transposed": {"dgrad", "wgrad", "f32 lay 3"}, "lay1_as_3": {"f32 lay 1"}, "truncate": {"dgrad", "wgrad"}}
    assert set(want) == set(B.DEFECTS)
    for d, layouts in want.items():
        assert {(d, l) for l in layouts} <= have, d


@pytest.mark.parametrize("defect", B.DEFECTS)
def test_each_wrong_reference_leaves_the_bound_at_every_case_it_applies_to(defect):
    smallest, n = (float("inf"), None), 0
    for c in (c for d, c in DEFECT_CASES if d == defect):
        ref, b = B.reference(c)
        q = B.worst(B.part_ratios(B.wrong_reference(c, defect), ref.C, b))
        assert q > 1.0, f"a kernel with {defect} would pass {c.tag} (err / bound = {q:.3g})"
        n += 1
        if q < smallest[0]:
            smallest = (q, c.tag)
        if defect == "truncate":                                         # on a good part of the elements, not on one
            frac = float(((B.wrong_reference(c, defect) - ref.C).abs() > b).double().mean())
            assert frac > 0.2, (c.tag, frac)
    print(f"{defect}: {n} cases, smallest err / bound {smallest[0]:.3g} ({smallest[1]})")


# ------------------------------------------------------------------------------------------------------------------ (c) the kernel a case names
def test_every_case_is_taken_by_the_kernel_geometry_and_path_it_names():
    assert len(CASES) > 400
    for c in CASES:
        assert B.path_of(c) == (c.kernel, c.path), (c.tag, B.path_of(c))
    seen = {(c.kernel, c.layout, c.path, c.out) for c in CASES}
    for lay in ("dgrad", "wgrad"):
        for o in B.OUTS:
            assert {(k, lay, p, o) for k, p in [("ring", g) for g in B.RING_CFGS] + [("pptr", 6)]} <= seen
    assert {(c.layout, c.path) for c in CASES if c.kernel == "f32"} >= {(f"f32 lay {l}", p) for l in (1, 2, 3) for p in ("vec small", "scalar small")}
    assert {c.path for c in CASES if c.kernel == "f32"} == {"vec small", "scalar small", "vec 64", "scalar 64"}
    # the gaps the table is there to close: the two-pass epilogue (NS1, fp32 output), bf16-output weight gradients on the ring, 64-column taps re-routed
    assert any(c.path == 5 and c.out == F32 and c.layout == "wgrad" for c in CASES) and any(c.path == 5 and c.out == F32 and c.layout == "dgrad" for c in CASES)
    assert any(c.kernel == "ring" and c.layout == "wgrad" and c.out == BF16 and c.kranges for c in CASES)
    assert any(c.cfg in (1, 3, 5) and c.path == 4 and c.tap_cols == 64 for c in CASES)
    nine = B.nine_expert_case(F32)
    assert nine.E == 9 and not B.pptr_takes(nine) and B.pptr_takes(nine._replace(counts=nine.counts[:8])) and B.path_of(nine) == ("ring", 2)


def test_refused_descriptors_are_refused_by_the_predicates_too():
    d = B.case("dgrad", "ring", 1, F32, 129, 72, 128)
    w = B.case("wgrad", "ring", 1, F32, 136, 72, 65)
    assert B.tr_status(d) == B.tr_status(w) == B.OK
    for bad in (d._replace(N=76, pad=(8, 4, 8, 0)), w._replace(N=76, pad=(8, 4, 8, 0)), w._replace(M=132, pad=(4, 8, 8, 0)), d._replace(pad=(4, 8, 8, 0)), w._replace(pad=(4, 8, 8, 0)), d._replace(pad=(8, 8, 6, 0)),
                d._replace(out=BF16, pad=(8, 8, 4, 0)), d._replace(K=256, split_k=3), w._replace(split_k=2), d._replace(K=96)):
        assert B.tr_status(bad) == B.UNSUPPORTED, bad.tag
    assert B.tr_status(d, a_rows=True) == B.tr_status(w, a_rows=True) == B.UNSUPPORTED
    assert B.tr_status(w, expert_offsets=True) == B.UNSUPPORTED and B.tr_status(d, k_groups=True) == B.UNSUPPORTED
    assert B.tr_status(w, flags=B.A_KM) == B.BAD_ARG
    assert B.tr_status(w._replace(w_rows="taps", tap_cols=40, N=80)) == B.UNSUPPORTED
    f = B.case("f32 lay 2", "f32", 0, F32, 36, 52, 36)
    assert B.f32_status(f) == B.OK and B.f32_status(f._replace(K=35)) == B.UNSUPPORTED and B.f32_status(f._replace(pad=(8, 8, 8, 4))) == B.UNSUPPORTED
