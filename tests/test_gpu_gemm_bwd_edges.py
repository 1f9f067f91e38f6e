"""mode_gemm's backward-pass kernels at their edges, element by element against the fp64 reference and the derived bound of tests/gemm_bwd_refs.py
(validated on the CPU by tests/test_gemm_bwd_references.py): the ring kernel of gemm_bf16_tr.hip in its five geometries, the persistent ping-pong
kernel of gemm_bf16_pptr.hip and the fp32 layouts of gemm_f32.hip - data gradient (expert segments, K-slices) and weight gradient (K groups that start
above row 0 and end before the buffers do, gathered rows, taps).  Every launch goes through hip_helpers.gemm_into into one NaN-prefilled GuardedCols
buffer between canary rows that holds every part (K group or K-slice) with one spare row after each, with leading dimensions that differ from the
logical widths; after it, in this order: status 0, canaries intact, spare rows still NaN, no NaN inside the logical output, an empty group exactly
+0.0, the per-element bound.  Each test prints its worst err / bound per (kernel, layout, output) (LABNOTES.md, "Backward GEMM family against fp64")."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import gemm_bwd_refs as B  # noqa: E402
import hip_helpers as H  # noqa: E402
from gemm_bwd_refs import BF16, F32  # noqa: E402
from mode_diffusion_policy_amd import _lib as L  # noqa: E402


@pytest.fixture
def tr_cfg():
    """Sets "gemm_tr_cfg" (the option is process-wide) and puts the automatic choice back afterwards."""
    lib = L.load()

    def set_cfg(v):
        assert lib.mode_set_option(b"gemm_tr_cfg", v) == 0

    yield set_cfg
    lib.mode_set_option(b"gemm_tr_cfg", 0)


def dev(t):
    return None if t is None else t.to("cuda")


class Launched:
    """Status and output of one launch.  got [Z, M, N]: the parts, on the CPU."""

    def __init__(self, c, rc, out, parts):
        self.rc, self.intact = rc, out.intact()
        t = out.out.cpu().contiguous()
        if parts > 1:                                                    # part z at z * (M + 1) rows: one untouched row after each
            t = t.reshape(parts, c.M + 1, c.N)
            self.gaps_untouched = bool(torch.isnan(t[:, c.M]).all())
            self.got = t[:, :c.M]
        else:
            self.gaps_untouched, self.got = True, t[None]
        self.untouched = bool(torch.isnan(self.got).all()) and self.gaps_untouched
        self.nan_left = bool(torch.isnan(self.got).any())

    def bits(self):
        return self.got.contiguous().view(torch.int16 if self.got.dtype == BF16 else torch.int32)


def launch(c, set_cfg, inp=None, cfg=None, a_rows=None, expert_offsets=None, k_group_offsets=None, flags=None):
    """One mode_gemm call for case `c` under its "gemm_tr_cfg" (or `cfg`).  The keyword arguments put descriptor fields a Case cannot state (the
    refusals): an a_rows gather, expert_offsets on a weight gradient, k_group_offsets on a data gradient, other flags."""
    inp = inp or B.inputs(c)
    off = c.op_off
    A = dev(inp.A_buf)[:, off:off + c.a_cols]
    W = dev(inp.W_buf)[:, off:off + c.w_cols]
    assert inp.A_buf.shape[1] == c.lda and inp.W_buf.shape[1] == c.ldw
    parts = max(c.Z, c.split_k)
    out = H.GuardedCols(c.M if parts == 1 else parts * (c.M + 1), c.N, c.ldc, c.out, col0=c.c_off)
    i32 = lambda v: None if v is None else torch.tensor(v, dtype=torch.int32, device="cuda")
    seg = dev(inp.seg) if expert_offsets is None else expert_offsets
    koffs = i32(c.offsets) if k_group_offsets is None else k_group_offsets      # (the case's own: a case may borrow another's inputs)
    idx = dev(inp.idx)
    set_cfg(c.cfg if cfg is None else cfg)
    try:
        rc = H.gemm_into(A, W, out, c.M, c.N, c.K, L.EPI_NONE, a_rows=a_rows, offsets=seg, num_experts=0 if seg is None else seg.numel() - 1,
                         w_estride=c.w_estride if c.counts else 0, split_k=c.split_k if c.split_k > 1 else 0,
                         split_stride=c.part_stride if c.split_k > 1 else 0, flags=c.flags if flags is None else flags, lda=c.lda, ldw=c.ldw,
                         k_group_offsets=koffs, num_k_groups=0 if koffs is None else koffs.numel() - 1, c_group_stride=c.part_stride if koffs is not None else 0,
                         w_rows=idx, w_tap_cols=c.tap_cols, w_rows_tap_stride=c.tap_stride if c.tap_cols else 0)
        torch.cuda.synchronize()
    finally:
        set_cfg(0)
    return Launched(c, rc, out, parts)


def check(rep, c, set_cfg):
    """Reference and bound before the launch; then status, canaries, spare rows, NaN, empty groups, bound.  Returns the launch (None when it did not
    get to the bound)."""
    ref, bound = B.reference(c)
    r = launch(c, set_cfg)
    if r.rc != 0 or not r.intact or r.nan_left or not r.gaps_untouched:
        rep.fail(f"{c.tag}: status {r.rc}, canaries intact {r.intact}, NaN left {r.nan_left}, rows between parts untouched {r.gaps_untouched}")
        return None
    for z, k in enumerate(ref.k):
        if k == 0 and bool((r.bits()[z] != 0).any()):
            rep.fail(f"{c.tag}: the empty group {z} is not exactly +0.0")
    rep.add(c, B.part_ratios(r.got, ref.C, bound, ref.total))
    return r


def sweep(what, cases, set_cfg):
    rep = B.Report(what)
    for c in cases:
        check(rep, c, set_cfg)
    rep.close()


# ------------------------------------------------------------------------------------------------------------------ ring kernel
@pytest.mark.parametrize("cfg", B.RING_CFGS)
def test_ring_data_gradient(cfg, tr_cfg):
    """M = 1 .. 129 at N = 72, N = 8 .. 136 at M = 129, K = 64 / 128 / 192 (one and two K-steps: below the three-slot rings' prefetch depth), fp32 and
    bf16 output; four experts in segments (0, 1, 128, 129) and (130, 0, 0, 0) with weights three rows further apart than one matrix, also in 2 and 4
    K-slices - each slab against its own K range, their sum against the whole product; NaN in every pad column and between the experts' matrices."""
    sweep(f"ring {cfg} dgrad", B.ring_dgrad_cases(cfg), tr_cfg)


@pytest.mark.parametrize("cfg", B.RING_CFGS)
def test_ring_weight_gradient(cfg, tr_cfg):
    """M = 8 / 128 / 136, N = 8 .. 136, K = 1 .. 129 rows ungrouped; seven K groups of 0 .. 130 rows from row 67 to 5 rows before the end, with NaN
    (or NaN in A and the largest finite bf16 in W) in every row outside them; the same through a gathered index table with repeats and 15 % negative
    indices; taps of 64 (re-routed to the 64-wide two-slot ring), 128 and 192 columns, 1 / 4 / 9 of them; fp32 and bf16 output."""
    sweep(f"ring {cfg} wgrad", B.ring_wgrad_cases(cfg), tr_cfg)


# ------------------------------------------------------------------------------------------------------------------ ping-pong kernel
def test_pingpong(tr_cfg):
    """ "gemm_tr_cfg" 6.  Data gradient: M one under, at and one over the tile's 256 rows and M = 1, N of one and two tiles, K = 128 and 256, segments
    (0, 1, 256, 257) and (258, 0, 0, 0), two K-slices of 128, nine experts (declined: the ring runs them).  Weight gradient: K groups of
    (0, 1, 64, 65, 128, 129) rows from row 0 and from row 67 - the first group empty, every row outside the groups poisoned."""
    sweep("pingpong", B.pptr_cases(), tr_cfg)


def test_nine_experts_fall_back_to_the_ring(tr_cfg):
    """More than 8 experts under a forced "gemm_tr_cfg" 6: status 0, inside the bound, and the bits of the launch that never asks the ping-pong kernel."""
    rep = B.Report("nine experts")
    for o in B.OUTS:
        c = B.nine_expert_case(o)
        a = check(rep, c, tr_cfg)
        b = launch(c, tr_cfg, cfg=7)
        if a is None or b.rc != 0 or not b.intact or not torch.equal(a.bits(), b.bits()):
            rep.fail(f"{c.tag}: differs from the ring's own launch (status {b.rc})")
    rep.close()


# ------------------------------------------------------------------------------------------------------------------ fp32
def test_f32_layouts(tr_cfg):
    """gemm_f32.hip's layouts 1, 2, 3 at K = 1 .. 100 on shapes that take the float4 and the scalar global loads, K groups (100, 0, 71, 129) from row 7
    (layouts 1 and 3; poisoned outside), and the 64 x 64 tile reached by size (832 x 832, 830 x 830 at K = 5) and by the group count (256 x 256, 11 groups)."""
    sweep("f32", B.f32_cases(), tr_cfg)


def test_f32_paths_agree_bit_for_bit(tr_cfg):
    """An element's MFMA chain depends neither on the tile nor on how the operands were loaded: a group of the 11-group launch (64 x 64 tiles) equals
    the same range launched alone (32 x 32 tiles); the first 51 columns at N = 52 (float4 loads) equal the launch with N = 51 (scalar loads)."""
    big = B.f32_group_count_case()
    inp = B.inputs(big)
    all_groups = launch(big, tr_cfg, inp)
    assert all_groups.rc == 0 and all_groups.intact and B.f32_path(big) == "vec 64"
    for z in (2, 7, 10):
        kb, ke = big.ranges[z]
        one = big._replace(kranges=(kb, (ke - kb,), big.K - ke), path="vec small")
        assert one.K == big.K and B.path_of(one) == ("f32", "vec small")
        r = launch(one, tr_cfg, inp)
        assert r.rc == 0 and r.intact and not r.nan_left and torch.equal(r.bits()[0], all_groups.bits()[z]), z
    wide = B.case("f32 lay 3", "f32", 0, F32, 36, 52, 36)
    narrow = wide._replace(N=51)
    assert (B.f32_path(wide), B.f32_path(narrow)) == ("vec small", "scalar small") and narrow.ldw == wide.ldw
    a, b = launch(wide, tr_cfg), launch(narrow, tr_cfg, B.inputs(wide))
    assert a.rc == b.rc == 0 and a.intact and b.intact and not b.nan_left and torch.equal(a.bits()[:, :, :51], b.bits())


# ------------------------------------------------------------------------------------------------------------------ strides, bit identity
def test_operands_as_column_slices(tr_cfg):
    """lda = cols + 64 and A, W, C 16 bytes into their buffers on every kernel, with poisoned pad columns and poisoned rows outside the K groups."""
    sweep("strides", B.strided_cases(), tr_cfg)


@pytest.mark.parametrize("out", B.OUTS, ids=("f32", "bf16"))
def test_geometries_agree_bit_for_bit(out, tr_cfg):
    """The same k-ordered fp32 MFMA chain everywhere: ring geometries 2 .. 5 equal geometry 1, and the ping-pong kernel ("gemm_tr_cfg" 6) equals the ring
    ("gemm_tr_cfg" 7), at one data-gradient and one weight-gradient shape."""
    rep = B.Report("bit identity")
    ring_d, ring_w, pp_d, pp_w = B.bit_identity_cases(out)
    for c in (ring_d, ring_w):
        first = check(rep, c, tr_cfg)
        for g in B.RING_CFGS[1:]:
            other = check(rep, c._replace(cfg=g, path=g), tr_cfg)
            if first is None or other is None or not torch.equal(first.bits(), other.bits()):
                rep.fail(f"{c.tag}: geometry {g} differs from geometry 1")
    for c in (pp_d, pp_w):
        assert B.path_of(c) == ("pptr", 6)
        a = check(rep, c, tr_cfg)
        b = launch(c, tr_cfg, cfg=7)
        if a is None or b.rc != 0 or not b.intact or not torch.equal(a.bits(), b.bits()):
            rep.fail(f"{c.tag}: the ping-pong kernel differs from the ring (status {b.rc})")
    rep.close()


# ------------------------------------------------------------------------------------------------------------------ refusals
def test_refusals_leave_the_outputs_untouched(tr_cfg):
    """The contract's refusals return before any launch: their status, every output still NaN, every canary intact."""
    d = B.case("dgrad", "ring", 1, F32, 129, 72, 128)
    w = B.case("wgrad", "ring", 1, F32, 136, 72, 65)
    f = B.case("f32 lay 2", "f32", 0, F32, 36, 52, 36)
    i32 = lambda *v: torch.tensor(v, dtype=torch.int32, device="cuda")
    rows_d, rows_w = torch.arange(d.M, dtype=torch.int32, device="cuda"), torch.arange(w.K, dtype=torch.int32, device="cuda")
    table = ((d._replace(N=76, pad=(8, 4, 8, 0)), {}, B.UNSUPPORTED), (w._replace(N=76, pad=(8, 4, 8, 0)), {}, B.UNSUPPORTED),      # N % 8 (ldw = 80)
             (w._replace(M=132, pad=(4, 8, 8, 0)), {}, B.UNSUPPORTED),                                          # M % 8, weight gradient (lda = 136)
             (d._replace(pad=(4, 8, 8, 0)), {}, B.UNSUPPORTED), (w._replace(pad=(4, 8, 8, 0)), {}, B.UNSUPPORTED),    # lda % 8
             (d._replace(pad=(8, 8, 6, 0)), {}, B.UNSUPPORTED), (d._replace(out=BF16, pad=(8, 8, 4, 0)), {}, B.UNSUPPORTED),   # ldc % 4 / % 8
             (d, dict(a_rows=rows_d), B.UNSUPPORTED), (w, dict(a_rows=rows_w), B.UNSUPPORTED),                  # a_rows on the backward layouts
             (w, dict(expert_offsets=i32(0, w.M)), B.UNSUPPORTED),                                              # expert_offsets with A_KM
             (d, dict(k_group_offsets=i32(0, d.K)), B.UNSUPPORTED),                                             # k_group_offsets with the data gradient
             (d._replace(K=256, split_k=3), {}, B.UNSUPPORTED), (w._replace(split_k=2), {}, B.UNSUPPORTED),     # K % (64 split_k); K-slices of a weight gradient
             (d._replace(K=96), {}, B.UNSUPPORTED),                                                             # K % 64, data gradient
             (w, dict(flags=B.A_KM), B.BAD_ARG),                                                                # bf16 A_KM without W_KN
             (w._replace(w_rows="taps", taps=2, tap_cols=40, N=80), {}, B.UNSUPPORTED),                         # taps of 40 columns
             (f._replace(K=34), {}, B.UNSUPPORTED))                                                             # fp32 [M, K] rows that are no multiple of 16 bytes
    for c, over, status in table:
        for cfg in (1, 6):
            r = launch(c._replace(cfg=cfg), tr_cfg, **over)
            assert r.rc == status and r.intact and r.untouched, (c.tag, over.keys(), cfg, r.rc, r.intact, r.untouched)
        if not over and c.dtype == BF16:
            assert B.tr_status(c) == status, c.tag


# ------------------------------------------------------------------------------------------------------------------ sensitivity
SHORTLIST = {
    "ring": (B.case("dgrad", "ring", 1, BF16, 128, 128, 128), B.case("dgrad", "ring", 3, BF16, 0, 72, 256, counts=(0, 1, 128, 129), wextra=3, split_k=2),
             B.case("dgrad", "ring", 2, F32, 0, 72, 128, family="spiky", counts=(0, 1, 128, 129), wextra=3),
             B.case("wgrad", "ring", 5, BF16, 136, 72, kranges=B.RING_KG), B.case("wgrad", "ring", 1, F32, 136, 136, 65),
             B.case("wgrad", "ring", 4, F32, 136, 72, kranges=B.RING_KG, family="spiky", w_rows="gathered", path=4),
             B.case("wgrad", "ring", 1, F32, 136, 0, kranges=B.TAP_KG, w_rows="taps", taps=9, tap_cols=64, family="poison", path=4)),
    "pptr": (B.case("dgrad", "pptr", 6, BF16, 256, 256, 128), B.case("dgrad", "pptr", 6, F32, 257, 256, 256, split_k=2),
             B.case("dgrad", "pptr", 6, F32, 0, 256, 128, counts=(0, 1, 256, 257), wextra=3),
             B.case("wgrad", "pptr", 6, BF16, 256, 256, kranges=(67, B.PPTR_KG, 5), family="spiky")),
    "f32": (B.case("f32 lay 3", "f32", 0, F32, 36, 52, kranges=B.F32_KG, path="vec small"), B.case("f32 lay 1", "f32", 0, F32, 70, 36, 36, path="scalar small"),
            B.case("f32 lay 2", "f32", 0, F32, 36, 52, 36, path="vec small"), B.f32_group_count_case()),
}
ONLY = {"neg_as_row0": ("ring",), "tap0_table": ("ring",), "tap_swap": ("ring",), "slab_range": ("ring", "pptr"), "next_expert": ("ring", "pptr"),
        "lay1_as_3": ("f32",), "truncate": ("ring", "pptr"), "k_past": ("ring", "pptr", "f32")}


def test_the_kernels_miss_every_wrong_reference(tr_cfg):
    """For each wrong reading of the descriptor (tests/test_gemm_bwd_references.py), at one shape per kernel it can be stated for: the kernel's output
    lies inside the bound of the right reference and misses the wrong one by more than the bound."""
    runs, rep = {}, B.Report("sensitivity")
    for defect in B.DEFECTS:
        for kernel in ONLY.get(defect, ("ring", "pptr", "f32")):
            c = next((c for c in SHORTLIST[kernel] if B.applies(defect, c)), None)
            assert c is not None and B.path_of(c) == (c.kernel, c.path), (defect, kernel)
            if c not in runs:
                runs[c] = check(rep, c, tr_cfg)
            if runs[c] is None:
                continue
            ref, bound = B.reference(c)
            q = B.worst(B.part_ratios(runs[c].got, B.wrong_reference(c, defect), bound))
            print(f"sensitivity | {defect} on {kernel}: the kernel misses the wrong reference by {q:.3g} x the bound ({c.tag})")
            if not q > 1.0:
                rep.fail(f"{c.tag}: the kernel's output is inside the bound of the reference with {defect}")
    rep.close()
