"""mode_gemm's forward kernels at their edges, element by element against the fp64 reference and the derived bound of tests/gemm_refs.py (validated on the
CPU by tests/test_gemm_references.py): the ring kernel's geometries, the persistent ping-pong kernel, the weight streamer, the register-resident mid
kernel and the fp32 kernels.  Every launch goes through hip_helpers.gemm_into into NaN-prefilled outputs between canary rows, with leading dimensions
that differ from the logical widths (pad columns hold the canary too); after it, in this order: status 0, canaries intact, no NaN left inside the
logical output, the per-element bound.  Each test prints its worst err / bound per (path, epilogue, output) and the reference-alone gaps of its
GELU / SwiGLU cases (LABNOTES.md, "Forward GEMM family against fp64")."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import gemm_refs as R  # noqa: E402
import hip_helpers as H  # noqa: E402
from gemm_refs import BF16, F32, NONE, BIAS, BIAS_GELU, RESIDUAL, SWIGLU, RESIDUAL_NORM  # noqa: E402
from mode_diffusion_policy_amd import _lib as L  # noqa: E402

BAD_ARG, UNSUPPORTED = -1, -2


def dev(t):
    return None if t is None else t.to("cuda")


class Launched:
    """Status and outputs of one launch.  got: dict name -> CPU tensor of the logical output, as gemm_refs.ratios reads it."""

    def __init__(self, c, rc, outs, M):
        self.rc, self.outs = rc, outs
        self.intact = all(o.intact() for o in outs.values())
        self.got, self.gaps_untouched = {}, True
        for name, o in outs.items():
            t = (o.out if isinstance(o, H.GuardedCols) else o.t).cpu().contiguous()
            if name == "C" and c.split_k > 1:                            # slab z at z * split_stride = z * (M + 1) rows: one untouched row after each slab
                t = t.reshape(c.split_k, M + 1, c.N)
                self.gaps_untouched = bool(torch.isnan(t[:, M]).all())
                self.got["slab"] = t[:, :M]
            else:
                self.got[name] = t
        self.untouched = all(bool(torch.isnan(t).all()) for t in self.got.values()) and self.gaps_untouched
        self.nan_left = any(bool(torch.isnan(t).any()) for t in self.got.values())


def launch(c, inp=None, flags=None, rows=None):
    """One mode_gemm call for case `c` under its "gemm_cfg"; rows: launch the first `rows` rows only (ungrouped cases)."""
    inp = inp or R.inputs(c)
    lib = L.load()
    off, M = c.pad[3], rows or c.M
    A = dev(inp.A_buf)[:, off:off + c.K]
    W = dev(inp.W_buf)[:c.Nw, off:off + c.K]
    bias = dev(inp.bias) if c.epi in (BIAS, BIAS_GELU, SWIGLU) else None
    resid = dev(inp.resid_buf)[:, off:off + c.N] if c.epi in (RESIDUAL, RESIDUAL_NORM) else None
    outs = dict(C=H.GuardedCols(M if c.split_k == 1 else c.split_k * (M + 1), c.N, c.ldc, c.out, col0=c.c_off))
    if c.epi == RESIDUAL_NORM:
        outs["C2"] = H.GuardedCols(M, c.N, c.ldc2, BF16, col0=off)
        outs["row_ss_out"] = H.Guarded(M, c.N // c.group)
    a_rows, offsets, gain, row_ss = dev(inp.a_rows), dev(inp.offsets), dev(inp.gain), dev(inp.row_ss) if c.ss_n else None
    assert lib.mode_set_option(b"gemm_cfg", c.cfg) == 0
    try:
        rc = H.gemm_into(A, W, outs["C"], M, c.N, c.K, c.epi, bias=bias, resid=resid, a_rows=a_rows, offsets=offsets, num_experts=c.E if c.counts else 0,
                         w_estride=c.w_estride if c.counts else 0, b_estride=c.b_estride if c.counts else 0, split_k=c.split_k if c.split_k > 1 else 0,
                         split_stride=(M + 1) * c.ldc if c.split_k > 1 else 0, flags=c.flags if flags is None else flags, C2=outs.get("C2"),
                         gain=gain if c.epi == RESIDUAL_NORM else None, row_ss_out=outs.get("row_ss_out"), row_ss=row_ss, row_eps=inp.row_eps)
        torch.cuda.synchronize()
    finally:
        lib.mode_set_option(b"gemm_cfg", 0)
    return Launched(c, rc, outs, M)


def clamped_rows(c, inp):
    return [m for m in range(c.M) if (int(inp.a_rows[m]) if c.gather else m) in inp.clamped]


def check(rep, c):
    """Reference, gap and bound before the launch; then status, canaries, NaN, bound.  Returns the launch (None when it did not get to the bound)."""
    inp = R.inputs(c)
    ref, bound, gap = R.reference(c)
    if c.epi in (BIAS_GELU, SWIGLU):
        print(f"  {c.tag}: reference-alone gap {gap:.3g}")
    r = launch(c, inp)
    if r.rc != 0 or not r.intact or r.nan_left or not r.gaps_untouched:
        rep.fail(f"{c.tag}: status {r.rc}, canaries intact {r.intact}, NaN left {r.nan_left}, rows between slabs untouched {r.gaps_untouched}")
        return None
    rep.add(c, R.ratios(r.got, ref, bound, clamped_rows(c, inp)), gap)
    return r


def same_bits(a, b):
    return all(torch.equal(a.got[k].view(torch.int16) if a.got[k].dtype == BF16 else a.got[k], b.got[k].view(torch.int16) if b.got[k].dtype == BF16 else b.got[k])
               for k in a.got)


# ------------------------------------------------------------------------------------------------------------------ ring kernels
@pytest.mark.parametrize("cfg", R.RING_CFGS + (20,))
def test_ring_geometry(cfg):
    """Sweeps over M (1 .. 257 at N = 68), N (4 .. 260 at M = 65) and K (64: one K-step, the ring never wraps; 192) with every epilogue the geometry
    takes, fp32 and bf16 output, GELU and SwiGLU on the `soft` and the `tails` family."""
    rep = R.Report(f"ring {cfg}")
    for c in R.ring_cases(cfg):
        check(rep, c)
    rep.close()


@pytest.mark.parametrize("cfg", R.RING_CFGS + (20,))
def test_ring_grouped_and_gathered(cfg):
    """Four experts with segments (0, 1, 128, 129) and (130, 0, 0, 0), a gather in which every token serves two rows, weights three rows further apart
    than one matrix: the SwiGLU up-projection with row_ss by token (tails, and clamp rows checked row by row), a gathered BIAS GEMM at K = 64, and the
    down-projection in 2 and 4 bf16 K-slice slabs - each slab against its own K range, their sum against the whole product."""
    rep = R.Report(f"ring {cfg} grouped")
    for c in R.grouped_ring_cases(cfg):
        check(rep, c)
    rep.close()


def test_ring_geometries_agree_bit_for_bit():
    """The header's promise: every forward geometry produces the same bits.  One ragged shape per epilogue against geometry 1."""
    rep = R.Report("ring bit identity")
    for c in R.bit_identity_cases():
        first = check(rep, c)
        for cfg in R.other_geometries(c):
            if first is None:
                continue
            other = check(rep, c._replace(cfg=cfg))
            if other is not None and not same_bits(first, other):
                rep.fail(f"{c.tag}: geometry {cfg} differs from geometry 1")
    rep.close()


@pytest.mark.parametrize("cfg", (0,) + R.RING_CFGS)
def test_residual_norm_three_outputs(cfg):
    """MODE_EPI_RESIDUAL_NORM: C, the gain-scaled bf16 C2 and row_ss_out per 64-column group, each against fp64, with ldc, ldc2 and ldr all different from
    N.  cfg 0: the mid kernel at K = 1024 (M = 1 .. 100); else that ring geometry at N = 64, 128, 192."""
    rep = R.Report(f"residual_norm {cfg}")
    for c in R.residual_norm_cases(cfg):
        check(rep, c)
    rep.close()


# ------------------------------------------------------------------------------------------------------------------ streamer and mid kernel
@pytest.mark.parametrize("K", R.STREAM_K)
def test_streamer(K):
    """Automatic geometry, M = 1 .. 32 x N = 4 .. 132 (N % 8 == 4: the 8-byte tail) with every epilogue the streamer takes."""
    rep = R.Report(f"streamer K={K}")
    for c in R.stream_cases(K):
        check(rep, c)
    rep.close()


def test_streamer_small_rows():
    """MODE_GEMM_SMALL_ROWS: RESIDUAL_NORM with 16-column partials [M, N / 16]; SwiGLU with row_ss at row_ss_n = 3, 6, 18 and 70 (clamp rows row by row);
    grouped + gathered with segments (0, 1, 32, 5), also in two K-slices."""
    rep = R.Report("streamer small rows")
    for c in R.stream_small_rows_cases():
        check(rep, c)
    rep.close()


def test_mid_kernel():
    """NONE / BIAS at K = 1024, M = 33 .. 128; at M = 129 the ring takes over: inside the bound, and its first 128 rows are the bits the mid kernel
    writes for those rows alone (the same k-ordered chain, gemm_bf16_skinny.hip:386)."""
    rep = R.Report("mid")
    for c in R.mid_cases():
        check(rep, c)
    for out in (F32, BF16):
        c = R.mid_boundary_case(out)
        ring = check(rep, c)
        mid = launch(c, rows=128)
        if ring is None or mid.rc != 0 or not mid.intact or not torch.equal(ring.got["C"][:128].float(), mid.got["C"].float()):
            rep.fail(f"{c.tag}: the ring's first 128 rows are not the mid kernel's bits (status {mid.rc})")
    rep.close()


# ------------------------------------------------------------------------------------------------------------------ ping-pong kernel
@pytest.mark.parametrize("cfg", (17, 18))
def test_pingpong(cfg):
    """M one under, at and one over the tile's rows, N of one and two tiles, K = 128 and 256, two K-slices of 128, grouped segments of 0 / 1 / tile /
    tile + 1 rows with bias_expert_stride > N; on the 224-row tile SwiGLU (tails) and its gathered form with row_ss at row_ss_n = 4 and 16 (clamp rows)."""
    rep = R.Report(f"pingpong {cfg}")
    for c in R.pp_cases(cfg):
        check(rep, c)
    rep.close()


def test_pingpong_identity_rows_promise():
    """MODE_GEMM_IDENTITY_ROWS over an identity gather: the same bits as the launch that loads the indices."""
    rep = R.Report("pingpong identity rows")
    c = R.pp_identity_case()
    a = check(rep, c)
    b = launch(c, flags=R.UNIFORM_GROUPS)
    if a is None or b.rc != 0 or not b.intact or not same_bits(a, b):
        rep.fail(f"{c.tag}: differs from the launch without the promise (status {b.rc})")
    rep.close()


# ------------------------------------------------------------------------------------------------------------------ strides
def test_operands_as_column_slices():
    """A, W, C and resid 8 columns into wider buffers (lda = K + 64, ldw = K + 8, ldc = N + 8) on every kernel family; the pad columns keep their canary."""
    rep = R.Report("strides")
    for c in R.strided_cases():
        check(rep, c)
    rep.close()


# ------------------------------------------------------------------------------------------------------------------ fp32
@pytest.mark.parametrize("K", R.F32_K)
@pytest.mark.parametrize("flags", (0, R.SKINNY_OK))
def test_gemm_f32(flags, K):
    """gemm_f32.hip: the MFMA kernel, the dot kernel (N <= 16, K >= 64) and, under MODE_GEMM_SKINNY_OK, the GEMV (M <= 16), with K from 1, N from 1 and
    ldc = N + 3; the bound counts K + 3 roundings."""
    rep = R.Report(f"f32 flags={flags} K={K}")
    for c in R.f32_cases(flags, K):
        check(rep, c)
    rep.close()


# ------------------------------------------------------------------------------------------------------------------ refusals
def test_refusals_leave_the_outputs_untouched():
    """The contract's refusals return before any launch: their status, every output still NaN, every canary intact."""
    ok = R.case("ring", 1, NONE, F32, 65, 68, 128)
    rn = R.case("ring", 1, RESIDUAL_NORM, F32, 65, 64, 128)
    for c, status in ((ok._replace(K=96), UNSUPPORTED), (ok._replace(N=66), UNSUPPORTED), (ok._replace(pad=(4, 8, 8, 0)), UNSUPPORTED),
                      (ok._replace(epi=BIAS, split_k=2), UNSUPPORTED), (rn._replace(out=BF16), BAD_ARG),
                      (R.case("ring", 1, RESIDUAL_NORM, F32, 0, 64, 128, counts=(1, 64)), BAD_ARG), (ok._replace(epi=BIAS, ss_n=2), BAD_ARG),
                      (R.case("stream", 1, NONE, F32, 17, 20, 128, flags=R.SMALL_ROWS), UNSUPPORTED)):
        r = launch(c)
        assert r.rc == status and r.intact and r.untouched, (c.tag, r.rc, r.intact, r.untouched)
