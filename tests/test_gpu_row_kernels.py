"""The row kernels of csrc/rowops.hip launched alone, through ctypes, against the fp64 restatements of tests/row_refs.py: both forms of the MoE
combine (one workgroup per row / one wave per row) on the same inputs, the shapes only the one-wave-per-row fallbacks take (combine, head), and the
options of the head / embed row kernels and of rmsnorm, ddim_edm_step and sigma_embed that no other test sets.

Every output is NaN-prefilled between canary rows that must survive the launch (hip_helpers.Guarded); hip_helpers.launch_guard asserts the kernels'
contract on the host before each launch (D % 4 == 0, 16-byte aligned operands, pos inside the sorted rows).

Bounds: fp32 row outputs (x_next, fp32 h, rmsnorm) rel-L2 < 1e-6; bf16 copies < 4e-3 (one bf16 rounding, 2^-8); head outputs ||got - ref|| <= 1e-5 ||ref||
per tensor and x_next at 3x that (tests/test_gpu_guidance.py); other fp32 kernels < 1e-5.

Each family also turns its reference wrong on the CPU (last slab dropped, two expert slots' weights swapped) and requires the kernel's output to MISS
that reference by more than the bound: the comparison would see such a kernel."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

from mode_diffusion_policy_amd import _lib as L  # noqa: E402

import hip_helpers as H  # noqa: E402
import row_refs as R  # noqa: E402
from row_refs import nrm, rel  # noqa: E402

F32, LP, HEAD = 1e-6, 4e-3, 1e-5
ROW_MAX_DEFAULT = 0x7fffffff
N = 9                                    # token rows of the combine cases: the one-wave-per-row form's last workgroup (4 rows each) holds one row
TDT = {"bf16": torch.bfloat16, "fp32": torch.float32}


def rnd(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def cu(t):
    return None if t is None else t.cuda().contiguous()


def combine_inputs(D, k, S, ydt, nss, rpc, n=N, seed=0):
    """CPU tensors of one combine case (Y already rounded to its dtype); nss = partials per row of the fused ln_2 (0: u arrives normalised)."""
    NK = n * k
    d = dict(u=rnd(n, D, seed=seed + 1), Y=rnd(S, NK, D, seed=seed + 2, scale=0.5).to(TDT[ydt]),
             pos=torch.randperm(NK, generator=torch.Generator().manual_seed(seed + 3)).to(torch.int32).view(n, k),
             posw=0.2 + rnd(n, k, seed=seed + 4).abs(), g=1.0 + 0.1 * rnd(D, seed=seed + 5),
             cond=rnd(-(-n // rpc), D, seed=seed + 6) if rpc else None, u_ss=None, u_gain=None)
    if nss:
        d["u_ss"], d["u_gain"] = R.partial_ss(d["u"], nss), 1.0 + 0.2 * rnd(D, seed=seed + 7)
    return d


def run_combine(d, rpc, hdt, row_max, want_x=True, want_h=True):
    """One launch with "combine_row_max" = row_max (restored afterwards).  Returns (x_next, h) on the CPU, either None when not asked for."""
    lib = L.load()
    n, D = d["u"].shape
    g_ = {k_: cu(v) for k_, v in d.items()}
    xn = H.Guarded(n, D) if want_x else None
    h = H.Guarded(n, D, TDT[hdt]) if want_h else None
    assert lib.mode_set_option(b"combine_row_max", row_max) == 0
    try:
        rc = H.combine_fused(g_["u"], g_["Y"], g_["pos"], g_["posw"], g_["g"], g_["cond"], max(rpc, 1), xn, h, g_["u_ss"], g_["u_gain"])
        torch.cuda.synchronize()
    finally:
        lib.mode_set_option(b"combine_row_max", ROW_MAX_DEFAULT)
    assert rc == 0, rc
    assert (xn is None or xn.intact()) and (h is None or h.intact()), "canary rows overwritten"
    return (xn.t.cpu() if xn else None), (h.t.float().cpu() if h else None)


def check_combine(d, rpc, hdt, got, what):
    """got = (x_next, h) against fp64; prints each figure before asserting."""
    xr, hr = R.combine(d["u"], d["Y"].float(), d["pos"], d["posw"], d["g"], d["cond"], max(rpc, 1), u_ss=d["u_ss"], u_gain=d["u_gain"])
    ex = rel(got[0], xr) if got[0] is not None else 0.0
    eh = rel(got[1], hr) if got[1] is not None else 0.0
    print(f"combine {what}: x_next {ex:.2e} (< {F32:.0e}), h[{hdt}] {eh:.2e} (< {F32 if hdt == 'fp32' else LP:.0e})")
    assert ex < F32 and eh < (F32 if hdt == "fp32" else LP), (what, ex, eh)
    return xr, hr


def check_combine_sensitivity(d, rpc, got_x, what):
    """The wrong references: without the last slab, with the weights of two expert slots swapped.  The kernel's x_next must miss both."""
    S, k = d["Y"].shape[0], d["pos"].shape[1]
    kw = dict(u_ss=d["u_ss"], u_gain=d["u_gain"])
    if S > 1:
        bad, _ = R.combine(d["u"], d["Y"][:-1].float(), d["pos"], d["posw"], **kw)
        assert rel(got_x, bad) > 100 * F32, (what, "a dropped slab would pass")
    if k > 1:
        bad, _ = R.combine(d["u"], d["Y"].float(), d["pos"], d["posw"].flip(1), **kw)
        assert rel(got_x, bad) > 100 * F32, (what, "swapped slot weights would pass")


# ================================================================================================================== a. combine, both forms
#          D    k  S  Y dtype  partials per row   rows_per_cond (0: cond = NULL)
CASES_A = [(68, 1, 1, "fp32", 0, 0),
           (256, 2, 3, "bf16", 16, 3),             # D/16 = 16 partials: the serial partial sum; 3 slabs under the bound 4 (masked slab)
           (272, 2, 1, "bf16", 17, 3),             # D/16 = 17: the wave partial sum
           (512, 2, 5, "fp32", 0, 3),              # 5 slabs under the bound 8
           (1280, 2, 8, "bf16", 20, 4),            # NC = 2, a quarter-filled second chunk; D/64 partials
           (2048, 1, 2, "bf16", 0, 3),
           (3076, 2, 4, "fp32", 769, 3),           # NC = 4, a 4-column fourth chunk; one partial per 4 columns
           (4096, 2, 1, "bf16", 64, 3)]


@pytest.mark.parametrize("hdt", ["bf16", "fp32"])
@pytest.mark.parametrize("D,k,S,ydt,nss,rpc", CASES_A)
def test_combine_both_forms(D, k, S, ydt, nss, rpc, hdt):
    """mode_moe_combine_norm_fused_fwd on 9 rows with "combine_row_max" at its default (one workgroup per row) and at 0 (one wave per row): each
    against fp64, and against each other at the fp32 bound (their reduction orders differ: no bit equality asked)."""
    d = combine_inputs(D, k, S, ydt, nss, rpc, seed=D)
    what = (D, k, S, ydt, nss, rpc, hdt)
    row = run_combine(d, rpc, hdt, ROW_MAX_DEFAULT)
    wave = run_combine(d, rpc, hdt, 0)
    check_combine(d, rpc, hdt, row, f"{what} row")
    check_combine(d, rpc, hdt, wave, f"{what} wave")
    ex, eh = rel(row[0], wave[0]), rel(row[1], wave[1])
    print(f"combine {what}: row vs wave x_next {ex:.2e} h {eh:.2e}")
    assert ex < F32 and eh < (F32 if hdt == "fp32" else LP), (what, ex, eh)
    check_combine_sensitivity(d, rpc, row[0], what)
    check_combine_sensitivity(d, rpc, wave[0], what)


@pytest.mark.parametrize("row_max", [ROW_MAX_DEFAULT, 0])
def test_combine_null_outputs(row_max):
    """h == NULL (only x_next is written; g may then be NULL too) and x_next == NULL (only h), D = 512 with 5 fp32 slabs, both forms."""
    D, k, S, ydt, nss, rpc = CASES_A[3]
    d = combine_inputs(D, k, S, ydt, nss, rpc, seed=77)
    x_only = run_combine(dict(d, g=None, cond=None), rpc, "bf16", row_max, want_h=False)
    h_only = run_combine(d, rpc, "bf16", row_max, want_x=False)
    check_combine(d, rpc, "bf16", (x_only[0], h_only[1]), f"null outputs row_max={row_max}")


# ================================================================================================================== b. fallback-only shapes
@pytest.mark.parametrize("k,S,row_max", [(3, 1, ROW_MAX_DEFAULT), (3, 2, ROW_MAX_DEFAULT), (8, 1, ROW_MAX_DEFAULT), (8, 2, ROW_MAX_DEFAULT),
                                         (2, 9, ROW_MAX_DEFAULT), (2, 1, 0), (2, 2, 0)])
@pytest.mark.parametrize("D,nss", [(256, 4), (1024, 16), (1284, 107)])
def test_combine_one_wave_per_row_only(D, nss, k, S, row_max):
    """top_k in {3, 8} and 9 slabs reach the one-wave-per-row kernel whatever the option says; k = 2 with 1 / 2 slabs and fused ln_2 is sent there by the
    option, for its unrolled slab loop (YS = 1, 2).  D = 256 / 1024 are its unrolled-chunk forms (NCH = 1, 4), 1284 the generic loop.  Fused and not,
    Y and h in both dtypes."""
    for fused in ((True,) if row_max == 0 else (False, True)):      # (the unrolled slab loop exists in the fused kernel only)
        for ydt, hdt in (("bf16", "fp32"), ("fp32", "bf16")):
            d = combine_inputs(D, k, S, ydt, nss if fused else 0, 3, seed=D + 10 * k + S)
            what = (D, k, S, fused, ydt, hdt)
            got = run_combine(d, 3, hdt, row_max)
            check_combine(d, 3, hdt, got, what)
            check_combine_sensitivity(d, 3, got[0], what)


# ================================================================================================================== c. head
B_H, A_LEN_H, T_H = 3, 3, 7
SCAL = [[0.4, 0.8, 0.6, 0.35], [0.1, 1.1, 0.2, 0.0], [0.9, 0.3, 0.5, 1.5]]       # {c_skip, c_out, r, c}; the second row's c == 0: the DDIM update


def head_inputs(D, A_dim, k, S, ydt, nss, B=B_H, A_len=A_LEN_H, T=T_H, seed=0):
    d = combine_inputs(D, k, S, ydt, nss, 0, n=B * T, seed=seed)
    d.pop("cond")
    sh = (B, A_len, A_dim)
    d.update(w_out=rnd(A_dim, D, seed=seed + 13, scale=D ** -0.5), b_out=rnd(A_dim, seed=seed + 14, scale=0.1), x_a=rnd(*sh, seed=seed + 15, scale=3.0),
             den_prev=rnd(*sh, seed=seed + 16), aux1=rnd(*sh, seed=seed + 17), aux2=rnd(*sh, seed=seed + 18), lin=torch.tensor([0.3, -0.7, 1.2, 0.5]),
             scal=torch.tensor(SCAL)[:B].contiguous())
    return d


def run_head(d, form, scal_stride, B=B_H, A_len=A_LEN_H, T=T_H, with_scal=True):
    """One mode_head_ddim_fwd launch.  form: "ddim" | "den_prev" | "lin".  Returns the Guarded outputs (F, denoised, x_next) and the device inputs."""
    lib = L.load()
    A_dim = d["w_out"].shape[0]
    g_ = {k_: cu(v) for k_, v in d.items()}
    rows = B * A_len
    out = {"F": H.Guarded(rows, A_dim)}
    if with_scal:
        out["denoised"] = H.Guarded(rows, A_dim)
        out["x_next"] = H.Guarded(rows, A_dim)
    upd = {"den_prev": dict(den_prev=g_["den_prev"]), "lin": dict(lin=g_["lin"], aux1=g_["aux1"], aux2=g_["aux2"]), "ddim": {}}[form] if with_scal else {}
    scal = (g_["scal"] if scal_stride else g_["scal"][:1].contiguous()) if with_scal else None
    desc = H.head_desc(g_["u"], g_["Y"], g_["pos"], g_["posw"], g_["g"], g_["w_out"], g_["b_out"], B, T, A_len, u_ss=g_["u_ss"], u_gain=g_["u_gain"],
                       x_a=g_["x_a"] if with_scal else None, scal=scal, scal_stride=scal_stride if with_scal else 0,
                       **{k_: v.t for k_, v in out.items()}, **upd)
    rc = lib.mode_head_ddim_fwd(C.byref(desc), H.stream())
    torch.cuda.synchronize()
    assert rc == 0, rc
    assert all(v.intact() for v in out.values()), "canary rows overwritten"
    return out, g_


def head_ref(d, form, scal_stride, B=B_H, A_len=A_LEN_H, T=T_H, with_scal=True, **over):
    upd = {"den_prev": dict(den_prev=d["den_prev"]), "lin": dict(lin=d["lin"], aux1=d["aux1"], aux2=d["aux2"]), "ddim": {}}[form]
    kw = dict(u=d["u"], Y=d["Y"].float(), pos=d["pos"], posw=d["posw"])
    kw.update(over)
    return R.head(kw["u"], kw["Y"], kw["pos"], kw["posw"], d["g"], d["w_out"], d["b_out"], B, T, A_len, u_ss=d["u_ss"], u_gain=d["u_gain"],
                  x_a=d["x_a"] if with_scal else None, scal=(d["scal"] if scal_stride else d["scal"][:1]) if with_scal else None, **(upd if with_scal else {}))


def check_head(out, ref, what):
    A_dim = out["F"].t.shape[1]
    errs = []
    for name, r, mult in (("F", ref[0], 1), ("denoised", ref[1], 1), ("x_next", ref[2], 3)):
        if name in out:
            r = r.reshape(-1, A_dim)
            tol = mult * HEAD * nrm(r)                                    # x_next: 3x, as in test_guided_head_kernel
            e = nrm(out[name].t.double().cpu() - r)
            errs.append((name, e, tol))
    print(f"head {what}: " + ", ".join(f"{n_} {e:.2e} (<= {t:.2e})" for n_, e, t in errs))
    for n_, e, t in errs:
        assert e <= t, (what, n_, e, t)


HEAD_FORMS = [("bf16", True, 4, "ddim"), ("fp32", False, 0, "den_prev"), ("bf16", False, 4, "lin"), ("fp32", True, 0, "ddim"),
              ("bf16", True, 4, "den_prev"), ("fp32", False, 4, "lin")]


@pytest.mark.parametrize("k,S", [(3, 1), (3, 4), (2, 9)])
@pytest.mark.parametrize("A_dim", [7, 14])
@pytest.mark.parametrize("D,nss", [(256, 4), (1024, 16), (1284, 107)])
def test_head_one_wave_per_row(D, nss, A_dim, k, S):
    """mode_head_ddim_fwd where only head_ddim_kernel takes the shape (k = 3; 9 slabs: its run-time slab loop): 3 samples x 3 action rows of T = 7,
    A_dim 7 / 14 (AMAX 8 / 32), D = 1024 its unrolled form.  Y dtype, fused ln_2, per-sample / shared scalings and the three update forms are spread
    over six launches per case."""
    for ydt, fused, scal_stride, form in HEAD_FORMS:
        d = head_inputs(D, A_dim, k, S, ydt, nss if fused else 0, seed=D + A_dim + 10 * k + S)
        what = (D, A_dim, k, S, ydt, fused, scal_stride, form)
        out, _ = run_head(d, form, scal_stride)
        check_head(out, head_ref(d, form, scal_stride), what)
        if S > 1:                                                        # the wrong references: the kernel's F must miss them
            bad = head_ref(d, form, scal_stride, Y=d["Y"][:-1].float())[0].reshape(-1, A_dim)
            assert nrm(out["F"].t.double().cpu() - bad) > 100 * HEAD * nrm(bad), (what, "a dropped slab would pass")
        bad = head_ref(d, form, scal_stride, posw=d["posw"].flip(1))[0].reshape(-1, A_dim)
        assert nrm(out["F"].t.double().cpu() - bad) > 100 * HEAD * nrm(bad), (what, "swapped slot weights would pass")


def test_head_row_form_options():
    """The one-workgroup-per-row head (k = 2, D = 256) where test_guided_head_kernel does not go: scal == NULL (F alone), x_next aliasing x_a (the bits
    of a run into a separate buffer), A_len = 1, A_dim in {1, 32}."""
    D, k, S = 256, 2, 2
    for A_dim, A_len in ((7, 3), (1, 3), (32, 3), (7, 1), (32, 1)):
        T = 1 + 1 + 2 + A_len
        d = head_inputs(D, A_dim, k, S, "bf16", 4, A_len=A_len, T=T, seed=A_dim + A_len)
        what = (A_dim, A_len)
        out, _ = run_head(d, "ddim", 4, A_len=A_len, T=T, with_scal=False)                       # scal == NULL: F alone
        assert set(out) == {"F"}
        check_head(out, head_ref(d, "ddim", 4, A_len=A_len, T=T, with_scal=False), (what, "F alone"))
        for form in ("ddim", "den_prev", "lin"):
            sep, _ = run_head(d, form, 4, A_len=A_len, T=T)
            check_head(sep, head_ref(d, form, 4, A_len=A_len, T=T), (what, form))
            xa = H.Guarded(B_H * A_len, A_dim)                                                      # x_next aliases x_a
            xa.t.copy_(d["x_a"].reshape(-1, A_dim))
            lib = L.load()
            g_ = {k_: cu(v) for k_, v in d.items()}
            upd = {"den_prev": dict(den_prev=g_["den_prev"]), "lin": dict(lin=g_["lin"], aux1=g_["aux1"], aux2=g_["aux2"]), "ddim": {}}[form]
            desc = H.head_desc(g_["u"], g_["Y"], g_["pos"], g_["posw"], g_["g"], g_["w_out"], g_["b_out"], B_H, T, A_len, u_ss=g_["u_ss"],
                               u_gain=g_["u_gain"], x_a=xa.t, scal=g_["scal"], scal_stride=4, x_next=xa.t, **upd)
            assert lib.mode_head_ddim_fwd(C.byref(desc), H.stream()) == 0
            torch.cuda.synchronize()
            assert xa.intact() and torch.equal(xa.t, sep["x_next"].t), (what, form, "aliased x_next differs")


# ================================================================================================================== d. embed, row form
@pytest.mark.parametrize("D", [68, 1024, 4096])
@pytest.mark.parametrize("A_len", [1, 16])
@pytest.mark.parametrize("A_dim", [1, 8, 9, 32])
def test_embed_row_form_options(A_dim, A_len, D):
    """mode_embed_tokens_fwd (one workgroup per row, B = 2) with the options test_guided_embed_kernel fixes: first without the sigma token, one image
    token, c_in == NULL and cond == NULL (bf16 h); then with the sigma token and the conditioning row shared by the batch (row strides 0) and one shared
    c_in scalar (c_in_stride 0), two image tokens (fp32 h)."""
    lib, B = L.load(), 2
    act, w_act = rnd(B, A_len, A_dim, seed=4, scale=2.0), rnd(D, A_dim, seed=6, scale=0.3)
    pos, g, goal_e = rnd(1 + A_len, D, seed=7, scale=0.2), 1.0 + 0.1 * rnd(D, seed=8), rnd(B, D, seed=2)
    for noise, n_img, hdt in ((0, 1, "bf16"), (1, 2, "fp32")):
        T = noise + 1 + n_img + A_len
        img_e = rnd(B, n_img, D, seed=3)
        emb_t, c_in, cond = (rnd(1, D, seed=1), 0.1 + rnd(1, seed=5).abs(), rnd(1, D, seed=9)) if noise else (None, None, None)
        dv = [cu(t) for t in (emb_t, goal_e, img_e, act, c_in, w_act, pos, g, cond)]
        x, h = H.Guarded(B * T, D), H.Guarded(B * T, D, TDT[hdt])
        H.launch_guard(D, *dv, x.t, h.t)
        desc = L.ModeEmbedDesc(B=B, T=T, D=D, A_len=A_len, A_dim=A_dim, n_img=n_img, use_noise_token=noise, emb_t=H.p(dv[0]), emb_row_stride=0,
                               goal_e=H.p(dv[1]), img_e=H.p(dv[2]), actions=H.p(dv[3]), c_in=H.p(dv[4]), c_in_stride=0, w_act=H.p(dv[5]), pos=H.p(dv[6]),
                               g=H.p(dv[7]), cond=H.p(dv[8]), cond_row_stride=0, eps=1e-6, x=H.p(x.t), h=H.p(h.t), h_dtype=H.dt_of(h.t))
        rc = lib.mode_embed_tokens_fwd(C.byref(desc), H.stream())
        torch.cuda.synchronize()
        assert rc == 0 and x.intact() and h.intact(), rc
        xr, hr = R.embed(goal_e, img_e, act, w_act, pos, g, emb_t=emb_t, c_in=c_in, cond=cond)
        ex, eh = rel(x.t, xr.reshape(-1, D)), rel(h.t.float(), hr.reshape(-1, D))
        print(f"embed A_dim={A_dim} A_len={A_len} D={D} noise={noise}: x {ex:.2e} (< {F32:.0e}), h[{hdt}] {eh:.2e}")
        assert ex < F32 and eh < (F32 if hdt == "fp32" else LP), (A_dim, A_len, D, noise, ex, eh)


# ================================================================================================================== e. rmsnorm
@pytest.mark.parametrize("rows", [1, 5])
@pytest.mark.parametrize("D", [4, 68, 512, 1284])
def test_rmsnorm_cond_options(D, rows):
    """mode_rmsnorm_cond_fwd: both outputs; y_f32 == NULL (the low-precision copy alone); an fp32 "low-precision" copy; y_lp == NULL; one conditioning
    row for all rows (rows_per_cond > rows); no conditioning."""
    lib = L.load()
    x, g = rnd(rows, D, seed=D + rows), 1.0 + 0.1 * rnd(D, seed=2)
    for want32, lpdt, rpc in ((True, "bf16", 2), (False, "bf16", 8), (False, "fp32", 1), (True, None, 8), (True, "fp32", 0)):
        cond = rnd(-(-rows // rpc), D, seed=3) if rpc else None
        xd, gd, cd = cu(x), cu(g), cu(cond)
        y32 = H.Guarded(rows, D) if want32 else None
        ylp = H.Guarded(rows, D, TDT[lpdt]) if lpdt else None
        H.launch_guard(D, xd, gd, cd, y32 and y32.t, ylp and ylp.t)
        rc = lib.mode_rmsnorm_cond_fwd(H.p(xd), H.p(gd), H.p(cd), rows, D, max(rpc, 1), 1e-6, H.p(y32 and y32.t), H.p(ylp and ylp.t),
                                       L.MODE_BF16 if lpdt == "bf16" else L.MODE_F32, H.stream())
        torch.cuda.synchronize()
        assert rc == 0 and (y32 is None or y32.intact()) and (ylp is None or ylp.intact()), rc
        ref = R.rmsnorm_cond(x, g, cond, max(rpc, 1))
        e32 = rel(y32.t, ref) if y32 else 0.0
        elp = rel(ylp.t.float(), ref) if ylp else 0.0
        print(f"rmsnorm D={D} rows={rows} f32={want32} lp={lpdt} rpc={rpc}: y_f32 {e32:.2e} y_lp {elp:.2e}")
        assert e32 < F32 and elp < (LP if lpdt == "bf16" else F32), (D, rows, want32, lpdt, rpc, e32, elp)


# ================================================================================================================== f. ddim_edm_step, sigma_embed
@pytest.mark.parametrize("scal_stride", [0, 4])
@pytest.mark.parametrize("per_sample", [7, 300])
@pytest.mark.parametrize("B", [1, 5])
def test_ddim_edm_step(B, per_sample, scal_stride):
    lib = L.load()
    Fh, xa = rnd(B, per_sample, seed=B), rnd(B, per_sample, seed=per_sample, scale=3.0)
    scal = torch.cat([torch.tensor(SCAL), torch.tensor(SCAL) * 0.5])[: B if scal_stride else 1].contiguous()
    Fd, xd, sd = cu(Fh), cu(xa), cu(scal)
    rden, rxn = R.ddim_edm_step(Fh, xa, scal)
    for want_den, want_xn in ((True, True), (False, True), (True, False)):
        den = H.Guarded(B, per_sample) if want_den else None
        xn = H.Guarded(B, per_sample) if want_xn else None
        H.launch_guard(4, Fd, xd, sd, den and den.t, xn and xn.t)
        rc = lib.mode_ddim_edm_step(H.p(Fd), H.p(xd), H.p(sd), scal_stride, B, per_sample, H.p(den and den.t), H.p(xn and xn.t), H.stream())
        torch.cuda.synchronize()
        assert rc == 0 and (den is None or den.intact()) and (xn is None or xn.intact()), rc
        ed, ex = (rel(den.t, rden) if den else 0.0), (rel(xn.t, rxn) if xn else 0.0)
        print(f"ddim_edm_step B={B} n={per_sample} stride={scal_stride}: denoised {ed:.2e} x_next {ex:.2e} (< {HEAD:.0e})")
        assert ed < HEAD and ex < HEAD, (B, per_sample, scal_stride, ed, ex)


@pytest.mark.parametrize("scal_stride", [0, 4])
def test_ddim_edm_step_equals_the_head_epilogue(scal_stride):
    """The header documents mode_ddim_edm_step as the head's plain DDIM epilogue standalone: fed the head's own F, its denoised / x_next agree with the
    head's at the fp32 bound."""
    lib = L.load()
    d = head_inputs(256, 7, 2, 1, "bf16", 4, seed=5)
    out, g_ = run_head(d, "ddim", scal_stride)
    n = A_LEN_H * 7
    den, xn = H.Guarded(B_H, n), H.Guarded(B_H, n)
    scal = g_["scal"] if scal_stride else g_["scal"][:1].contiguous()
    H.launch_guard(4, out["F"].t, g_["x_a"], scal, den.t, xn.t)
    assert lib.mode_ddim_edm_step(H.p(out["F"].t), H.p(g_["x_a"]), H.p(scal), scal_stride, B_H, n, H.p(den.t), H.p(xn.t), H.stream()) == 0
    torch.cuda.synchronize()
    assert den.intact() and xn.intact()
    ed, ex = rel(den.t.view(-1), out["denoised"].t.view(-1)), rel(xn.t.view(-1), out["x_next"].t.view(-1))
    print(f"ddim_edm_step vs head epilogue stride={scal_stride}: denoised {ed:.2e} x_next {ex:.2e} (< {F32:.0e})")
    assert ed < F32 and ex < F32


@pytest.mark.parametrize("D", [4, 260])
@pytest.mark.parametrize("Rr", [1, 5])
def test_sigma_embed(Rr, D):
    lib = L.load()
    sigma = torch.tensor([1e-3, 80.0, 0.5, 1.0, 7.3])[:Rr].contiguous()
    w, b = rnd(D, 1, seed=1), rnd(D, seed=2)
    sd, wd, bd, e1 = cu(sigma), cu(w), cu(b), H.Guarded(Rr, D)
    H.launch_guard(D, sd, wd, bd, e1.t)
    rc = lib.mode_sigma_embed(H.p(sd), H.p(wd), H.p(bd), H.p(e1.t), Rr, D, H.stream())
    torch.cuda.synchronize()
    assert rc == 0 and e1.intact()
    e = rel(e1.t, R.sigma_embed(sigma, w, b))
    print(f"sigma_embed R={Rr} D={D}: {e:.2e} (< {HEAD:.0e})")
    assert e < HEAD


# ================================================================================================================== refusals before any launch
def test_one_wave_per_row_launchers_refuse_rows_past_their_lds():
    """4 rows x D fp32 of dynamic LDS per workgroup without the large-LDS attribute: D = 4100 (65600 bytes) is MODE_ERR_UNSUPPORTED (-2) from the four
    one-wave-per-row launchers, on the host, before any launch (it used to come back as the launch's positive hipError_t)."""
    lib, D, n = L.load(), 4100, 2
    d = {k_: cu(v) for k_, v in combine_inputs(D, 2, 1, "bf16", 0, 1, n=n).items()}
    xn, h = H.Guarded(n, D), H.Guarded(n, D, torch.bfloat16)
    assert H.combine_fused(d["u"], d["Y"], d["pos"], d["posw"], d["g"], d["cond"], 1, xn, h) == -2
    assert lib.mode_rmsnorm_cond_fwd(H.p(d["u"]), H.p(d["g"]), None, n, D, 1, 1e-6, H.p(xn.t), H.p(h.t), L.MODE_BF16, H.stream()) == -2
    B, A_len, A_dim, n_img = 1, 1, 7, 0
    w_out, b_out, Fo = cu(rnd(A_dim, D)), cu(rnd(A_dim)), H.Guarded(A_len, A_dim)
    desc = H.head_desc(d["u"], d["Y"], d["pos"], d["posw"], d["g"], w_out, b_out, B, 2, A_len, F=Fo.t)
    assert lib.mode_head_ddim_fwd(C.byref(desc), H.stream()) == -2
    act, w_act, pos = cu(rnd(B, A_len, A_dim)), cu(rnd(D, A_dim)), cu(rnd(1 + A_len, D))
    e = L.ModeEmbedDesc(B=B, T=2, D=D, A_len=A_len, A_dim=A_dim, n_img=n_img, use_noise_token=0, goal_e=H.p(d["u"]), img_e=H.p(d["u"]), actions=H.p(act),
                        w_act=H.p(w_act), pos=H.p(pos), g=H.p(d["g"]), eps=1e-6, x=H.p(xn.t), h=H.p(h.t), h_dtype=L.MODE_BF16)
    assert lib.mode_embed_tokens_fwd(C.byref(e), H.stream()) == -2
    torch.cuda.synchronize()
    assert xn.intact() and h.intact() and Fo.intact() and bool(torch.isnan(xn.t).all()) and bool(torch.isnan(Fo.t).all())
