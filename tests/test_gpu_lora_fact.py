"""GPU: mode_lora_fact_grad (csrc/lora_train.hip) through ctypes, per element against the fp64 reference and the DERIVED bound of
tests/lora_fact_refs.py: every shape, rank, group count and row map there (ragged groups, one empty group in every G = 3 case), canaries around
both outputs, bit-identity of two runs, the deliberately wrong references outside the bound, exact +0.0 for a group without rows, the exactness
family with no tolerance at all, the scale read at run time, and refused descriptors that launch nothing."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

import lora_fact_refs as R  # noqa: E402
from hip_helpers import Guarded, stream  # noqa: E402
from mode_diffusion_policy_amd import _lib as L  # noqa: E402

WORST = {"dA": 0.0, "dB": 0.0}                                                     # the largest error / bound seen, printed by every case


def bits(t):
    return t.detach().contiguous().view(torch.int32).cpu()


def scale_dev(s=R.SCALE):
    return torch.tensor([s], dtype=torch.float32, device="cuda")


class Case:
    """Device operands of one reference case and NaN-prefilled, canary-guarded outputs."""

    def __init__(self, d, G, rows, cols, r, s):
        self.G, self.rows, self.cols, self.r = G, rows, cols, r
        self.X, self.dY, self.A, self.B = (d[k].cuda().contiguous() for k in ("X", "dY", "A", "B"))
        self.xr = d["x_rows"].cuda() if d["x_rows"] is not None else None
        self.off = torch.tensor(d["offsets"], dtype=torch.int32, device="cuda")
        self.M, self.s = d["M"], s
        self.fresh()

    def fresh(self, fill=float("nan")):
        self.dA, self.dB = Guarded(self.G * self.r, self.cols, fill=fill), Guarded(self.G * self.rows, self.r, fill=fill)

    def desc(self, **change):
        f = dict(G=self.G, rows=self.rows, cols=self.cols, r=self.r, M=self.M, dtype=L.MODE_BF16, X=self.X.data_ptr(), ld_x=self.cols,
                 x_rows=None if self.xr is None else self.xr.data_ptr(), dY=self.dY.data_ptr(), ld_dy=self.rows, group_offsets=self.off.data_ptr(),
                 A=self.A.data_ptr(), B=self.B.data_ptr(), scale=self.s.data_ptr(), dA=self.dA.t.data_ptr(), dB=self.dB.t.data_ptr())
        f.update(change)
        return L.ModeLoraFactDesc(**f)

    def run(self, d=None, ws_bytes=None):
        lib = L.load()
        d = d or self.desc()
        need = lib.mode_lora_fact_workspace_bytes(C.byref(d))
        self.ws = torch.empty(max(need, 256), dtype=torch.uint8, device="cuda")
        rc = lib.mode_lora_fact_grad(C.byref(d), self.ws.data_ptr(), need if ws_bytes is None else ws_bytes, stream())
        torch.cuda.synchronize()
        return rc

    def out(self):
        return self.dA.t.cpu().view(self.G, self.r, self.cols), self.dB.t.cpu().view(self.G, self.rows, self.r)


@pytest.mark.parametrize("G,rows,cols,r,perm", R.CASES)
def test_per_element_bit_identity_wrong_references_and_empty_groups(G, rows, cols, r, perm):
    d = R.inputs(G, rows, cols, r, perm)
    s = scale_dev()
    s32 = float(s.cpu()[0])                                                        # the reference uses the fp32 value the kernel reads
    args = (d["X"], d["dY"], d["offsets"], d["x_rows"], d["A"], d["B"], s32)
    (rA, rB), (bA, bB) = R.fact_ref(*args)
    c = Case(d, G, rows, cols, r, s)
    runs = []
    for _ in range(2):
        c.fresh()
        assert c.run() == 0
        assert c.dA.intact() and c.dB.intact()
        runs.append(c.out())
    (gA, gB), (gA2, gB2) = runs
    assert torch.equal(bits(gA), bits(gA2)) and torch.equal(bits(gB), bits(gB2))   # run to run: the same bits
    qa, qb = R.worst(gA, rA, bA), R.worst(gB, rB, bB)
    WORST["dA"], WORST["dB"] = max(WORST["dA"], qa), max(WORST["dB"], qb)
    print(f"fact G={G} {rows}x{cols} r={r} sizes={[b - a for a, b in zip(d['offsets'], d['offsets'][1:])]} x_rows={perm}: worst error / bound "
          f"dA {qa:.3f} dB {qb:.3f}   (so far: dA {WORST['dA']:.3f} dB {WORST['dB']:.3f})")
    assert torch.isfinite(gA).all() and torch.isfinite(gB).all() and qa <= 1.0 and qb <= 1.0, (qa, qb)
    for name, w in R.wrong_refs(*args).items():
        if w is None:
            assert name in R.EXCUSED                                               # G == 1 / no x_rows: said so by name, not skipped
            continue
        assert R.worst(gA, w[0], bA) > 1.0 and R.worst(gB, w[1], bB) > 1.0, name   # the kernel is told apart from each wrong reference
    for g in range(G):
        if d["offsets"][g] == d["offsets"][g + 1]:                                 # a group without rows: +0.0, bit pattern 0 (not -0.0)
            assert bool((bits(gA[g]) == 0).all()) and bool((bits(gB[g]) == 0).all())


@pytest.mark.parametrize("G,rows,cols,r", R.EXACT_CASES)
def test_exactness_inputs_come_back_without_any_error(G, rows, cols, r):
    d = R.exact_inputs(G, rows, cols, r)
    (rA, rB), _ = R.fact_ref(d["X"], d["dY"], d["offsets"], d["x_rows"], d["A"], d["B"], d["s"])
    c = Case(d, G, rows, cols, r, scale_dev(d["s"]))
    assert c.run() == 0 and c.dA.intact() and c.dB.intact()
    gA, gB = c.out()
    assert torch.equal(gA.double(), rA) and torch.equal(gB.double(), rB)           # A and B at full fp32 precision, every sum in fp32: exact


def test_scale_is_read_from_the_device_at_run_time_and_a_negative_scale_keeps_empty_groups_at_plus_zero():
    G, rows, cols, r = 3, 72, 64, 3
    d = R.inputs(G, rows, cols, r, True)
    s = scale_dev(0.5)
    c = Case(d, G, rows, cols, r, s)
    desc = c.desc()                                                                # ONE descriptor, the scalar changes under it
    for val in (0.5, -2.25):
        s.fill_(val)
        assert c.run(desc) == 0
        (rA, rB), (bA, bB) = R.fact_ref(d["X"], d["dY"], d["offsets"], d["x_rows"], d["A"], d["B"], val)
        gA, gB = c.out()
        assert R.worst(gA, rA, bA) <= 1.0 and R.worst(gB, rB, bB) <= 1.0 and c.dA.intact() and c.dB.intact()
        empty = [g for g in range(G) if d["offsets"][g] == d["offsets"][g + 1]]
        assert empty and all(bool((bits(gA[g]) == 0).all()) and bool((bits(gB[g]) == 0).all()) for g in empty)


def test_no_group_offsets_means_one_group_of_all_rows_and_no_rows_at_all_give_zeros():
    G, rows, cols, r = 1, 384, 128, 16
    d = R.inputs(G, rows, cols, r, False)
    s = scale_dev()
    (rA, rB), (bA, bB) = R.fact_ref(d["X"], d["dY"], None, None, d["A"], d["B"], float(s.cpu()[0]))
    c = Case(d, G, rows, cols, r, s)
    assert c.run(c.desc(group_offsets=None)) == 0
    gA, gB = c.out()
    assert R.worst(gA, rA, bA) <= 1.0 and R.worst(gB, rB, bB) <= 1.0
    c.fresh()
    assert c.run(c.desc(group_offsets=None, M=0)) == 0                             # M = 0: nothing but the finishing pass runs
    gA, gB = c.out()
    assert bool((bits(gA) == 0).all()) and bool((bits(gB) == 0).all()) and c.dA.intact() and c.dB.intact()


@pytest.mark.parametrize("change,status", [(dict(r=0), -2), (dict(r=65), -2), (dict(cols=68), -2), (dict(rows=12), -2), (dict(dtype=L.MODE_F32), -2),
                                           ("short workspace", -3)])
def test_bad_descriptors_return_the_stated_error_and_touch_nothing(change, status):
    G, rows, cols, r = 1, 72, 64, 16
    d = R.inputs(G, rows, cols, r, False)
    c = Case(d, G, rows, cols, r, scale_dev())
    c.fresh(fill=float("nan"))
    if change == "short workspace":
        need = L.load().mode_lora_fact_workspace_bytes(C.byref(c.desc()))
        assert need > 256 and c.run(ws_bytes=need - 1) == status
    else:
        assert c.run(c.desc(**change)) == status
    assert bool(torch.isnan(c.dA.t).all()) and bool(torch.isnan(c.dB.t).all()) and c.dA.intact() and c.dB.intact()
