"""CPU: the fp64 reference of tests/lora_fact_refs.py is the dense chain rule dA = s B^T (dY^T X), dB = s (dY^T X) A^T, every deliberately wrong
reference sits outside the derived bound on the inputs the GPU tests use (or is excused by name), the exactness family is exact in fp32 in any
order, and the host side of the feature - refused descriptors, the workspace query, the adapter's `grad` keyword - behaves as stated."""
import ctypes as C

import pytest
import torch

import lora_fact_refs as R
from mode_diffusion_policy_amd import _lib as L


@pytest.mark.parametrize("G,rows,cols,r,perm", R.CASES)
def test_reference_is_the_dense_chain_rule_and_wrong_references_are_outside_the_bound(G, rows, cols, r, perm):
    d = R.inputs(G, rows, cols, r, perm)
    args = (d["X"], d["dY"], d["offsets"], d["x_rows"], d["A"], d["B"], R.SCALE)
    (dA, dB), (bA, bB) = R.fact_ref(*args)
    wA, wB = R.dense_ref(*args)
    for got, ref in ((dA, wA), (dB, wB)):
        assert float((got - ref).abs().max()) <= 1e-12 * max(float(ref.abs().max()), 1e-300)
    sizes = [b - a for a, b in zip(d["offsets"], d["offsets"][1:])]
    assert (G == 1 and sizes[0] > 0) or sorted(sizes)[0] == 0 and sorted(sizes)[1] > 0          # every G = 3 case has exactly one empty group
    for g, n in enumerate(sizes):
        if n == 0:
            assert float(dA[g].abs().max()) == 0 and float(dB[g].abs().max()) == 0 and float(bA[g].max()) == 0 and float(bB[g].max()) == 0
    wrong = R.wrong_refs(*args)
    assert set(wrong) == {"scale dropped", "groups swapped", "x_rows ignored", "last row of each group dropped", "T and U exchanged"}
    # the cases that cannot tell a wrong reference apart are exactly these, by name (one condition per wrong reference)
    assert (wrong["groups swapped"] is None) == (G == 1) and (wrong["x_rows ignored"] is None) == (not perm) and set(R.EXCUSED) == {"groups swapped", "x_rows ignored"}
    for name, w in wrong.items():
        if w is None:
            assert name in R.EXCUSED
            continue
        qa, qb = R.worst(w[0], dA, bA), R.worst(w[1], dB, bB)
        # more than TWICE the bound away: whatever lies within the bound of the right reference is then outside the bound of the wrong one
        assert qa > 2 and qb > 2, (name, qa, qb)


@pytest.mark.parametrize("G,rows,cols,r", R.EXACT_CASES)
def test_exactness_inputs_are_exact_in_fp32_in_any_order(G, rows, cols, r):
    d = R.exact_inputs(G, rows, cols, r)                                           # asserts the 2^24 headroom itself
    (dA, dB), _ = R.fact_ref(d["X"], d["dY"], d["offsets"], d["x_rows"], d["A"], d["B"], d["s"])
    X = d["X"].float()[d["x_rows"].long()]
    dY = d["dY"].float()
    s = torch.tensor(d["s"])
    for order in (lambda n: torch.arange(n), lambda n: torch.arange(n).flip(0)):
        for g in range(G):
            lo, hi = d["offsets"][g], d["offsets"][g + 1]
            Xg, Yg = X[lo:hi], dY[lo:hi]
            T = torch.zeros(hi - lo, r)
            for i in order(rows):
                T = T + Yg[:, i, None] * d["B"][g, i][None, :]
            Uu = torch.zeros(hi - lo, r)
            for j in order(cols):
                Uu = Uu + Xg[:, j, None] * d["A"][g, :, j][None, :]
            gA, gB = torch.zeros(r, cols), torch.zeros(rows, r)
            for m in order(hi - lo):
                gA = gA + T[m][:, None] * Xg[m][None, :]
                gB = gB + Yg[m][:, None] * Uu[m][None, :]
            assert torch.equal((s * gA).double(), dA[g]) and torch.equal((s * gB).double(), dB[g])


def test_entry_points_refuse_bad_descriptors_without_a_device():
    lib = L.load()
    good = dict(G=3, rows=72, cols=64, r=16, M=300, dtype=L.MODE_BF16, ld_x=64, ld_dy=72)
    for change in (dict(r=0), dict(r=65), dict(cols=68), dict(rows=12), dict(dtype=L.MODE_F32)):
        d = L.ModeLoraFactDesc(**dict(good, **change))
        assert lib.mode_lora_fact_workspace_bytes(C.byref(d)) == 0, change
        assert lib.mode_lora_fact_grad(C.byref(d), None, 0, None) == -2, change
    d = L.ModeLoraFactDesc(**good)
    up = lambda n: (n + 255) // 256 * 256
    assert lib.mode_lora_fact_workspace_bytes(C.byref(d)) == 2 * up(300 * 16 * 4) + up((300 // 128 + 3 + 1) * 16 * (72 + 64) * 4)
    assert lib.mode_lora_fact_grad(C.byref(d), None, 0, None) == -1                # null pointers
    assert lib.mode_lora_fact_grad(None, None, 0, None) == -1 and lib.mode_lora_fact_workspace_bytes(None) == 0
    for change in (dict(G=0), dict(M=-1)):
        assert lib.mode_lora_fact_grad(C.byref(L.ModeLoraFactDesc(**dict(good, **change))), None, 0, None) == -1, change
    dims = L.ModeDims(D=1024, H=8, L=12, E=4, k=2, T=14, A_len=10, A_dim=7, O=2048, G=512, n_img=2, use_noise_token=1, router_normalize=1, eps=1e-6)
    need = lib.mode_dit_backward_lora_workspace_bytes(C.byref(dims), 128, 16)
    w1 = L.ModeLoraFactDesc(G=4, rows=8192, cols=1024, r=16, M=128 * 14 * 2, dtype=L.MODE_BF16)
    assert need == lib.mode_lora_fact_workspace_bytes(C.byref(w1)) > 0             # the up-projection is the largest of the four
    assert need < 64 << 20                                                         # tens of MB, not the 2.7 GB of a dense gradient
    assert lib.mode_dit_backward_lora_workspace_bytes(C.byref(dims), 128, 65) == 0 and lib.mode_dit_backward_lora_workspace_bytes(C.byref(dims), 0, 16) == 0
    assert lib.mode_dit_backward_lora(C.byref(dims), None, None, None, None, None, None, None, None, 0, None) == -1


def test_adapter_grad_keyword_on_the_host():
    """`grad` is validated, a plain attribute, and no part of the adapter's state: a dict saved in one mode loads in the other."""
    import mode_diffusion_policy_amd as M
    kw = dict(obs_dim=32, goal_dim=16, device="cpu", goal_conditioned=True, action_dim=7, embed_dim=64, embed_pdrob=0, attn_pdrop=0.0, n_layers=2,
              n_heads=4, goal_seq_len=1, obs_seq_len=1, action_seq_len=10, num_experts=4, top_k=2)
    m = M.MoDeDiT(**kw)
    assert M.LoraAdapter(m, rank=4).grad == "dense"
    ad = M.LoraAdapter(m, rank=4, alpha=6.0, seed=3, grad="factored")
    assert ad.grad == "factored"
    for bad in ("nonsense", None, "Dense"):
        with pytest.raises(ValueError, match="grad"):
            M.LoraAdapter(m, rank=4, grad=bad)
        with pytest.raises(ValueError, match="grad"):
            ad.grad = bad
    assert ad.grad == "factored"
    dense = M.LoraAdapter(m, rank=4, alpha=6.0, seed=3)
    sd_f, sd_d = ad.state_dict(), dense.state_dict()
    assert list(sd_f) == list(sd_d) and sd_f["_extra_state"] == sd_d["_extra_state"] and "grad" not in sd_f["_extra_state"]
    assert all(torch.equal(sd_f[k], sd_d[k]) for k in sd_f if k != "_extra_state")
    key = ad._key()
    ad.grad = "dense"
    assert ad._key() == key                                                        # not part of the merge key
    other = M.LoraAdapter(m, rank=4, seed=9, grad="dense")
    other.load_state_dict(M.LoraAdapter(m, rank=4, alpha=6.0, seed=3, grad="factored").state_dict())
    assert other.grad == "dense" and other.alpha == 6.0 and torch.equal(other.A_wo, ad.A_wo)
    from mode_diffusion_policy_amd.lora import small_grad_layout
    from mode_diffusion_policy_amd.arena import arena_layout
    from types import SimpleNamespace
    ar = SimpleNamespace(**dict(zip(("layout", "bounds"), arena_layout(m))))
    lay, total = small_grad_layout(ar)
    keys = [k for k, _, _ in lay]
    assert not any(k.split(".")[-1] in ("wqkv", "wo", "w1", "w2") for k in keys) and "l0.bqkv" in keys and "l1.b1" in keys and "r_w0" in keys
    assert total * 8 < ar.bounds["total"] and all(off % 64 == 0 for _, _, off in lay)
