"""CPU: the fp64 reference of the device-side gradient norms (tests/grad_norm_refs.py) against torch.nn.utils.clip_grad_norm_, and the chunk-table
builder of optim.GradClip (a pure function of (spans, chunk): no device involved)."""
import random

import pytest
import torch

import grad_norm_refs as R
from mode_diffusion_policy_amd import _lib as L
from mode_diffusion_policy_amd.optim import GRAD_CHUNK, build_chunk_table, chunk_slices


def _tensors(seed):
    sizes = [(1,), (3,), (5, 7), (1000,), (2, 3, 4, 5), (R.CH + 1,)]
    return [R.make_values(int(torch.Size(s).numel()), seed + i).reshape(s) for i, s in enumerate(sizes)]


@pytest.mark.parametrize("max_norm_factor,grad_scale", [(0.5, 1.0), (2.0, 1.0), (0.5, 0.5), (None, 1.0)])
def test_reference_matches_torch_clip_grad_norm(max_norm_factor, grad_scale):
    ts = _tensors(3)
    R.assert_normal_squares(ts)
    sq = R.ref_tensor_sq(ts)
    plain = R.ref_clip(sq, None, grad_scale)[1]
    max_norm = None if max_norm_factor is None else max_norm_factor * plain
    total, norm, coef, scale = R.ref_clip(sq, max_norm, grad_scale)
    params = [torch.nn.Parameter(torch.zeros(t.shape, dtype=torch.float64)) for t in ts]
    for p, t in zip(params, ts):
        p.grad = t.double() * grad_scale                              # torch clips the gradient it is given: the scaled one
    tn = torch.nn.utils.clip_grad_norm_(params, float("inf") if max_norm is None else max_norm)
    assert abs(float(tn) - norm) <= 1e-12 * norm
    for p, t in zip(params, ts):
        want = t.double() * scale                                     # scale = grad_scale * coef applied to the RAW gradient, as the AdamW launches do
        assert float((p.grad - want).abs().max()) <= 1e-12 * float(want.abs().max())
    assert (coef == 1.0) == (max_norm is None or max_norm_factor > 1)
    for s, t in zip(sq, ts):
        assert abs(s - float(t.double().norm() ** 2)) <= 1e-12 * s


def test_bound_constants_follow_the_kernel_structure():
    assert R.CH == GRAD_CHUNK == L.MODE_GRAD_CHUNK
    assert R.A == R.CH // (4 * 256) + 2 + 6 + 3 == 27 and R.REL_PARTIAL == 28 * 2.0 ** -24
    assert R.n_chunks(0) == 0 and R.n_chunks(1) == 1 and R.n_chunks(R.CH) == 1 and R.n_chunks(R.CH + 1) == 2


def _check_table(spans, tab, chunk):
    lo, n, tn, begin, index = tab["lo"], tab["n"], tab["tensor"], tab["begin"], tab["index"]
    included = [i for i, s in enumerate(spans) if s[2]]
    assert index == included and len(begin) == len(included) + 1 and begin[0] == 0 and begin[-1] == len(lo)
    assert all(x % 4 == 0 for x in lo) and all(0 < k <= chunk for k in n)                     # 16-byte aligned, at most one chunk long, never empty
    assert lo == sorted(lo)
    covered = {}
    for c, (a, k, t) in enumerate(zip(lo, n, tn)):
        s_lo, s_n, _ = spans[index[t]]
        assert s_lo <= a and a + k <= s_lo + s_n, "a chunk leaves its tensor"                 # no chunk spans two tensors
        assert begin[t] <= c < begin[t + 1]
        for e in range(a, a + k):
            assert e not in covered, "an element lies in two chunks"
            covered[e] = t
    want = {e for i in included for e in range(spans[i][0], spans[i][0] + spans[i][1])}
    assert set(covered) == want                                                               # every included element exactly once, nothing else
    for i, (s_lo, s_n, inc) in enumerate(spans):
        if not inc:
            assert not any(e in covered for e in range(s_lo, s_lo + s_n)), "an excluded span is covered"


def _random_spans(rng, count, chunk):
    spans, o = [], 0
    for _ in range(count):
        numel = rng.choice([0, 1, 3, 4, 5, chunk - 1, chunk, chunk + 1, 2 * chunk + 7, rng.randrange(1, 3 * chunk)])
        spans.append((o, numel, rng.random() < 0.8))
        o += (numel + 3) // 4 * 4 + 4 * rng.randrange(0, 3)                                    # alignment padding (never covered)
    return spans


@pytest.mark.parametrize("chunk", [8, 64])
def test_chunk_table_covers_every_included_element_exactly_once(chunk):
    rng = random.Random(chunk)
    for _ in range(20):
        spans = _random_spans(rng, rng.randrange(1, 12), chunk)
        _check_table(spans, build_chunk_table(spans, chunk), chunk)
    empty = build_chunk_table([(0, 5, False)], chunk)
    assert empty["lo"] == [] and empty["begin"] == [0] and empty["index"] == []


def test_chunk_table_at_the_shipped_chunk_size_and_refusals():
    CH = GRAD_CHUNK
    sizes = [0, 1, 3, 4, 5, 255, 1023, CH - 1, CH, CH + 1, 2 * CH + 7]
    spans, o = [], 4
    for k in sizes:
        spans.append((o, k, True))
        o += (k + 3) // 4 * 4 + 4
    tab = build_chunk_table(spans)
    assert [tab["begin"][t + 1] - tab["begin"][t] for t in range(len(sizes))] == [R.n_chunks(k) for k in sizes]
    assert all(x % 4 == 0 for x in tab["lo"]) and max(tab["n"]) == CH
    assert sum(tab["n"]) == sum(sizes)
    with pytest.raises(NotImplementedError):
        build_chunk_table([(2, 8, True)])                                                      # not 16-byte aligned
    with pytest.raises(ValueError):
        build_chunk_table([(0, 8, True), (4, 8, True)])                                        # overlapping
    with pytest.raises(ValueError):
        build_chunk_table([(0, 8, True)], chunk=6)
    assert build_chunk_table([(2, 8, False), (8, 8, True)])["lo"] == [8]                       # an excluded span needs no alignment: it is never read


def test_block_sub_ranges_of_the_overlap_path_partition_the_table():
    """FusedAdamW.step(overlap=True) measures block l's chunks behind block l's event and the rest after the backward: together every chunk once."""
    chunk = 16
    # a small arena: [stacked head tensors | block 1 | block 0 | tail tensors], blocks = slices that start and end on tensor boundaries
    sizes = [40, 7, 0, 33, 16, 5, 64, 17, 3, 100, 1]
    spans, o, offs = [], 0, []
    for i, k in enumerate(sizes):
        offs.append(o)
        spans.append((o, k, i != 4))                                                           # one frozen tensor inside a block
        o += (k + 7) // 8 * 8
    tab = build_chunk_table(spans, chunk)
    blocks = [(offs[3], offs[6]), (offs[6], offs[9])]
    per, rest = chunk_slices(tab, blocks)
    ranges = sorted(per + rest)
    flat = [c for a, k in ranges for c in range(a, a + k)]
    assert flat == list(range(len(tab["lo"])))                                                 # a partition: every chunk exactly once
    for (lo, hi), (a, k) in zip(blocks, per):
        assert all(lo <= tab["lo"][c] and tab["lo"][c] + tab["n"][c] <= hi for c in range(a, a + k))
        assert k == sum(1 for x in tab["lo"] if lo <= x < hi)
    # slices given in any order; a slice boundary inside a tensor is refused
    per2, rest2 = chunk_slices(tab, blocks[::-1])
    assert per2 == per[::-1] and rest2 == rest
    with pytest.raises(ValueError):
        chunk_slices(tab, [(offs[3] + 4, offs[6])])
    with pytest.raises(ValueError):
        chunk_slices(tab, [(offs[3], offs[6]), (offs[5], offs[9])])
    assert chunk_slices(tab, []) == ([], [(0, len(tab["lo"]))])
