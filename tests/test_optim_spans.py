"""The two pure range helpers of optim.py, no device: ``_merge_spans`` (frozen tensors / expert matrices -> the holes of an optimizer step) and
``_carve`` (the sub-ranges of ``[lo, hi)`` an AdamW launch sequence covers around those holes)."""
import random

from mode_diffusion_policy_amd.optim import _carve, _merge_spans


def test_merge_spans_empty_touching_nested_unsorted():
    assert _merge_spans([]) == []
    assert _merge_spans([(3, 9)]) == [[3, 9]]
    assert _merge_spans([(0, 4), (4, 8)]) == [[0, 8]]                                 # touching spans merge
    assert _merge_spans([(0, 4), (5, 8)]) == [[0, 4], [5, 8]]
    assert _merge_spans([(0, 16), (4, 8), (8, 12)]) == [[0, 16]]                      # nested
    assert _merge_spans([(0, 6), (4, 10)]) == [[0, 10]]                               # overlapping
    assert _merge_spans([(20, 24), (0, 4), (8, 12), (2, 8)]) == [[0, 12], [20, 24]]   # unsorted
    assert _merge_spans([[8, 12], (0, 4)]) == [[0, 4], [8, 12]]                       # lists and tuples mix (frozen ranges + expert ranges)
    assert _merge_spans(iter([(4, 8), (0, 4)])) == [[0, 8]]                           # any iterable


def test_carve_around_holes():
    carve = lambda lo, hi, holes: list(_carve(lo, hi, holes))                         # noqa: E731
    assert carve(0, 16, []) == [(0, 16)]
    assert carve(0, 16, [(0, 4)]) == [(4, 16)]                                        # a hole at the start
    assert carve(0, 16, [(12, 16)]) == [(0, 12)]                                      # a hole at the end
    assert carve(4, 12, [(4, 12)]) == [] and carve(4, 12, [(0, 16)]) == []            # a hole covering everything: nothing is launched
    assert carve(8, 16, [(0, 8), (16, 20), (40, 44)]) == [(8, 16)]                    # holes outside, touching included
    assert carve(0, 32, [(4, 8), (16, 20)]) == [(0, 4), (8, 16), (20, 32)]            # two holes inside
    assert carve(6, 18, [(4, 8), (16, 20)]) == [(8, 16)]                              # holes straddling both ends
    assert carve(0, 16, [[4, 8], [8, 12]]) == [(0, 4), (12, 16)]                      # touching holes (w1 / w2 of one block)
    assert carve(5, 5, [(0, 4)]) == [] and carve(8, 4, []) == []                      # an empty range yields nothing


def test_carved_pieces_and_holes_partition_the_range():
    rng = random.Random(20240)
    for case in range(400):
        holes = _merge_spans((a, a + rng.randint(1, 12)) for a in (rng.randint(0, 60) for _ in range(rng.randint(0, 6))))
        lo = rng.randint(0, 63)
        hi = rng.randint(lo, 63)
        pieces = list(_carve(lo, hi, holes))
        clipped = [(max(a, lo), min(b, hi)) for a, b in holes if max(a, lo) < min(b, hi)]
        assert all(a < b for a, b in pieces), (case, pieces)                          # no empty piece
        assert pieces == sorted(pieces)
        cover = sorted(pieces + clipped)
        assert [x for span in cover for x in range(*span)] == list(range(lo, hi)), (case, lo, hi, holes, pieces)   # every element exactly once
        for (_, b), (a, _) in zip(cover[:-1], cover[1:]):
            assert b == a
