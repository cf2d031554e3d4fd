"""The strip plan of the half-sweep schedule (acmmp_strip_plan) is a pure host function: boundaries
on multiples of 4 rows, strips of at least ACMMP_BAND_HALO = 23 rows covering [0, rows) exactly once, waits on
exactly the neighbouring strips, and a single strip with no waits.  No GPU."""
import pytest

from acmmp import capi

HALO = 23


@pytest.mark.parametrize("rows", [1, 3, 22, 23, 24, 47, 48, 49, 95, 96, 100, 128, 750, 1000, 1200, 1500, 1501, 4096])
@pytest.mark.parametrize("want", [1, 2, 3, 4, 7, 8, 64, 1000])
def test_plan(rows, want):
    bounds, waits = capi.strip_plan(rows, want)
    ns = len(bounds) - 1
    assert 1 <= ns <= min(want, 64) and len(waits) == ns
    assert bounds[0] == 0 and bounds[-1] == rows                     # covers [0, rows) ...
    assert all(a < b for a, b in zip(bounds, bounds[1:]))            # ... exactly once, no empty strip
    assert all(b % 4 == 0 for b in bounds[:-1])                      # every boundary between two strips
    if ns > 1:
        assert all(b - a >= HALO for a, b in zip(bounds, bounds[1:]))
    # as many strips as asked for whenever the rows allow it
    assert ns == max(1, min(want, 64, (rows // 4) // 6))
    for i, w in enumerate(waits):
        assert w == ([] if ns == 1 else [j for j in (i - 1, i, i + 1) if 0 <= j < ns])


def test_single_strip():
    assert capi.strip_plan(1500, 1) == ([0, 1500], [[]])
    assert capi.strip_plan(20, 4) == ([0, 20], [[]])                 # too short to cut


def test_even_deal():
    assert capi.strip_plan(96, 4)[0] == [0, 24, 48, 72, 96]
    assert capi.strip_plan(100, 3)[0] == [0, 36, 68, 100]
    assert capi.strip_plan(1500, 4)[0] == [0, 376, 752, 1128, 1500]
    assert capi.strip_plan(96, 64)[0] == [0, 24, 48, 72, 96]         # clamped


def test_invalid():
    with pytest.raises(capi.AcmmpError):
        capi.strip_plan(0, 4)
