"""The scratch slab's share of the kept-sample mask, through acmmp_keep_mask_bytes: a host function that applies the
gates build_kparams applies (the same functions: interpolation geometry, fast math, binary16 texels, V <= 4, the
ACMMP_REF_NEG_SKIP and ACMMP_KEEP_MASK switches, no geom pass) and the piece count it carves.  A run that publishes the
mask holds one 64-bit word per pixel of each colour grid and -- because k_init publishes the patch sums of both colours,
while the recompute path shares one colour's array between the half-sweeps -- a second colour's float4 sums: 32 bytes per
pixel of one colour grid.  Every other run grows by nothing.  No GPU."""
import pytest

from acmmp import capi

KNOBS = ("ACMMP_KEEP_MASK", "ACMMP_REF_NEG_SKIP", "ACMMP_REF_NEG_TAU")


@pytest.fixture(autouse=True)
def clean_env(monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)


@pytest.mark.parametrize("W,H,V", [(2000, 1000, 2), (2000, 1500, 4), (2001, 1001, 1), (4000, 2000, 3)])
def test_gated_run_grows(W, H, V):
    Pc = H * ((W + 1) // 2)                              # pixels of one colour grid
    assert capi.keep_mask_bytes(W, H, n_src=V) == 8 * 2 * Pc + 16 * Pc


def test_every_other_run_grows_by_nothing(monkeypatch):
    W, H = 2000, 1000
    assert capi.keep_mask_bytes(W, H, n_src=4) > 0
    assert capi.keep_mask_bytes(W, H, n_src=5) == 0                       # V > 4
    assert capi.keep_mask_bytes(W, H, fast=False) == 0                    # exact mode
    assert capi.keep_mask_bytes(W, H, tex16=False) == 0                   # fp32 texels
    assert capi.keep_mask_bytes(W, H, model=0) == 0                       # pinhole
    assert capi.keep_mask_bytes(W, H, geom=True) == 0                     # geom pass
    assert capi.keep_mask_bytes(1998, H) == 0 and capi.keep_mask_bytes(W, 998) == 0     # below the gate's size
    assert capi.keep_mask_bytes(W, H, patch_size=7) == 0                  # not 6 x 6 samples
    assert capi.keep_mask_bytes(4000, 2000, patch_size=21, radius_increment=4) > 0
    monkeypatch.setenv("ACMMP_KEEP_MASK", "0")
    assert capi.keep_mask_bytes(W, H) == 0
    monkeypatch.setenv("ACMMP_KEEP_MASK", "1")
    monkeypatch.setenv("ACMMP_REF_NEG_SKIP", "0")
    assert capi.keep_mask_bytes(W, H) == 0
    monkeypatch.delenv("ACMMP_REF_NEG_SKIP")
    monkeypatch.setenv("ACMMP_REF_NEG_TAU", "0.125")
    assert capi.keep_mask_bytes(W, H) > 0


def test_invalid():
    with pytest.raises(capi.AcmmpError):
        capi.keep_mask_bytes(0, 100)
