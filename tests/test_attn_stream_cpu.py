"""The forward bound of the streaming attention tests, checked without a GPU (the role tests/test_gemm_bounds_cpu.py plays for the GEMM bounds):
a torch emulation of the kernel's rounding points — bf16 P, fp32 online rescale, bf16 output — meets the bound on the GPU test's seeded
inputs, and the same emulation with the last key tile dropped, or with the O rescale left out at one tile, does not."""
import pytest
import torch

import attn_stream_ref as R

CASES = [(1, 577, 2, 32), (1, 1370, 2, 64)]


@pytest.mark.parametrize("geom", CASES)
def test_emulated_streaming_forward_meets_the_bound(geom):
    B, T, H, hd = geom
    qkv, dout = R.inputs(B, T, H, hd)
    ref, lse_ref, pabsv, _ = R.reference(qkv, dout, B, T, H, hd, backward=False)
    out, lse = R.emulate_stream_fwd(qkv, B, T, H, hd)
    excess, ratio = R.fwd_excess(out, ref, pabsv)
    print(f"emulated streaming forward {geom}: max |err| / (2^-9 (sum P|V| + |ref|)) = {ratio:.3f}, against the bound {excess:.3f}")
    assert excess <= 1.0, (geom, excess, ratio)
    assert float((lse.double() - lse_ref).abs().max()) <= 1e-3


@pytest.mark.parametrize("geom", CASES)
@pytest.mark.parametrize("bug", ["last key tile dropped", "no rescale at tile 1"])
def test_the_bound_sees_a_dropped_tile_and_a_missing_rescale(geom, bug):
    B, T, H, hd = geom
    qkv, dout = R.inputs(B, T, H, hd)
    ref, _, pabsv, _ = R.reference(qkv, dout, B, T, H, hd, backward=False)
    out, _ = R.emulate_stream_fwd(qkv, B, T, H, hd, drop_last_tile=bug.startswith("last"), no_rescale_tile=1 if bug.startswith("no") else None)
    excess, ratio = R.fwd_excess(out, ref, pabsv)
    print(f"{bug} {geom}: max |err| / (2^-9 (sum P|V| + |ref|)) = {ratio:.3f}, against the bound {excess:.3f}")
    assert excess > 1.0, (geom, bug, excess)
