"""Registers and scratch of k_links_flush, read from the code object inside the built product library (no GPU needed; the method of
tests/test_kernel_resources.py).

k_links_flush adds the link flow sums of up to SF3D_LINKS_RING accepted steps in one pass: per node it holds ten sums across a loop over
the steps.  It replaces a launch of the per-step sums per accepted step, so it must stream as they do: nothing in scratch, and at least
the waves per SIMD that k_accept - the per-step form, which stays for SF3D_OVERLAP_ACCEPT=0 - has."""
import re

from tests.test_kernel_resources import VGPRS_PER_SIMD_LANE, _pick, kernels  # noqa: F401  (the fixture)


def _waves_per_simd(vgpr):
    granule = (vgpr + 7) // 8 * 8            # VGPRs are allocated in blocks of 8
    return min(8, VGPRS_PER_SIMD_LANE // granule)


def test_links_flush_streams_without_scratch_at_the_occupancy_of_k_accept(kernels):  # noqa: F811
    flush = _pick(kernels, r"^void k_links_flush<(true|false)>\(DevView, LinksBatch\)$")
    accept = _pick(kernels, r"^void k_accept<(true|false)>\(DevView\)$")
    assert len(flush) == 2 and len(accept) == 2, (list(flush), list(accept))
    for name, r in flush.items():
        nt = re.search(r"<(true|false)>", name).group(1)
        a = accept[f"void k_accept<{nt}>(DevView)"]
        print(name, r, "k_accept:", a)
        assert r["scratch"] == 0, (name, r)
        assert r["lds"] == 0, (name, r)
        assert _waves_per_simd(r["vgpr"]) >= _waves_per_simd(a["vgpr"]), (name, r, a)


def test_accept_boundary_with_the_head_copy_stays_small(kernels):  # noqa: F811
    """k_accept_boundary also copies the accepted head into the ring: still a plain stream, full occupancy, nothing in scratch"""
    for name, r in _pick(kernels, r"^k_accept_boundary\(DevView\)$").items():
        print(name, r)
        assert r["scratch"] == 0 and r["vgpr"] <= 64, (name, r)
