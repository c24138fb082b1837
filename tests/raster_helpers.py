"""What the tests of the raster blocks and the output maps share (a plain module, no fixtures)."""
import numpy as np
import pytest


def bits(a):
    """the bit patterns of a 4- or 8-byte float array; an integer array as it is"""
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def need_glibc_set(product):
    if product.lib.sf3d_libm_set() != 1:
        pytest.skip("this build evaluates the 0.50-ulp routines, not the C library's bits (-DSF3D_LIBM_GLIBC=0): bit identity with the compiled reference is not its contract")
