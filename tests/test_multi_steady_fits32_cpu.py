"""The host's size check for the packed split kernel's steady loop (32-bit
byte offsets over the action ring and the done / winner rows): the
arithmetic alone, no device.  A ring past 4 GiB is not reached on the GPU in
a test's time and memory, so the refusal is checked here: such a launch keeps
the generic tick's 64-bit addressing.
"""
import ctypes

import pytest


@pytest.fixture(scope="module")
def fits():
    import skillshot_learning_amd as m
    L = m.load_library()
    f = L.skdiag_split_steady_fits32
    f.argtypes = [ctypes.c_int64] * 4
    f.restype = ctypes.c_int
    return lambda n, ring, out_slabs, out_stride: bool(f(n, ring, out_slabs, out_stride))


def test_the_benchmark_shapes_fit(fits):
    assert fits(65536, 400, 400, 0)
    assert fits(65536, 4000, 4000, 65536)
    assert fits(98304, 400, 400, 98304)
    assert fits(1, 1, 1, 0)


def test_ring_bytes_must_fit_32_bits(fits):
    # ring_slabs * 16 * n <= 2^32 - 1
    assert fits(65536, 4095, 1, 0)
    assert not fits(65536, 4096, 1, 0)       # exactly 2^32
    assert not fits(98304, 4000, 1, 0)
    assert fits(1, (2 ** 32 - 1) // 16, 1, 0)
    assert not fits(1, (2 ** 32 - 1) // 16 + 1, 1, 0)
    assert not fits(2 ** 28, 1, 1, 0)        # one slab alone is 2^32 bytes
    assert not fits(2 ** 40, 1, 1, 0)
    assert not fits(65536, 2 ** 62, 1, 0)    # no wrap in the product


def test_output_rows_must_fit_32_bits(fits):
    n = 65536
    # out_slabs * out_stride + n <= 2^32 - 1
    assert fits(n, 1, 65534, n)
    assert not fits(n, 1, 65535, n)
    assert fits(n, 1, 2 ** 31 - 1, 0)        # last row only: the stride is 0
    assert not fits(n, 1, 2 ** 31, 0)        # the row position must fit an int
    assert not fits(n, 1, 2 ** 40, 2 ** 40)


def test_bad_sizes_do_not_fit(fits):
    assert not fits(0, 1, 1, 0)
    assert not fits(1, 0, 1, 0)
    assert not fits(1, 1, 0, 0)
    assert not fits(1, 1, 1, -1)
