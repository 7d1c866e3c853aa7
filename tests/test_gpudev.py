"""tests/gpudev.py itself: the byte comparer on the CPU, and the guard protocol and close() on a device."""
import numpy as np
import pytest

import gpudev
from gpudev import L  # noqa: F401  (fixture)

F32 = np.float32


def test_same_bytes():
    a = np.array([[0.5, np.nan, -0.0], [1.0, 2.0, 3.0]], dtype=F32)
    gpudev.same_bytes(a, a.copy(), "equal")  # a NaN is equal to itself by its bytes
    b = a.copy()
    b[0, 2], b[1, 1] = 0.0, 2.5
    with pytest.raises(AssertionError) as e:
        gpudev.same_bytes(a, b, "planes")
    msg = str(e.value)
    assert "planes: 2 of 6 words differ, first at [0, 2]" in msg and repr(a[0, 2]) in msg and repr(b[0, 2]) in msg
    with pytest.raises(AssertionError):
        gpudev.same_bytes(np.array([-0.0], dtype=F32), np.array([0.0], dtype=F32), "zeros")
    with pytest.raises(AssertionError):
        gpudev.same_bytes(a, a.reshape(3, 2), "shapes")
    with pytest.raises(AssertionError):
        gpudev.same_bytes(a, a.ravel()[:5], "sizes")


@pytest.mark.gpu
def test_guard_check_and_close(L):
    n, guard = 3, 64  # one pixel
    with gpudev.Device(L) as dev:
        plane = dev.alloc((n + guard) * 4)
        dev.fill_guarded(plane, n, guard, -3.0)
        dev.upload(plane, np.array([0.25, 0.5, 0.75], dtype=F32))
        assert dev.read_guarded(plane, n, guard, -3.0, "the plane").tolist() == [0.25, 0.5, 0.75]
        dev.upload(plane, np.array([7.0], dtype=F32), offset=(n + 5) * 4)  # one guard float, inside the allocation
        with pytest.raises(AssertionError, match="the plane was written past its 3 elements"):
            dev.read_guarded(plane, n, guard, -3.0, "the plane")
    assert dev.ctx is None and dev._owned == []  # the with block closed it: nothing is left to free
    dev.close()
