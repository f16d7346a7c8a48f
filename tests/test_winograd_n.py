"""The gate of conv3x3_wino_n_kernel (csrc/conv3x3_wino_n.hip) on the host: which descriptors ccvpe_conv3x3_wino_n_ok and
ccvpe_conv3x3_wino_match1_ok serve (0 = not, 1 = computed correctly, 2 = also a launch the route takes), the setter behind
CCVPE_WINO_N=0, and that the entry points are registered for planned forwards."""
import ctypes

import pytest

from ccvpe_amd import _lib, plan
from ccvpe_amd._lib import ConvDesc


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def _desc(c0=40, n=40, hw=256, batch=64, ldd=None, ld0=None, **over):
    d = ConvDesc()
    d.src0, d.w, d.dst = 0x10000, 0x20000, 0x30000
    d.c0, d.ld0, d.c1, d.ld1 = c0, ld0 if ld0 is not None else c0, 0, 0
    d.batch, d.in_h, d.in_w = batch, hw, hw
    d.kh, d.kw, d.stride, d.pad = 3, 3, 1, 1
    d.n, d.kpad = n, 16 * (-(-c0 // 16) * 16)
    d.ldd, d.ldres = ldd if ldd is not None else n, 0
    d.act, d.out_mode = 0, 0
    for k, v in over.items():
        setattr(d, k, v)
    return d


def test_conv_gate(lib):
    ok = lambda **k: lib.ccvpe_conv3x3_wino_n_ok(ctypes.byref(_desc(**k)))
    for c, hw in ((80, 128), (40, 256)):                             # B = 64 and B = 8: the levels the probe showed a win at
        assert ok(c0=c, n=c, hw=hw) == 2 and ok(c0=c, n=c, hw=hw, batch=8) == 2, (c, hw)
    for c, hw in ((64, 128), (32, 256)):                             # no padded column block to remove: measured slower, not routed
        assert ok(c0=c, n=c, hw=hw) == 1, (c, hw)
    assert ok(c0=80, n=80, hw=128, batch=4) == 1                     # below the smallest launches that won
    assert ok(c0=40, n=40, hw=256, batch=4) == 1
    assert ok(c0=48, n=40, hw=16, batch=2) == 1                      # computed correctly, below the Winograd route's size rule
    assert ok(c0=40, n=40, hw=18, batch=2, ldd=44, ld0=44) == 1
    assert ok(c0=160, n=160, hw=64) == 0                             # n > 80
    assert ok(c0=32, n=16, hw=256) == 0                              # n <= 16
    assert ok(c0=16, n=40, hw=256) == 0                              # c0 < 32
    assert ok(hw=17) == 0                                            # odd H / W
    assert ok(ldd=42) == 0                                           # ldd % 4
    assert ok(kpad=9 * 48) == 0                                      # not the U pack
    assert ok(src0=0x10004) == 0                                     # misaligned
    assert ok(act=1) == 0 and ok(stride=2) == 0 and ok(c1=8) == 0
    assert lib.ccvpe_conv3x3_wino_n_ok(None) == 0
    # the old kernel's own query is unchanged by the split of its rule
    assert lib.ccvpe_conv3x3_wino_ok(ctypes.byref(_desc())) == 1
    assert lib.ccvpe_conv3x3_wino_ok(ctypes.byref(_desc(hw=16, batch=2))) == 0


def test_match_gate(lib):
    ok = lambda L, **k: lib.ccvpe_conv3x3_wino_match1_ok(ctypes.byref(_desc(**k)), 1, L)
    assert ok(40, c0=80, n=80, hw=128, ldd=88) == 2
    assert ok(20, c0=40, n=40, hw=256, ldd=48) == 2
    assert ok(40, c0=40, n=40, hw=16, batch=2, ldd=48) == 1
    assert ok(40, c0=40, n=40, hw=256, ldd=40) == 0                  # no room for the score column
    assert ok(41, c0=40, n=40, hw=256, ldd=48) == 0                  # L > n
    assert ok(0, c0=40, n=40, hw=256, ldd=48) == 0
    assert ok(40, c0=160, n=160, hw=64, ldd=168) == 0


def test_setter_caps_the_route(lib):
    d = _desc()
    prev = lib.ccvpe_set_wino_n(0)
    try:
        assert lib.ccvpe_conv3x3_wino_n_ok(ctypes.byref(d)) == 1
        assert lib.ccvpe_conv3x3_wino_match1_ok(ctypes.byref(_desc(ldd=48)), 1, 40) == 1
        assert lib.ccvpe_set_wino_n(1) == 0
        assert lib.ccvpe_conv3x3_wino_n_ok(ctypes.byref(d)) == 2
    finally:
        lib.ccvpe_set_wino_n(prev)


def test_registered_for_plans():
    for name in ("ccvpe_conv3x3_wino_n_f32", "ccvpe_conv3x3_wino_match1_f32"):
        assert name in plan.LAUNCHES
    for name in ("ccvpe_conv3x3_wino_n_ok", "ccvpe_conv3x3_wino_match1_ok"):
        assert name in plan.QUERIES
