"""Winograd F(2x2,3x3) for the fp32 convK.2 layers (csrc/conv3x3_wino.hip), on the CPU: the packed transformed weights
against a numpy definition, and an fp64 emulation of the kernel's tile algorithm (transforms, component order, padding)
against a direct convolution."""
import numpy as np
import torch

from ccvpe_amd import models

G = np.array([[1, 0, 0], [0.5, 0.5, 0.5], [0.5, -0.5, 0.5], [0, 0, 1]], dtype=np.float64)
BT = np.array([[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]], dtype=np.float64)
AT = np.array([[1, 1, 1, 0], [0, 1, -1, -1]], dtype=np.float64)


def _round_up(v, m):
    return (v + m - 1) // m * m


def _direct(x, w, bias):
    """x [B,H,W,C], w [N,C,3,3] (OIHW), stride 1, pad 1 -> [B,H,W,N] in fp64."""
    b, h, wd, c = x.shape
    xp = np.zeros((b, h + 2, wd + 2, c))
    xp[:, 1:-1, 1:-1] = x
    out = np.zeros((b, h, wd, w.shape[0])) + bias
    for ky in range(3):
        for kx in range(3):
            out += xp[:, ky:ky + h, kx:kx + wd] @ w[:, :, ky, kx].T
    return out


def _wino_emulated(x, u_packed, n, c, bias):
    """The kernel's arithmetic in fp64: V = B^T d B per 2x2 tile and channel, M_xi = V_xi @ U_xi over channels, Y = A^T M A."""
    b, h, wd, _ = x.shape
    cp = _round_up(c, 16)
    u = u_packed.reshape(-1, 16, cp)[:n, :, :c]                       # [N][xi][C]
    xp = np.zeros((b, h + 2, wd + 2, c))
    xp[:, 1:-1, 1:-1] = x
    out = np.zeros((b, h, wd, n))
    for ty in range(h // 2):
        for tx in range(wd // 2):
            d = xp[:, 2 * ty:2 * ty + 4, 2 * tx:2 * tx + 4]           # [B][4][4][C]
            v = np.einsum("ik,bklc,jl->bijc", BT, d, BT).reshape(b, 16, c)
            m = np.einsum("bxc,nxc->bxn", v, u).reshape(b, 4, 4, n)
            out[:, 2 * ty:2 * ty + 2, 2 * tx:2 * tx + 2] = np.einsum("ik,bkln,jl->bijn", AT, m, AT) + bias
    return out


def test_packed_u_matches_numpy_definition():
    rng = np.random.default_rng(0)
    for n, c in ((40, 40), (64, 32), (33, 20)):
        w = rng.standard_normal((n, c, 3, 3))
        u = models._pack_wino(torch.from_numpy(w).float())
        assert u.dtype == torch.float32 and u.shape == (_round_up(n, 32), 16 * _round_up(c, 16))
        ref = np.einsum("ak,ockl,bl->oabc", G, w.astype(np.float32).astype(np.float64), G)   # [N][4][4][C], fp64
        got = u.numpy().reshape(-1, 4, 4, _round_up(c, 16))
        np.testing.assert_array_equal(got[:n, :, :, :c], ref.astype(np.float32))       # one rounding, from fp64
        assert not got[n:].any() and not got[:, :, :, c:].any()                          # zero padding


def test_bf16_and_missing_packs():
    assert models._pack_wino(torch.zeros(8, 8, 3, 3), torch.bfloat16) is None


def test_tile_algorithm_equals_direct_conv_fp64():
    rng = np.random.default_rng(1)
    for b, h, wd, c, n in ((2, 6, 8, 24, 12), (1, 4, 4, 40, 40)):
        x = rng.standard_normal((b, h, wd, c))
        w = rng.standard_normal((n, c, 3, 3))
        bias = rng.standard_normal(n)
        # U in fp64 (the same packing, before its fp32 rounding) so that the comparison isolates the algorithm
        g = np.einsum("ak,ockl,bl->oabc", G, w, G)
        up = np.zeros((_round_up(n, 32), 4, 4, _round_up(c, 16)))
        up[:n, :, :, :c] = g
        got = _wino_emulated(x, up.reshape(up.shape[0], -1), n, c, bias)
        np.testing.assert_allclose(got, _direct(x, w, bias), rtol=1e-12, atol=1e-11)
