"""CPU-side checks of the three-plane pack of the early blocks' expand weights (models._pack_pw_s3 of the fp32 pack, read by
mbconv_front_s3_kernel in csrc/mbconv_front.hip) and of the host-only query ccvpe_mbconv_front_s3_ok."""
import torch

from ccvpe_amd import _lib, models, synth

# (cin, mid) of EfficientNet-B0's blocks 1, 2-3 and 4-5
SHAPES = ((16, 96), (24, 144), (40, 240))


def _w_exp(cin, mid):
    return models._pack_conv(synth.normal((mid, cin, 1, 1), 950 + cin, cin ** -0.5))


def test_planes_sum_exactly_to_the_fp32_expand_pack():
    for cin, mid in SHAPES:
        we = _w_exp(cin, mid)
        kpad = (cin + 15) // 16 * 16
        assert tuple(we.shape) == (mid, kpad)
        w3 = models._pack_pw_s3(we)
        assert w3.dtype == torch.bfloat16 and tuple(w3.shape) == (kpad // 16, mid, 48) and w3.is_contiguous()
        hi, mi, lo = models._unpack_pw_s3(w3)
        assert torch.equal((hi.double() + mi.double() + lo.double()).float(), we)          # exact: 8 + 8 + 8 significant bits
        assert torch.equal(hi, we.to(torch.bfloat16).float())                               # hi is the round-to-nearest bf16 of w
        assert we[:, :cin].abs().min() > 0                                                  # (the check below is about the padding only)


def test_padded_channels_are_zero_in_all_three_planes():
    for cin, mid in SHAPES:
        w3 = models._pack_pw_s3(_w_exp(cin, mid))
        for plane in models._unpack_pw_s3(w3):
            assert torch.count_nonzero(plane[:, cin:]) == 0
            assert cin % 16 == 0 or plane[:, cin:].shape[1] == 8
        # the same in the packed layout: block cin // 16, channels cin % 16 .. 15 of each 16-wide plane
        if cin % 16:
            last = w3[cin // 16].reshape(mid, 3, 16)
            assert torch.count_nonzero(last[:, :, cin % 16:]) == 0 and torch.count_nonzero(last[:, 0, :cin % 16]) == mid * (cin % 16)


def test_only_the_fp32_eval_pack_carries_the_early_blocks_packs():
    sd = synth.synthetic_state_dict("vigor", 0)
    pk = models._pack_model(sd, "vigor", 20, torch.float32, fold=True)
    for e in (pk.grd, pk.sat):
        have = [i for i, b in enumerate(e.blocks) if getattr(b, "w_exp3", None) is not None]
        assert have == [1, 2, 3, 4, 5]                                                      # the expanding blocks with Cin <= 48
        for i in have:
            b = e.blocks[i]
            assert tuple(b.w_exp3.shape) == ((b.cin + 15) // 16, b.mid, 48)
            assert torch.equal(sum(p.double() for p in models._unpack_pw_s3(b.w_exp3)).float(), b.w_exp)
    for other in (models._pack_model(sd, "vigor", 20, torch.float32, fold=False),
                  models._pack_model(sd, "vigor", 20, torch.bfloat16, fold=True)):
        for e in (other.grd, other.sat):
            assert all(getattr(b, "w_exp3", None) is None for b in e.blocks)


def test_ok_is_zero_for_shapes_the_kernel_does_not_serve():
    ok = _lib.load().ccvpe_mbconv_front_s3_ok
    assert ok(40, 80, 80, 480, 3, 1, 64) == 0                     # late block: mbconv_plane_kernel's
    assert ok(64, 64, 40, 240, 5, 2, 64) == 0                     # k5 s2 with Cin > 32: not instantiated for the fp32 kernel either
    assert ok(64, 64, 16, 96, 3, 1, 64) == 0                      # the 16-row tile form (Cin <= 16, stride 1): no B0 block
    assert ok(64, 64, 40, 240, 4, 1, 64) == 0 and ok(64, 64, 40, 240, 3, 3, 64) == 0
    for cin, k, s in ((16, 3, 2), (24, 3, 1), (24, 5, 2), (40, 5, 1), (40, 3, 2)):
        assert ok(20, 36, cin, 6 * cin, k, s, 2) >= 1
