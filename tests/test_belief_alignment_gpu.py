"""The 16-byte / scalar dispatch of the five belief steps (csrc/belief.hip: VEC of belief_step_kernel and of
belief_finish_kernel) is invisible in the results: a map that is 4-byte but not 16-byte aligned with w % 4 == 0 takes the scalar
forms and must give the bits of the vector forms.

Equality follows from the code: both staging forms write the same values into LDS, and both finish forms apply the same single
multiply per element.  So equality is the condition; there is no tolerance.

B = 2, 20 x 72, R = 3: two tile rows by two tile columns (16 x 64 tiles), w % 4 == 0, the second column tile partial.  Track 0
moves so that part of its prior leaves the grid; track 1 has its reset / cut flag set."""
import numpy as np
import pytest
import torch

import test_tracking_gpu as G
from ccvpe_amd import tracking as T

pytestmark = pytest.mark.gpu

B, H, W, R, OUTLIER = 2, 20, 72, 3, 0.02
STEPS = ["belief_step", "belief_step_rigid", "belief_viterbi_step", "belief_smooth_step", "belief_smooth_step_rigid"]
_SCENE = {}


def scene():
    """Computed once and shared (read-only, on the host)."""
    if not _SCENE:
        rng = np.random.default_rng(72)
        shift = np.array([[7.3, -30.6], [-1.2, 2.4]])
        offsets, taps = T.motion_taps_spec(shift, 1.0, R)
        _SCENE.update(maps=[G.softmax_maps(rng, B, H, W).reshape(B, 1, H, W) for _ in range(3)], ori=G.unit_ori(rng, B, H, W),
                      offsets=offsets, taps=taps, centred=T.motion_taps_spec(np.zeros((B, 2)), 1.0, R)[1],
                      motion=T.rigid_motion(shift, np.array([11.0, -4.0]), (H, W)), flags=np.array([0, 1], np.int32))
    return _SCENE


def _place(a, lead):
    """`a` on the device as a contiguous tensor that starts `lead` elements into a 16-byte aligned flat buffer."""
    a = torch.as_tensor(np.array(a))
    flat = torch.zeros((a.numel() + 4,), dtype=a.dtype, device="cuda")
    assert flat.data_ptr() % 16 == 0
    view = flat[lead:lead + a.numel()].view(a.shape)
    view.copy_(a)
    assert view.is_contiguous() and view.data_ptr() % 16 == 4 * lead
    return view


def run(name, lead_in, lead_out):
    """One call of ops.<name> with every input map `lead_in` and every output map `lead_out` floats off 16-byte alignment.
    Returns [the output maps as int32 bits ..., the rows as int64 bits]."""
    from ccvpe_amd import ops
    s = scene()
    rigid, smooth = name.endswith("rigid"), "smooth" in name
    a, heat, c = (_place(m, lead_in) for m in s["maps"])
    ori = _place(s["ori"], lead_in)
    move = _place(s["motion"] if rigid else s["offsets"], 0)
    taps = _place(s["centred"] if rigid else s["taps"], 0)
    flags = _place(s["flags"], 0)
    outs = [_place(np.zeros((B, 1, H, W), np.float32), lead_out) for _ in range(2 if smooth else 1)]
    if smooth:
        got = getattr(ops, name)(a, heat, c, ori, move, taps, outlier=OUTLIER, cut=flags, beta_out=outs[0], smooth=outs[1])
    else:
        got = getattr(ops, name)(a, heat, ori, move, taps, outlier=OUTLIER, reset=flags, post=outs[0])
    assert got[0].dtype == torch.float64 and got[0].data_ptr() % 8 == 0
    torch.cuda.synchronize()
    return [m.cpu().contiguous().view(torch.int32) for m in got[1:]] + [got[0].cpu().view(torch.int64)]


@pytest.mark.parametrize("name", STEPS)
def test_unaligned_maps_give_the_bits_of_aligned_maps(name):
    want = run(name, 0, 0)
    assert all(int(t.count_nonzero()) > 0 for t in want)
    for what, lead_in, lead_out in (("every map offset", 1, 1), ("output maps offset", 0, 1)):
        got = run(name, lead_in, lead_out)
        for k, (g, w) in enumerate(zip(got, want)):
            assert torch.equal(g, w), (name, what, "rows" if k == len(want) - 1 else "map %d" % k)
