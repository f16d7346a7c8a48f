"""The device-side optimizer (ccvpe_amd/optim.py device path, csrc/optim.hip) against torch's own optimizers run live on the
CPU with the same synthetic gradients: AdamW / L2 weight decay, the device hyper rows, the global gradient norm, clipping,
the skipped non-finite step and state-dict interchange.

Shapes: those of test_adam_matches_torch_adam plus (4096,) and (1,) - a chunk tail, a tensor that is exactly one chunk, the
unaligned scalar path (numel % 4 != 0), 119 chunks in one tensor, and one tensor (index 1) that never gets a gradient."""
import copy
import functools
import math

import pytest
import torch

from ccvpe_amd import synth

pytestmark = pytest.mark.gpu

SHAPES = [(160, 336, 3, 3), (17,), (1, 10, 1, 1), (4099,), (96, 1, 5, 5), (4096,), (1,)]
NO_GRAD, LATE = 1, 5          # never receives a gradient / starts receiving them at step 3
BIG = (4300000,)              # 1 050 chunks: the prepare kernel's lane-strided pass over the partials loops 5 times


@functools.lru_cache(maxsize=None)
def _init(i, shape=None):
    return synth.normal(shape or SHAPES[i], 2000 + i, 0.1)


@functools.lru_cache(maxsize=None)
def _grad(i, step, shape=None):
    return synth.normal(shape or SHAPES[i], 3000 + 10 * step + i, 1e-3 * (1 + i))


def _groups(ps):
    """Two groups with different lr, betas and weight_decay; the second excludes its tensors from the decay."""
    return [dict(params=ps[:4], weight_decay=0.05), dict(params=ps[4:], lr=3e-3, betas=(0.8, 0.99), weight_decay=0.0)]


def _fresh(device=None):
    return [torch.nn.Parameter(_init(i).clone().to(device or "cpu")) for i in range(len(SHAPES))]


def _has_grad(i, step):
    return i != NO_GRAD and not (i == LATE and step < 3)


def _set_grads(ps, step, in_place, scale=1.0, clear=True):
    for i, p in enumerate(ps):
        if not _has_grad(i, step):
            if clear:
                p.grad = None
            continue
        g = _grad(i, step) * scale
        if in_place and p.grad is not None:
            p.grad.copy_(g)                       # the static-address case: the device tables are NOT rebuilt
        else:
            p.grad = g.to(p.device)


def _assert_close(ref_p, our_p, base=None):
    """The project's rule (test_adam_matches_torch_adam): per tensor, d <= 2e-3 * (how far the reference moved) + 1e-9."""
    for i, (a, b) in enumerate(zip(ref_p, our_p)):
        a, b = a.detach().cpu(), b.detach().cpu()
        d = (a - b).abs().max().item()
        moved = (a - (_init(i) if base is None else base[i])).abs().max().item()
        assert d <= 2e-3 * moved + 1e-9, (i, d, moved)


@functools.lru_cache(maxsize=None)
def _torch_reference(kind, steps=5):
    """torch.optim.AdamW / Adam (L2 decay) on the CPU, 5 steps with a StepLR: final parameters and step counts."""
    ps = _fresh()
    opt = (torch.optim.AdamW if kind == "adamw" else torch.optim.Adam)(_groups(ps), lr=1e-3)
    sched = torch.optim.lr_scheduler.StepLR(opt, step_size=2, gamma=0.5)
    for step in range(steps):
        _set_grads(ps, step, False)
        opt.step()
        sched.step()
    return [p.detach() for p in ps], {i: float(opt.state[p]["step"]) for i, p in enumerate(ps) if len(opt.state[p])}


@pytest.mark.parametrize("capturable", [False, True])
@pytest.mark.parametrize("kind", ["adamw", "adam_l2"])
def test_weight_decay_matches_torch(kind, capturable):
    from ccvpe_amd import optim
    ref_p, ref_steps = _torch_reference(kind)
    ps = _fresh("cuda")
    ours = (optim.AdamW if kind == "adamw" else optim.Adam)(_groups(ps), lr=1e-3, capturable=capturable)
    sched = torch.optim.lr_scheduler.StepLR(ours, step_size=2, gamma=0.5)
    for step in range(5):
        _set_grads(ps, step, in_place=capturable)
        ours.step()
        sched.step()
    torch.cuda.synchronize()
    _assert_close(ref_p, ps)
    assert torch.equal(ps[NO_GRAD].detach().cpu(), _init(NO_GRAD))                  # bit-untouched
    got = {i: float(ours.state[p]["step"]) for i, p in enumerate(ps) if len(ours.state.get(p, ()))}
    assert got == ref_steps and got[LATE] == 2.0 and got[0] == 5.0 and NO_GRAD not in got
    if capturable:
        assert all(ours.state[p]["step"].is_cuda and ours.state[p]["step"].dtype == torch.float32 for p in ps if len(ours.state.get(p, ())))


def test_device_hyper_rows_match_the_host_formula():
    """Steps 1..6, betas (0.9, 0.999) and (0.8, 0.99): the rows adam_prepare_kernel derives against optim.Adam._hyper_row (the
    host path's formula, Python floats = double).  Both round ONE double to fp32; the device's beta^step (repeated squaring)
    may differ from libm's pow in its last double bits, which can move the rounded float by one place at most: <= 1 ulp."""
    from ccvpe_amd import optim
    ps = [torch.nn.Parameter(_init(2).clone().cuda()), torch.nn.Parameter(_init(3).clone().cuda())]
    cfg = [dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.05), dict(lr=3e-3, betas=(0.8, 0.99), eps=1e-6, weight_decay=0.0)]
    for cls in (optim.AdamW, optim.Adam):
        ours = cls([dict(params=[p], **c) for p, c in zip(ps, cfg)], capturable=True)
        for k in range(1, 7):
            for i, p in zip((2, 3), ps):
                p.grad = _grad(i, k).cuda()
            ours.step()
            rows = ours._dev["lay"]["dev"]["hyper"].cpu()
            for t, c in enumerate(cfg):
                want = optim.Adam._hyper_row(c["lr"], c["betas"][0], c["betas"][1], c["eps"], float(k)) + optim.Adam._decay_of(ours.param_groups[t])
                want = torch.tensor(want, dtype=torch.float64).to(torch.float32)
                ulps = (rows[t, :9].view(torch.int32) - want.view(torch.int32)).abs()
                assert int(ulps.max()) <= 1, (cls.__name__, k, t, rows[t].tolist(), want.tolist())
                assert int(ulps[[1, 2, 3, 4, 5, 7, 8]].max()) == 0            # no pow in these: the same double, the same float
            assert [float(ours.state[p]["step"]) for p in ps] == [float(k)] * 2


def _norm64(grads, scale):
    return math.sqrt(sum(float((g.double() * scale).pow(2).sum()) for g in grads))


def test_global_norm_matches_float64_and_is_deterministic():
    """last_grad_norm against the float64 norm of the same gradients, relative error <= 1e-5.

    Derivation from the kernels as built (csrc/optim.hip).  One fp32 partial per 4 096-element chunk: each lane adds at most
    16 squares on one accumulator (the scalar path; 4 per accumulator on the 16-byte path), 2 additions merge the four
    accumulators, 6 butterfly steps the wave, 2 the four waves: <= 26 dependent fp32 additions.  The partials are then summed in
    DOUBLE (lane-strided + LDS tree), which adds nothing at this scale.  Each term carries <= 1.5 ulp from scaling and squaring.
    With u = 2^-24 = 6e-8 the sum is within (26 + 1.5) u = 1.7e-6 relative - under the 6e-6 that 100 dependent additions would
    give - the norm within half of that plus one rounding of the square root: < 1e-6, a factor 10 inside the bound."""
    from ccvpe_amd import optim
    ps = _fresh("cuda") + [torch.nn.Parameter(_init(7, BIG).clone().cuda())]
    grads = {i: _grad(i, 0, BIG if i == 7 else None) for i in range(8) if i != NO_GRAD}
    for i, g in grads.items():
        ps[i].grad = g.cuda()
    ours = optim.Adam(ps, lr=1e-5, skip_nonfinite=True)                  # the norm pass without clipping
    seen = []
    for scale in (1.0, 1.0, 0.25):                                       # grad_scale is applied INSIDE the norm
        ours.grad_scale = scale
        ours.step()
        seen.append(ours.last_grad_norm.clone())
    torch.cuda.synchronize()
    assert ours._layout["chunk_tensor"].numel() > 1024 + 119              # several passes of the final reduction
    assert seen[0].view(torch.int32).item() == seen[1].view(torch.int32).item()      # two runs: the same bits
    for got, scale in ((seen[0], 1.0), (seen[2], 0.25)):
        want = _norm64(grads.values(), scale)
        rel = abs(float(got) - want) / want
        print("global norm: got %.9g want %.9g rel %.3g" % (float(got), want, rel))
        assert rel <= 1e-5, (float(got), want, rel)
    assert float(ours.skipped_steps) == 0.0
    # a tensor without a gradient contributes 0: drop the big one, the norm is that of the rest
    ps[7].grad = None
    ours.grad_scale = 1.0
    ours.step()
    want = _norm64([g for i, g in grads.items() if i != 7], 1.0)
    assert abs(float(ours.last_grad_norm) - want) / want <= 1e-5
    assert float(ours.state[ps[7]]["step"]) == 3.0 and float(ours.state[ps[0]]["step"]) == 4.0


@functools.lru_cache(maxsize=None)
def _clip_reference(max_norm, steps=3):
    """torch.nn.utils.clip_grad_norm_ then torch.optim.AdamW, on the CPU."""
    ps = _fresh()
    opt = torch.optim.AdamW(_groups(ps), lr=1e-3)
    norms = []
    for step in range(steps):
        _set_grads(ps, step + 3, False)
        norms.append(float(torch.nn.utils.clip_grad_norm_(ps, max_norm)))
        opt.step()
    return [p.detach() for p in ps], norms


def _clip_run(max_norm, steps=3):
    from ccvpe_amd import optim
    ps = _fresh("cuda")
    ours = optim.AdamW(_groups(ps), lr=1e-3, capturable=True, max_grad_norm=max_norm)
    norms = []
    for step in range(steps):
        _set_grads(ps, step + 3, in_place=True)
        ours.step()
        norms.append(float(ours.last_grad_norm))
    torch.cuda.synchronize()
    return ps, norms, ours


def test_clipping_matches_clip_grad_norm_then_adamw():
    n0 = _norm64([_grad(i, 3) for i in range(len(SHAPES)) if i != NO_GRAD], 1.0)
    max_norm = n0 / 10                                                   # the norm is about 10 x max_grad_norm: clipped
    ref_p, ref_norms = _clip_reference(max_norm)
    ps, norms, ours = _clip_run(max_norm)
    _assert_close(ref_p, ps)
    for a, b in zip(norms, ref_norms):
        assert abs(a - b) <= 1e-5 * b and b > 5 * max_norm, (a, b)
    assert float(ours._scalars[1]) < 0.2 and float(ours.skipped_steps) == 0.0


def test_unclipped_norm_clamps_to_one_and_changes_no_bit():
    n0 = _norm64([_grad(i, 3) for i in range(len(SHAPES)) if i != NO_GRAD], 1.0)
    max_norm = 2 * n0 * 1.3                                              # above every step's norm: the coefficient clamps to 1
    ref_p, ref_norms = _clip_reference(max_norm)
    assert max(ref_norms) < max_norm
    ps, norms, ours = _clip_run(max_norm)
    _assert_close(ref_p, ps)
    assert float(ours._scalars[1]) == 1.0
    plain, _, _ = _clip_run(None)                                        # the same device optimizer with clipping off
    for a, b in zip(ps, plain):
        assert torch.equal(a.detach(), b.detach())


@functools.lru_cache(maxsize=None)
def _first_step_reference():
    ps = _fresh()
    opt = torch.optim.AdamW(_groups(ps), lr=1e-3)
    _set_grads(ps, 3, False)
    opt.step()
    return [p.detach() for p in ps]


@pytest.mark.parametrize("bad,kw", [(float("inf"), dict(skip_nonfinite=True)), (float("nan"), dict(max_grad_norm=1e9))])
def test_nonfinite_step_is_skipped_whole(bad, kw):
    """DELIBERATE departure from torch (optim.py): clip_grad_norm_ + step() would write NaN into the weights; here the step
    is skipped - parameters, both moments and every step count keep their bits - and counted."""
    from ccvpe_amd import optim
    ps = _fresh("cuda")
    ours = optim.AdamW(_groups(ps), lr=1e-3, **kw)

    def snapshot():
        """(parameters, first moments, second moments, [step counts]) as bit patterns"""
        torch.cuda.synchronize()
        have = [p for p in ps if len(ours.state.get(p, ()))]
        bits = lambda ts: [t.detach().clone().view(torch.int32) for t in ts]
        return (bits(ps), bits(ours.state[p]["exp_avg"] for p in have), bits(ours.state[p]["exp_avg_sq"] for p in have),
                bits([ours._steps]))

    def same(a, b):
        return all(len(u) == len(v) and all(torch.equal(x, y) for x, y in zip(u, v)) for u, v in zip(a, b))

    _set_grads(ps, 3, in_place=True)
    ps[3].grad[1234] = bad
    ours.step()
    snap = snapshot()
    assert all(torch.equal(p.detach().cpu(), _init(i)) for i, p in enumerate(ps))
    assert all(int(m.abs().max()) == 0 for m in snap[1] + snap[2] + snap[3]) and len(snap[1]) == len(SHAPES) - 1
    assert float(ours.skipped_steps) == 1.0 and not math.isfinite(float(ours.last_grad_norm))
    _set_grads(ps, 3, in_place=True)                                     # the next, finite, step is torch's FIRST step
    ours.step()
    _assert_close(_first_step_reference(), ps)
    assert float(ours.skipped_steps) == 1.0 and float(ours.state[ps[0]]["step"]) == 1.0
    before = snapshot()                                                  # and with non-trivial moments: still not one bit moves
    ps[0].grad[0, 0, 0, 0] = bad
    ours.step()
    assert same(before, snapshot()) and float(ours.skipped_steps) == 2.0


def test_capturable_state_dict_interchanges_with_torch():
    from ccvpe_amd import optim
    ps = _fresh("cuda")
    ours = optim.AdamW(_groups(ps), lr=1e-3, capturable=True)
    for step in range(2):
        _set_grads(ps, step + 3, in_place=True)
        ours.step()
    sd = ours.state_dict()
    assert sd["state"][0]["step"].is_cuda and sd["state"][0]["step"].dtype == torch.float32 and float(sd["state"][0]["step"]) == 2.0
    assert NO_GRAD not in sd["state"]
    base = [p.detach().clone() for p in ps]
    twin_p = [torch.nn.Parameter(b.clone()) for b in base]
    twin = optim.AdamW(_groups(twin_p), lr=1e-3, capturable=True)
    twin.load_state_dict(copy.deepcopy(sd))             # (load_state_dict may alias the tensors it is given)
    ref_p = [torch.nn.Parameter(b.clone()) for b in base]
    ref = torch.optim.AdamW(_groups(ref_p), lr=1e-3, capturable=True)   # torch's own capturable AdamW, on the device
    ref.load_state_dict(copy.deepcopy(sd))
    for group in (ps, twin_p, ref_p):
        _set_grads(group, 5, in_place=False, clear=False)
    ours.step(); twin.step(); ref.step()
    torch.cuda.synchronize()
    for a, b in zip(ps, twin_p):
        assert torch.equal(a.detach(), b.detach())                        # continues identically
    _assert_close(ref_p, ps, base=[b.cpu() for b in base])
    # the re-bound step views advanced, and they ARE the flat device array the prepare kernel increments
    assert float(twin.state[twin_p[0]]["step"]) == 3.0 and float(twin._steps[0]) == 3.0
    assert twin.state[twin_p[0]]["step"].data_ptr() == twin._steps.data_ptr()
    assert float(ref.state[ref_p[0]]["step"]) == 3.0 and float(ours.state[ps[LATE]]["step"]) == 3.0
    # and the other way: torch's capturable state loads into ours
    back = optim.AdamW(_groups(twin_p), lr=1e-3, capturable=True)
    back.load_state_dict(copy.deepcopy(ref.state_dict()))
    assert float(back.state[twin_p[0]]["step"]) == 3.0


def test_step_subset_is_refused_on_the_device_path():
    from ccvpe_amd import optim
    ps = _fresh("cuda")
    for kw in (dict(max_grad_norm=1.0), dict(capturable=True)):
        with pytest.raises(ValueError):
            optim.AdamW(ps, **kw).step_subset(ps[:2])
