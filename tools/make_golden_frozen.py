"""Frozen-BatchNorm fixtures from the REFERENCE: tests/golden/fwd_vigor_frozenbn.npz, grad_vigor_frozenbn*.npz and
grad_vigor_frozenbn_f64*.npz.

The reference's fine-tuning idiom: `model.train()`, then `.eval()` on every BatchNorm2d — running statistics normalise and
stay untouched, drop_connect stays active.  Same case as the train-mode parity fixtures of tools/make_golden.py
(golden_util.TRAIN_CASE: CVM_VIGOR, B = 2, pair seed 2024, the injected drop_connect draws, golden_util.train_loss).
The float64 file is autograd through the ORACLE (train_stats=None: running statistics; drop_scales applied), the
round-off-free value of what the reference computes in fp32.  Runs only where the reference is present.  Usage:
    python tools/make_golden_frozen.py      (CPU, about a minute)
"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from ref_import import import_reference          # noqa: E402
from ccvpe_amd import synth                       # noqa: E402
import golden_util as G                           # noqa: E402
import frozen_bn_util as FZ                       # noqa: E402
from make_golden import save                      # noqa: E402
from oracle import ccvpe_oracle as O              # noqa: E402


def main():
    torch.set_num_threads(8)
    ref_models, _ = import_reference()
    import efficientnet_pytorch.model as effmodel
    c = G.TRAIN_CASE
    sd = synth.synthetic_state_dict(c["kind"], c["wseed"])
    masks, scales, skip = G.train_drop_masks(c["batch"])
    order = [("grd_efficientnet", i) for i in skip] + [("sat_efficientnet", i) for i in skip]
    calls = []

    def injected_drop_connect(inputs, p, training):
        assert training, "drop_connect must stay active with the BatchNorms in eval()"
        key = order[len(calls)]
        calls.append(key)
        return inputs / (1 - p) * masks[key].view(-1, 1, 1, 1)

    # ---- the reference: .train(), every BatchNorm2d in .eval() ------------------------------------------------------
    net = ref_models.CVM_VIGOR("cpu", c["circular"])
    net.load_state_dict(sd, strict=True)
    net.train()
    n_bn = 0
    for m in net.modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            m.eval()
            n_bn += 1
    before = FZ.buffers_of(net.state_dict())
    grd, sat = synth.synthetic_pair(c["batch"], c["grd"], c["pseed"])
    real_dc = effmodel.drop_connect
    effmodel.drop_connect = injected_drop_connect
    try:
        out = net(grd, sat)
    finally:
        effmodel.drop_connect = real_dc
    assert len(calls) == len(order), "%d of %d injected draws consumed" % (len(calls), len(order))
    G.train_loss(out).backward()
    after = net.state_dict()
    assert all(torch.equal(after[k], v) for k, v in before.items()), "a frozen BatchNorm buffer changed"
    print("%d BatchNorm2d frozen, %d buffers bit-identical, %d draws" % (n_bn, len(before), len(calls)))
    ref_g = G.summarize_grads([(n, p.grad) for n, p in net.named_parameters()])
    save("fwd_vigor_frozenbn", G.summarize_forward([t.detach() for t in out]))
    FZ.save_grads("grad_vigor_frozenbn", ref_g)
    ref_logits = out[0].detach().double()

    # ---- float64 autograd through the oracle ------------------------------------------------------------------------
    params = {}
    for k, v in sd.items():
        if v.is_floating_point():
            v = v.double()
            params[k] = v.clone().requires_grad_(True) if "running_" not in k else v.clone()
        else:
            params[k] = v.clone()
    scales64 = {e: {i: m.double() for i, m in d.items()} for e, d in scales.items()}
    out64 = O.forward(params, grd.double(), sat.double(), c["kind"], c["circular"], None, train_stats=None,
                      drop_scales=scales64)
    G.train_loss(out64).backward()
    names = set(str(n) for n in ref_g["names"])
    f64_g = G.summarize_grads([(k, v.grad) for k, v in params.items() if k in names])
    assert [str(n) for n in f64_g["names"]] == [str(n) for n in ref_g["names"]]
    FZ.save_grads("grad_vigor_frozenbn_f64", f64_g)

    # ---- what the tests' bounds rest on -----------------------------------------------------------------------------
    bad, med = G.compare_grads(ref_g, f64_g)
    rel = G.grad_rel_errors(ref_g, f64_g)
    worst = max(rel, key=rel.get)
    print("tensors with a gradient: %d (%d at noise level)" % (len(ref_g["names"]), len(ref_g["names"]) - len(rel)))
    print("reference fp32 vs float64: median %.3e, max %.3e (%s); compare_grads: %s" % (med, rel[worst], worst, bad))
    print("reference logits vs float64 oracle: %.3e of max |logit|" % (
        float((ref_logits - out64[0].detach()).abs().max() / out64[0].detach().abs().max())))


if __name__ == "__main__":
    main()
