"""CPU-side surface of the device-side optimizer (ccvpe_amd/optim.py, csrc/optim.hip): the constructors, the group defaults a
state dict carries, and the new C entry points' argument validation (tests/test_abi.py checks their prototypes against the
header and the .so once they are in _lib.PROTOTYPES)."""
import pytest
import torch

from ccvpe_amd import _lib, optim

NEW = ("ccvpe_adam_device_layout", "ccvpe_grad_sqnorm_f32", "ccvpe_adam_prepare_f32", "ccvpe_adam_update_f32")


def _params():
    return [torch.nn.Parameter(torch.zeros(3, 4)), torch.nn.Parameter(torch.zeros(5))]


def test_constructors_and_group_defaults():
    assert issubclass(optim.AdamW, optim.Adam) and issubclass(optim.Adam, torch.optim.Optimizer)
    a = optim.Adam(_params(), weight_decay=1e-2)
    assert a.defaults["weight_decay"] == 1e-2 and a.defaults["capturable"] is False and not a.capturable
    assert a.param_groups[0]["weight_decay"] == 1e-2 and a.param_groups[0]["decoupled_weight_decay"] is False
    c = optim.Adam(_params(), capturable=True)
    assert c.capturable and c.defaults["capturable"] is True and c.param_groups[0]["capturable"] is True
    assert c.defaults["weight_decay"] == 0
    w = optim.AdamW(_params())
    assert w.defaults["weight_decay"] == 1e-2 and w.defaults["decoupled_weight_decay"] is True       # torch.optim.AdamW's default
    p = _params()
    g = optim.AdamW([dict(params=p[:1]), dict(params=p[1:], weight_decay=0.0)], weight_decay=0.05, capturable=True)
    assert [q["weight_decay"] for q in g.param_groups] == [0.05, 0.0]                                 # bias / BatchNorm excluded by group
    # the global-norm options decide on the device whether the step counts advance: they imply the capturable state layout
    n = optim.AdamW(_params(), max_grad_norm=1.0)
    assert n.capturable and n.defaults["capturable"] is True and n.max_grad_norm == 1.0
    assert optim.Adam(_params(), skip_nonfinite=True).capturable
    assert n.last_grad_norm is None and n.skipped_steps is None                                       # before the first step
    sd = c.state_dict()
    assert sd["param_groups"][0]["capturable"] is True and sd["state"] == {}


def test_unsupported_options_still_raise():
    with pytest.raises(ValueError):
        optim.Adam(_params(), amsgrad=True)
    with pytest.raises(ValueError):
        optim.AdamW(_params(), amsgrad=True)
    with pytest.raises(ValueError):
        optim.Adam(_params(), weight_decay=-1.0)
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError):
            optim.Adam(_params(), max_grad_norm=bad)
    with pytest.raises(ValueError):                       # the global norm needs every gradient
        optim.AdamW(_params(), max_grad_norm=1.0).step_subset([])
    with pytest.raises(ValueError):
        optim.Adam(_params(), capturable=True).step_subset([])
    optim.Adam(_params()).step_subset([])                 # the default path's step_subset() is untouched (nothing to do here)


def test_graphed_train_step_refuses_a_host_path_optimizer():
    """The check comes before anything touches the GPU."""
    from ccvpe_amd import graph
    net = torch.nn.Linear(2, 2).train()
    with pytest.raises(ValueError, match="capturable=True"):
        graph.GraphedTrainStep(lambda: None, net, optimizer=optim.Adam(net.parameters()))


def test_new_entry_points_are_bound_and_reject_bad_arguments_without_a_gpu():
    for name in NEW:
        assert name in _lib.PROTOTYPES, name
    lib = _lib.load()
    EINVAL = -1
    assert lib.ccvpe_abi_version() == 7
    assert lib.ccvpe_adam_device_layout(0) >= lib.ccvpe_adam_hyper_floats() + 2        # the old row + l2 + decay
    assert lib.ccvpe_adam_device_layout(1) == 6 and lib.ccvpe_adam_device_layout(2) == 4
    assert lib.ccvpe_adam_device_layout(3) == EINVAL and b"adam_device_layout" in lib.ccvpe_last_error()
    P = 256                                               # fake aligned "pointers": never dereferenced
    nan, inf = float("nan"), float("inf")
    assert lib.ccvpe_grad_sqnorm_f32(None, P, P, 1, 1.0, P, None) == EINVAL
    assert b"grad_sqnorm" in lib.ccvpe_last_error()
    assert lib.ccvpe_grad_sqnorm_f32(P, P, P, 0, 1.0, P, None) == EINVAL               # no chunks
    assert lib.ccvpe_grad_sqnorm_f32(P, P, P, 1, 1.0, None, None) == EINVAL            # no partials
    assert lib.ccvpe_grad_sqnorm_f32(P, P, P, 1, inf, P, None) == EINVAL
    assert lib.ccvpe_adam_prepare_f32(P, None, P, P, 1, None, 0, 0.0, P, None) == EINVAL
    assert b"adam_prepare" in lib.ccvpe_last_error()
    assert lib.ccvpe_adam_prepare_f32(P, P, P, P, 0, None, 0, 0.0, P, None) == EINVAL  # no tensors
    assert lib.ccvpe_adam_prepare_f32(P, P, P, P, 1, None, 3, 0.0, P, None) == EINVAL  # partials counted but absent
    assert lib.ccvpe_adam_prepare_f32(P, P, P, P, 1, P, -1, 0.0, P, None) == EINVAL
    assert lib.ccvpe_adam_prepare_f32(P, P, P, P, 1, None, 0, 1.0, P, None) == EINVAL  # clipping without a norm pass
    assert b"norm partials" in lib.ccvpe_last_error()
    assert lib.ccvpe_adam_prepare_f32(P, P, P, P, 1, P, 1, nan, P, None) == EINVAL
    assert lib.ccvpe_adam_prepare_f32(P, P, P, P, 1, None, 0, 0.0, None, None) == EINVAL
    assert lib.ccvpe_adam_update_f32(P, P, P, P, 1, 1.0, None, None) == EINVAL          # no scalar block
    assert b"adam_update" in lib.ccvpe_last_error()
    assert lib.ccvpe_adam_update_f32(P, None, P, P, 1, 1.0, P, None) == EINVAL
    assert lib.ccvpe_adam_update_f32(P, P, P, P, 0, 1.0, P, None) == EINVAL
    assert lib.ccvpe_adam_update_f32(P, P, P, P, 1, nan, P, None) == EINVAL
