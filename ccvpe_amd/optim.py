"""Adam / AdamW for the training step on the MI355X: torch.optim.Adam's arithmetic (train_VIGOR.py:104 / train_KITTI.py:
`torch.optim.Adam(params, lr, betas=(0.9, 0.999))`, eps 1e-8) for all ~520 parameter tensors at once, over a device table of
(param, grad, exp_avg, exp_avg_sq, numel) rows, a per-tensor hyper-parameter row and a workgroup -> (tensor, chunk) map.

Both classes ARE torch.optim.Optimizers: param groups (per-group lr / betas / eps / weight_decay), `state[p] = {step, exp_avg,
exp_avg_sq}` in torch.optim.Adam's format, the base class's validated state_dict() / load_state_dict() (checkpoints interchange
with torch.optim.Adam / AdamW), add_param_group(), and torch LR schedulers all work.  Like torch, every parameter keeps its own
step count (a parameter that starts receiving gradients later gets its own bias correction).

Two paths:

* host path (the default; what the reference's configuration takes): the step counts are host numbers, the bias corrections are
  formed on the host per step and uploaded, ONE launch of ccvpe_adam_step_f32.  With `weight_decay` the same walk fills the
  wider rows of ccvpe_adam_update_f32 (L2 decay for Adam as torch.optim.Adam, decoupled decay for AdamW as torch.optim.AdamW).
* device path (`capturable=True`, and implied by `max_grad_norm` / `skip_nonfinite`): csrc/optim.hip.  The step counts are ONE
  flat fp32 device array (`state[p]["step"]` are views of it, as torch's capturable optimizers keep device steps), the table, the
  chunk maps, the constant rows (lr, betas, eps, weight_decay per tensor, in double) and the norm partials are static device
  buffers, and a step is two launches (prepare: step counts += 1 and the derived rows; update) or three with the global-norm
  pass in front.  Nothing is computed, uploaded or read back on the host per step, so step() can be captured into a hipGraph
  (graph.GraphedTrainStep(loss_fn, net, optimizer)).  The buffers are rebuilt, outside any capture, only when the parameter set
  or a gradient's address changes; the constant rows are refreshed (sync_hyper(), from pinned memory) only when a group's lr /
  betas / eps / weight_decay changed - which is how LR schedulers keep working with a captured step.  `grad_scale` and
  `max_grad_norm` travel as kernel arguments: a captured step keeps the values it was captured with.

Global-norm clipping (`max_grad_norm`) is torch.nn.utils.clip_grad_norm_ folded into the step: `last_grad_norm` (a device scalar
at a fixed address) is the L2 norm of all gradients after grad_scale and before clipping, and the update multiplies every gradient
by min(1, max_grad_norm / (norm + 1e-6)).  DELIBERATE DEPARTURE from torch: when the norm is inf / NaN and `max_grad_norm` or
`skip_nonfinite` is set, the WHOLE step is skipped - parameters, moments and step counts stay bit-untouched and the device counter
`skipped_steps` goes up by one - where clip_grad_norm_ + step() would write NaN into every weight.

Not supported (raises): amsgrad, maximize, sparse gradients; step_subset() with the device path."""
import math

import numpy as np
import torch

from . import _lib, ops
from ._lib import check


class Adam(torch.optim.Optimizer):
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False, capturable=False,
                 max_grad_norm=None, skip_nonfinite=False, decoupled_weight_decay=False):
        if amsgrad:
            raise ValueError("ccvpe_amd.optim.Adam: amsgrad is not implemented")
        if lr < 0 or eps < 0 or weight_decay < 0 or not (0 <= betas[0] < 1 and 0 <= betas[1] < 1):
            raise ValueError("invalid Adam hyper-parameters")
        if max_grad_norm is not None and not (float(max_grad_norm) > 0 and math.isfinite(float(max_grad_norm))):
            raise ValueError("max_grad_norm must be a positive finite number (or None)")
        # the global-norm options need the device-side step counts (a skipped step must not advance them, and the decision is
        # never read back), so they imply the capturable state layout
        self.capturable = bool(capturable or max_grad_norm is not None or skip_nonfinite)
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        self.skip_nonfinite = bool(skip_nonfinite)
        super().__init__(params, dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay, amsgrad=False,
                                      capturable=self.capturable, decoupled_weight_decay=bool(decoupled_weight_decay)))
        self._layout = None
        self._subset_layouts = {}    # tuple of parameter ids -> launch geometry of step_subset()
        self._pre_stepped = set()    # ids updated by step_subset() since the last step(): step() skips them once
        self.grad_scale = 1.0        # caller-set multiplier applied to every gradient inside the update kernel (e.g. loss scaling)
        self._dev = None             # device path: table + key of the (parameter, gradient) addresses it was built for
        self._steps = None           # device path: flat fp32 step counts, one per parameter
        self._steps_ids = None
        self._state_stale = False    # load_state_dict() replaced the state tensors: re-bind the step views, rebuild the table
        self._scalars = None         # device: (total_norm, clip_coef, finite, skipped_steps)

    # ---- static launch geometry: rebuilt only when the parameter set changes --------------------------------
    def _build_layout(self, params=None):
        lib = _lib.load()
        whole = params is None
        if whole:
            params = [p for g in self.param_groups for p in g["params"]]
        for p in params:
            if not (p.is_cuda and p.dtype == torch.float32 and p.is_contiguous()):
                raise ValueError("ccvpe_amd.optim.Adam needs contiguous fp32 parameters on the MI355X (no CPU fallback)")
        chunk = lib.ccvpe_adam_chunk_elems()
        ct, co = [], []
        for t, p in enumerate(params):
            n = (p.numel() + chunk - 1) // chunk
            ct.append(np.full((n,), t, dtype=np.int32))
            co.append(np.arange(n, dtype=np.int32))
        dev = params[0].device
        lay = dict(params=params, ids=tuple(id(p) for p in params),
                   chunk_tensor=torch.from_numpy(np.concatenate(ct)).to(dev),
                   chunk_off=torch.from_numpy(np.concatenate(co)).to(dev),
                   table=np.zeros((len(params), 5), dtype=np.int64),
                   hyper=np.zeros((len(params), lib.ccvpe_adam_hyper_floats()), dtype=np.float32),
                   hyper_wd=np.zeros((len(params), lib.ccvpe_adam_device_layout(0)), dtype=np.float32))
        if whole:
            self._layout = lay
        return lay

    def _state_of(self, p):
        st = self.state[p]
        if len(st) == 0:                                     # lazy, as torch.optim.Adam._init_group
            st["step"] = torch.tensor(0.0, dtype=torch.float32)
            st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
        return st

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        if self.capturable:
            self._step_device()
            return loss
        lay = self._layout
        if lay is None or lay["ids"] != tuple(id(p) for g in self.param_groups for p in g["params"]):
            lay = self._build_layout()
        skip, self._pre_stepped = self._pre_stepped, set()
        self._launch(lay, skip)
        return loss

    @torch.no_grad()
    def step_subset(self, params):
        """Update ONLY `params` now (their .grad must be final) and remember them: the next step() skips them once.
        harness.GradientAllReducer(step_in_backward=True) calls this per gradient group as soon as the group's all-reduce has
        finished, so the optimizer of the early groups runs beside the collectives of the late ones and the last (small)
        all-reduce is not exposed in front of a whole-model update.  Same arithmetic, same per-parameter step counts as step().
        Host path only: the global norm needs every gradient, and the device path's tables cover the whole parameter set."""
        if self.capturable:
            raise ValueError("ccvpe_amd.optim: step_subset() is not available with capturable / max_grad_norm / skip_nonfinite")
        params = [p for p in params if p.grad is not None and id(p) not in self._pre_stepped]
        if not params:
            return
        key = tuple(id(p) for p in params)
        lay = self._subset_layouts.get(key)
        if lay is None:
            lay = self._subset_layouts[key] = self._build_layout(params)
        self._launch(lay, set())
        self._pre_stepped.update(key)

    def _group_of(self):
        return {id(p): g for g in self.param_groups for p in g["params"]}

    @staticmethod
    def _hyper_row(lr, b1, b2, eps, k):
        """The derived numbers of one tensor at its 1-based step count k: bias corrections and 1 - beta in double on the host,
        as torch.optim.Adam does with Python floats (csrc/optim.hip: adam_prepare_kernel forms the same on the device)."""
        return (lr / (1.0 - b1 ** k), b1, b2, 1.0 - b1, 1.0 - b2, eps, math.sqrt(1.0 - b2 ** k))

    @staticmethod
    def _decay_of(g):
        """(l2, decay factor) of a param group: torch.optim.Adam adds weight_decay * p to the gradient, torch.optim.AdamW
        multiplies the parameter by 1 - lr * weight_decay."""
        wd = float(g.get("weight_decay", 0))
        if g.get("decoupled_weight_decay", False):
            return 0.0, 1.0 - float(g["lr"]) * wd
        return wd, 1.0

    def _launch(self, lay, skip):
        lib = _lib.load()
        decay = any(g.get("weight_decay", 0) for g in self.param_groups)      # no group decays: the original launch, untouched
        table, hyper = lay["table"], lay["hyper_wd"] if decay else lay["hyper"]
        group_of = self._group_of()
        keep, any_grad = [], False
        for t, p in enumerate(lay["params"]):
            g = group_of[id(p)]
            lr, (b1, b2), eps = float(g["lr"]), g["betas"], float(g["eps"])
            if g.get("amsgrad", False) or g.get("maximize", False):
                raise ValueError("ccvpe_amd.optim.Adam: amsgrad / maximize are not implemented")
            gr = p.grad
            if gr is None or id(p) in skip:
                table[t, 1] = 0
                continue
            if gr.is_sparse:
                raise RuntimeError("ccvpe_amd.optim.Adam does not support sparse gradients")
            if not gr.is_contiguous() or gr.dtype != torch.float32:
                gr = gr.contiguous().float()
                keep.append(gr)
            st = self._state_of(p)
            st["step"] += 1
            k = float(st["step"])
            hyper[t] = self._hyper_row(lr, b1, b2, eps, k) + ((self._decay_of(g) + (0.0,)) if decay else (0.0,))
            table[t] = (p.data_ptr(), gr.data_ptr(), st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr(), p.numel())
            any_grad = True
        if not any_grad:
            return
        dev = lay["params"][0].device
        tab_d = torch.from_numpy(table).to(dev, non_blocking=False)
        hyp_d = torch.from_numpy(hyper).to(dev, non_blocking=False)
        if decay:
            check(lib.ccvpe_adam_update_f32(ops._ptr(tab_d), ops._ptr(hyp_d), ops._ptr(lay["chunk_tensor"]), ops._ptr(lay["chunk_off"]),
                                            lay["chunk_tensor"].numel(), float(self.grad_scale), ops._ptr(self._unit_scalars(dev)),
                                            ops._stream()), "ccvpe_adam_update_f32")
        else:
            check(lib.ccvpe_adam_step_f32(ops._ptr(tab_d), ops._ptr(hyp_d), ops._ptr(lay["chunk_tensor"]), ops._ptr(lay["chunk_off"]),
                                          lay["chunk_tensor"].numel(), float(self.grad_scale), ops._stream()), "ccvpe_adam_step_f32")
        _lib.weights_epoch += 1          # parameters changed without a torch version bump: invalidate packed weights
        cur = torch.cuda.current_stream()
        for k in keep + [tab_d, hyp_d]:
            k.record_stream(cur)

    def _unit_scalars(self, dev):
        """(total_norm 0, clip_coef 1, finite 1, skipped 0): what the update kernel reads when no prepare launch precedes it."""
        if getattr(self, "_unit", None) is None or self._unit.device != dev:
            self._unit = torch.tensor([0.0, 1.0, 1.0, 0.0], dtype=torch.float32, device=dev)
        return self._unit

    # ---- device path -------------------------------------------------------------------------------------------------------
    @property
    def last_grad_norm(self):
        """Device scalar (fixed address): L2 norm of all gradients of the last step(), after grad_scale, before clipping.
        None before the first step; 0 unless max_grad_norm or skip_nonfinite is set."""
        return None if self._scalars is None else self._scalars[0]

    @property
    def skipped_steps(self):
        """Device counter (fp32, fixed address) of the steps skipped for a non-finite gradient norm; None before the first step."""
        return None if self._scalars is None else self._scalars[3]

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        self._state_stale = True
        for g in self.param_groups:              # which path runs is this object's choice, not the checkpoint's
            g["capturable"] = self.capturable
        if not self.capturable:                  # a capturable checkpoint: the host path counts on the host
            for st in self.state.values():
                if torch.is_tensor(st.get("step")) and st["step"].is_cuda:
                    st["step"] = st["step"].cpu()

    def _hyper_sig(self):
        sig = []
        for g in self.param_groups:
            if g.get("amsgrad", False) or g.get("maximize", False):
                raise ValueError("ccvpe_amd.optim.Adam: amsgrad / maximize are not implemented")
            sig.append((float(g["lr"]), float(g["betas"][0]), float(g["betas"][1]), float(g["eps"]),
                        float(g.get("weight_decay", 0)), 1.0 if g.get("decoupled_weight_decay", False) else 0.0, len(g["params"])))
        return tuple(sig)

    def _bind_steps(self, params):
        """One flat fp32 device array of step counts; state[p]["step"] become views of it (values carried over)."""
        dev = params[0].device
        flat = torch.zeros(len(params), dtype=torch.float32, device=dev)
        have = [t for t, p in enumerate(params) if len(self.state.get(p, ())) > 0]
        if have:
            vals = [torch.as_tensor(self.state[params[t]]["step"], dtype=torch.float32).reshape(()).to(dev) for t in have]
            flat[torch.tensor(have, device=dev)] = torch.stack(vals)
            for t in have:
                self.state[params[t]]["step"] = flat[t]
        self._steps, self._steps_ids = flat, tuple(id(p) for p in params)

    def _device_tables(self):
        """The static device buffers for the current (parameter, gradient) addresses; rebuilt only when those change, and
        never inside a stream capture (a rebuild uploads)."""
        params = [p for g in self.param_groups for p in g["params"]]
        grads, keep = [], []
        for p in params:
            gr = p.grad
            if gr is not None:
                if gr.is_sparse:
                    raise RuntimeError("ccvpe_amd.optim.Adam does not support sparse gradients")
                if not gr.is_contiguous() or gr.dtype != torch.float32:
                    gr = gr.contiguous().float()         # a new address every step: works, but rebuilds the table every step
                    keep.append(gr)
            grads.append(gr)
        key = tuple((id(p), p.data_ptr(), 0 if gr is None else gr.data_ptr()) for p, gr in zip(params, grads))
        dv = self._dev
        if dv is not None and dv["key"] == key and not self._state_stale:
            dv["keep"] = keep
            return dv
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("ccvpe_amd.optim: the parameter set or a gradient's address changed; the device tables cannot be "
                               "rebuilt inside a stream capture (run one step(), or sync_hyper(), outside the capture first)")
        lib = _lib.load()
        lay = self._layout
        ids = tuple(id(p) for p in params)
        if lay is None or lay["ids"] != ids:
            lay = self._build_layout()
        dev = params[0].device
        if self._steps is None or self._steps_ids != ids or self._state_stale:
            self._bind_steps(params)
        if self._scalars is None:
            self._scalars = torch.zeros(lib.ccvpe_adam_device_layout(2), dtype=torch.float32, device=dev)
            self._scalars[1:3] = 1.0
        if "dev" not in lay:
            n = len(params)
            lay["dev"] = dict(consts=torch.zeros((n, lib.ccvpe_adam_device_layout(1)), dtype=torch.float64, device=dev),
                              consts_host=torch.zeros((n, lib.ccvpe_adam_device_layout(1)), dtype=torch.float64).pin_memory(),
                              hyper=torch.zeros((n, lib.ccvpe_adam_device_layout(0)), dtype=torch.float32, device=dev),
                              partials=torch.zeros(lay["chunk_tensor"].numel(), dtype=torch.float32, device=dev),
                              sig=None, event=None)
        table = np.zeros((len(params), 5), dtype=np.int64)
        for t, (p, gr) in enumerate(zip(params, grads)):
            if gr is None:                               # no state yet (lazy, as torch): a null row, skipped by every kernel
                table[t] = (p.data_ptr(), 0, 0, 0, p.numel())
                continue
            st = self.state[p]
            if len(st) == 0:
                st["step"] = self._steps[t]
                st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            for k in ("exp_avg", "exp_avg_sq"):
                if not (st[k].is_cuda and st[k].dtype == torch.float32 and st[k].is_contiguous()):
                    st[k] = st[k].to(device=dev, dtype=torch.float32).contiguous()
            table[t] = (p.data_ptr(), gr.data_ptr(), st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr(), p.numel())
        self._dev = dict(key=key, table=torch.from_numpy(table).to(dev), keep=keep, lay=lay)
        self._state_stale = False
        return self._dev

    def bind(self):
        """Build the device tables for the gradients the parameters hold NOW and refresh the hyper rows: call it, outside
        the capture, before capturing step() (graph.GraphedTrainStep does, once the backward's static gradients exist)."""
        if not self.capturable:
            raise ValueError("ccvpe_amd.optim: bind() belongs to the device path (capturable=True)")
        self._device_tables()
        self.sync_hyper()

    def sync_hyper(self):
        """Refresh the device constant rows (lr, betas, eps, weight_decay per tensor) if a param group changed since the last
        call - an LR scheduler, or the user.  One asynchronous copy from pinned memory when something changed, nothing
        otherwise.  step() calls it when not capturing; a captured step is replayed, so whoever replays it calls this first
        (graph.GraphedTrainStep does).  No-op on the host path."""
        if not self.capturable:
            return
        dv = self._dev if self._dev is not None else self._device_tables()
        d = dv["lay"]["dev"]
        sig = self._hyper_sig()
        if sig == d["sig"]:
            return
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("ccvpe_amd.optim: hyper-parameters changed; call sync_hyper() outside the stream capture")
        if d["event"] is not None:
            d["event"].synchronize()                     # the previous refresh has left the pinned rows
        rows, t = d["consts_host"].numpy(), 0
        for row in sig:
            rows[t:t + row[-1]] = row[:-1]
            t += row[-1]
        d["consts"].copy_(d["consts_host"], non_blocking=True)
        d["event"] = torch.cuda.Event()
        d["event"].record()
        d["sig"] = sig

    def _step_device(self):
        lib = _lib.load()
        dv = self._device_tables()
        self.sync_hyper()
        lay = dv["lay"]
        d = lay["dev"]
        n_chunks = lay["chunk_tensor"].numel()
        gs, stream = float(self.grad_scale), ops._stream()
        norm = self.max_grad_norm is not None or self.skip_nonfinite
        if norm:
            check(lib.ccvpe_grad_sqnorm_f32(ops._ptr(dv["table"]), ops._ptr(lay["chunk_tensor"]), ops._ptr(lay["chunk_off"]), n_chunks,
                                            gs, ops._ptr(d["partials"]), stream), "ccvpe_grad_sqnorm_f32")
        check(lib.ccvpe_adam_prepare_f32(ops._ptr(dv["table"]), ops._ptr(d["consts"]), ops._ptr(self._steps), ops._ptr(d["hyper"]),
                                         len(lay["params"]), ops._ptr(d["partials"]) if norm else None, n_chunks if norm else 0,
                                         self.max_grad_norm or 0.0, ops._ptr(self._scalars), stream), "ccvpe_adam_prepare_f32")
        check(lib.ccvpe_adam_update_f32(ops._ptr(dv["table"]), ops._ptr(d["hyper"]), ops._ptr(lay["chunk_tensor"]),
                                        ops._ptr(lay["chunk_off"]), n_chunks, gs, ops._ptr(self._scalars), stream),
              "ccvpe_adam_update_f32")
        _lib.weights_epoch += 1          # parameters changed without a torch version bump: invalidate packed weights


class AdamW(Adam):
    """torch.optim.AdamW: Adam with DECOUPLED weight decay (p *= 1 - lr * weight_decay before the update), torch's default 1e-2.
    Weight decay is per param group: put BatchNorm and bias tensors into a group with weight_decay=0 to exclude them."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, amsgrad=False, capturable=False,
                 max_grad_norm=None, skip_nonfinite=False):
        super().__init__(params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=amsgrad, capturable=capturable,
                         max_grad_norm=max_grad_norm, skip_nonfinite=skip_nonfinite, decoupled_weight_decay=True)
