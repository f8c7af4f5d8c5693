"""The optimizer of the training step: torch.optim.Adam's arithmetic and state format on one launch.

`Adam` is what `UFORecon.configure_optimizers` builds in the reference (code1/model.py:86: `optim.Adam(params, lr)`, every
other option at its default).  `step()` gathers the tensors that have a gradient and hands them to `ops.adam_step` --
ufr_adam_step on the GPU, the same formula as torch expressions on the CPU.  The state (`step`, `exp_avg`, `exp_avg_sq` per
parameter, created at a parameter's first gradient) and the param-group keys are torch.optim.Adam's, so a `state_dict()` of
either class loads into the other.

The step is ~62 small tensors, so its cost is the host's: what torch spends per tensor and step is not spent here.  Between
`state_dict()` calls a parameter's `step` is a python float (torch keeps a host tensor and adds 1 to it with a tensor op per
parameter and step; `state_dict()` writes torch's form, `load_state_dict()` reads it), and the table of addresses is built and
checked once per set of tensors with a gradient (`ops.AdamTable`): a step sets the gradients' addresses and the bias
corrections, and makes one call.
"""
from __future__ import annotations

import torch

from . import ops
from ._lib import UfrError


class Adam(torch.optim.Optimizer):
    def __init__(self, params, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8):
        if not (lr >= 0.0 and eps >= 0.0 and 0.0 <= betas[0] < 1.0 and 0.0 <= betas[1] < 1.0):
            raise UfrError(f"Adam: lr {lr}, betas {betas}, eps {eps} (lr, eps >= 0; 0 <= beta < 1)")
        # torch.optim.Adam's group keys with its defaults: the options beyond lr / betas / eps are carried for the format and
        # refused at any other value (step)
        super().__init__(params, dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=0, amsgrad=False, maximize=False,
                                      foreach=None, capturable=False, differentiable=False, fused=None,
                                      decoupled_weight_decay=False))
        self._tables = {}         # group index -> (ids of the parameters with a gradient, ops.AdamTable)

    def state_dict(self):
        sd = super().state_dict()
        # (the entries torch returns ARE the live ones: copy them, the live `step` stays a float)
        sd["state"] = {k: dict(st, step=torch.tensor(float(st["step"]), dtype=torch.float32)) for k, st in sd["state"].items()}
        return sd

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        for st in self.state.values():
            st["step"] = float(st["step"])       # a host or device tensor (torch's plain / fused forms) or a number
        self._tables.clear()

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        for gi, group in enumerate(self.param_groups):
            if group["weight_decay"] != 0 or group["amsgrad"] or group["maximize"] or group.get("decoupled_weight_decay", False):
                raise UfrError("Adam: weight_decay, amsgrad, maximize and decoupled_weight_decay are not implemented here "
                               "(the reference trains with torch.optim.Adam's defaults)")
            beta1, beta2 = group["betas"]
            live = [p for p in group["params"] if p.grad is not None]     # as torch: no gradient, no update, no step counted
            if not live:
                continue
            states, corrections, bc1, bc2 = [], {}, [], []
            for p in live:
                state = self.state[p]
                if len(state) == 0:
                    if p.grad.is_sparse or p.dtype != torch.float32 or not p.is_contiguous():
                        raise UfrError("Adam: dense float32 contiguous parameters only")
                    state["step"] = 0.0
                    state["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    state["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                t = state["step"] = state["step"] + 1.0
                if t not in corrections:
                    corrections[t] = (1.0 - beta1 ** t, 1.0 - beta2 ** t)
                bc1.append(corrections[t][0])
                bc2.append(corrections[t][1])
                states.append(state)
            grads = [p.grad for p in live]
            hyper = (float(group["lr"]), beta1, beta2, group["eps"])
            if not live[0].is_cuda:
                ops.adam_step(live, grads, [s["exp_avg"] for s in states], [s["exp_avg_sq"] for s in states], bc1, bc2, *hyper)
                continue
            ids = [id(p) for p in live]
            ent = self._tables.get(gi)
            if ent is None or ent[0] != ids or not ent[1].current() or any(
                    s["exp_avg"] is not m for s, m in zip(states, ent[1].tensors[len(live):2 * len(live)])):
                ent = self._tables[gi] = (ids, ops.AdamTable(live, [s["exp_avg"] for s in states], [s["exp_avg_sq"] for s in states]))
            ent[1].step(grads, bc1, bc2, *hyper)
        return loss
