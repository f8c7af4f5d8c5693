"""What the training front door's tests share: the Adam yardstick (torch.optim.Adam in float64 on the same float32 gradients),
its bound, and the inputs of the ray draw."""
from __future__ import annotations

import numpy as np
import torch

STEPS = 5


def adam_case(numels, seed=0, skip=(1, 2), never=True):
    """Seeded N(0,1) parameters of the given sizes (+ one of 5 elements that never gets a gradient) and STEPS gradients each;
    tensor ``skip[0]`` has no gradient at step index ``skip[1]``.  -> (params, grads[step][tensor] with None entries)."""
    g = torch.Generator().manual_seed(1000 + seed)
    params = [torch.randn(n, generator=g) for n in numels] + ([torch.randn(5, generator=g)] if never else [])
    grads = []
    for s in range(STEPS):
        row = [torch.randn(n, generator=g) * (0.1 + 0.3 * s) for n in numels] + ([None] if never else [])
        if skip is not None and s == skip[1]:
            row[skip[0]] = None
        grads.append(row)
    return params, grads


def run_adam(make_first, params, grads, dtype=torch.float32, device="cpu", make_second=None, switch_at=None, place=None,
             place_grad=None):
    """STEPS optimizer steps on clones of ``params`` in ``dtype``; at step index ``switch_at`` the optimizer is replaced by
    ``make_second(params)`` loaded with the first one's state_dict.  ``place(i, tensor)`` / ``place_grad(i, tensor)`` (optional)
    put parameter / gradient ``i`` where the caller wants it (views, offsets).  -> (final parameters as float64 CPU tensors,
    the last optimizer)."""
    place = place or (lambda i, t: t)
    place_grad = place_grad or (lambda i, t: t)
    ps = [place(i, p.to(device=device, dtype=dtype).clone()).requires_grad_(True) for i, p in enumerate(params)]
    opt = make_first(ps)
    for s in range(STEPS):
        if switch_at is not None and s == switch_at:
            sd = opt.state_dict()
            opt = make_second(ps)
            opt.load_state_dict(sd)
        for i, (p, gr) in enumerate(zip(ps, grads[s])):
            p.grad = None if gr is None else place_grad(i, gr.to(device=device, dtype=dtype).clone())
        opt.step()
    return [p.detach().double().cpu() for p in ps], opt


def adam_bounds(params, grads, lr):
    """Per tensor: (yardstick result, max(4 x the error of torch.optim.Adam in float32 against it, one float32 ulp of max|p|))."""
    want, _ = run_adam(lambda ps: torch.optim.Adam(ps, lr=lr), params, grads, dtype=torch.float64)
    t32, _ = run_adam(lambda ps: torch.optim.Adam(ps, lr=lr), params, grads, dtype=torch.float32)
    bounds = []
    for w, t in zip(want, t32):
        ulp = float(np.spacing(np.float32(w.abs().max())))
        bounds.append(max(4.0 * float((w - t).abs().max()), ulp))
    return want, bounds


def quantised_uniforms(n, seed=0):
    """rand quantised to 2^-10: many ties, some of them at any k-th position"""
    return torch.floor(torch.rand(n, generator=torch.Generator().manual_seed(seed)) * 1024.0) / 1024.0


def stable_first_k(u, k):
    return torch.sort(u.cpu(), stable=True).indices[:k]
