"""Drop-in gradient utilities for models whose parameters live in a flat space.

``clip_grad_norm_`` replaces ``torch.nn.utils.clip_grad_norm_`` in eager (not graph-captured)
GPU training loops.  torch's function reads ``p.grad`` parameter by parameter: on a flattened
model that is ~200 small launches, and it is wrong when called before the flat space has made
its gradients final (deferred 3x3 folds, regions nobody wrote).  Here the space is finished
first, the norm is ONE deterministic launch over the flat gradient buffer and the scale one
in-place pass, with the coefficient never leaving the device.

Inside ``KubeModel.step`` / a captured step use the optimizers' ``max_grad_norm`` instead: the
coefficient is then consumed by the fused update and the gradient is not rewritten at all.
"""
from __future__ import annotations

import torch

__all__ = ["clip_grad_norm_"]


def _one_gpu_space(params):
    """The flat space holding exactly ``params`` (all of its parameters) on a GPU, else None."""
    sp = getattr(params[0], "_kml_flat", None) if params else None
    if sp is None or sp.device.type != "cuda" or sp.grad is None:
        return None
    if any(getattr(p, "_kml_flat", None) is not sp for p in params):
        return None
    if {id(p) for p in params} != {id(p) for p in sp.params}:
        return None          # a subset: its norm is not the buffer's norm
    return sp


def clip_grad_norm_(parameters, max_norm, norm_type=2.0, error_if_nonfinite=False, foreach=None):
    """``torch.nn.utils.clip_grad_norm_`` for flat-space models.

    When ``parameters`` are all the parameters of one GPU flat space (and the norm is L2): the
    space's gradients are made final, one launch computes the global norm, one scales the flat
    gradient by ``min(1, max_norm / (norm + 1e-6))`` in place; returns the norm as a 0-d device
    tensor (no synchronisation).  Anything else defers to torch's function."""
    if isinstance(parameters, torch.Tensor):
        parameters = [parameters]
    params = list(parameters)
    sp = _one_gpu_space(params) if float(norm_type) == 2.0 and not error_if_nonfinite else None
    if sp is None:
        return torch.nn.utils.clip_grad_norm_(params, max_norm, norm_type=norm_type,
                                              error_if_nonfinite=error_if_nonfinite, foreach=foreach)
    from ..ops import kernels as K
    sp.finish_grads()
    out = torch.empty(3, dtype=torch.float32, device=sp.device)
    thr = torch.full((1,), float(max_norm), dtype=torch.float32, device=sp.device)
    K.grad_norm_(sp.grad, out, thr)
    K.scale_by_coef_(sp.grad, out)
    return out[1]
