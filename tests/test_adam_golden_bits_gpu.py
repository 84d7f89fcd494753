"""The single-group ``adam_`` / ``sgd_`` launches give the bits they have always given.

The kernels are built with ``-ffp-contract=fast``: which products the compiler fuses into FMAs is
its choice, and a refactor or a compiler change can move it (the float4 body of ``k_adam`` has one
rounding pattern for elements 0-2 and another for element 3; ``adam_vec4`` in
``csrc/kernels/optim.hip`` spells it out).  Results of training runs must not change with it, so
the digests of three steps on a fixed input are pinned in ``tests/golden/optim_bits.json`` (recorded
on an MI355X from the commit before the element update was factored out).  The input is built from
integer hashes, exactly representable, so it does not depend on any random generator."""
import hashlib
import json
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "optim_bits.json")
N = 4 * 1027 + 3            # float4 body over more than one block, and a 3-element scalar tail


def _hashed(n, salt, scale):
    i = torch.arange(n, dtype=torch.int64)
    h = ((i + salt) * 2654435761) % (1 << 32)
    h = (h ^ (h >> 15)) * 40503 % (1 << 32)
    return (((h >> 8).double() / float(1 << 24) - 0.5) * scale).float()     # 24-bit values: exact in fp32


def _digest(t):
    return hashlib.sha1(t.contiguous().view(torch.uint8).cpu().numpy().tobytes()).hexdigest()


def compute_digests(dev="cuda"):
    from kubeml_amd.ops import kernels as K
    w0 = _hashed(N, 1, 2.0).to(dev)
    grads = [_hashed(N, 100 + k, s).to(dev) for k, s in enumerate((1.0, 2.0 ** -10, 2.0 ** -23))]
    clip = torch.tensor([0.375], device=dev)
    out = {}
    for dec in (False, True):
        for cd in (None, clip):
            w, m, v = w0.clone(), torch.zeros_like(w0), torch.zeros_like(w0)
            sh = torch.zeros(N, dtype=torch.bfloat16, device=dev)
            for it, g in enumerate(grads):
                K.adam_(w, g, m, v, sh, 1e-3, it + 1, wd=0.01, decoupled=dec, grad_scale=0.5, clip_dev=cd)
            out[f"adam decoupled={dec} clip={cd is not None}"] = [_digest(t) for t in (w, m, v, sh)]
    for nest in (False, True):
        w, m = w0.clone(), torch.zeros_like(w0)
        sh = torch.zeros(N, dtype=torch.bfloat16, device=dev)
        for it, g in enumerate(grads):
            K.sgd_(w, g, m, sh, 0.1, wd=1e-4, momentum=0.9, dampening=0.0 if nest else 0.1, nesterov=nest,
                   first=it == 0, grad_scale=0.5, clip_dev=clip)
        out[f"sgd nesterov={nest}"] = [_digest(t) for t in (w, m, sh)]
    torch.cuda.synchronize()
    return out


def test_single_group_optimizer_bits_are_the_recorded_ones():
    with open(GOLDEN) as f:
        want = json.load(f)
    got = compute_digests()
    assert sorted(got) == sorted(want)
    for key in sorted(want):
        assert got[key] == want[key], key
