"""Graph-timed flash-attention kernels on the BERT-base shape (B 32, H 12, L 512, head 64):
forward, and the backward pair (dQ + dKV launched by ``attn_bwd``), with and without the
attention-probability dropout the training step uses.  One JSON line per case; the split
of the backward between its two kernels comes from a ``rocprofv3 --kernel-trace`` run of
this script.

    python tools/attn_micro.py [--B 32] [--L 512] [--H 12] [--causal]

``--causal`` times the causal kernels (GPT-2: ``--B 16 --L 1024 --causal``); the TFLOP/s
figures then count the computed tiles only, ``(nkb + 1) / (2 nkb)`` of the full square.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch

from kubeml_amd.ops import transformer as T
from conv_micro import gtime


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=32)
    ap.add_argument("--H", type=int, default=12)
    ap.add_argument("--L", type=int, default=512)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--causal", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda")
    B, H, L = a.B, a.H, a.L
    D = H * 64
    g = torch.Generator(device=dev).manual_seed(0)
    qkv = (torch.randn(B * L, 3 * D, device=dev, generator=g) * 0.5).to(torch.bfloat16)
    q, k, v = qkv[:, :D], qkv[:, D:2 * D], qkv[:, 2 * D:]
    dout = torch.randn(B * L, D, device=dev, generator=g).to(torch.bfloat16)
    dqkv = torch.empty_like(qkv)
    ctr = torch.tensor([3.0, 1.0], device=dev)
    fl_fwd = 4.0 * B * H * L * L * 64
    kw = {}
    if a.causal:
        nkb = (L + 63) // 64
        fl_fwd *= (nkb + 1) / (2.0 * nkb)
        kw["causal"] = True
    for name, drop in (("nodrop", None), ("drop0.1", (ctr, 77, 0.1))):
        out, lse = T.attn_fwd(q, k, v, B, H, L, drop=drop, **kw)
        tf = gtime(lambda: T.attn_fwd(q, k, v, B, H, L, out=out, drop=drop, **kw), reps=a.reps)
        tb = gtime(lambda: T.attn_bwd(q, k, v, out, dout, lse, B, H, L, dq=dqkv[:, :D], dk=dqkv[:, D:2 * D],
                                      dv=dqkv[:, 2 * D:], drop=drop, **kw), reps=a.reps)
        print(json.dumps({"case": name, "causal": a.causal, "B": B, "H": H, "L": L, "fwd_us": round(tf, 2),
                          "fwd_tflops": round(fl_fwd / tf / 1e6, 1), "bwd_us": round(tb, 2),
                          "bwd_tflops": round(2.5 * fl_fwd / tb / 1e6, 1)}), flush=True)


if __name__ == "__main__":
    main()
