"""Graph-timed split of a conv backward on ResNet-34's 3x3 / stride-1 layers (batch 256):
the grouped dgrad+wgrad launch the step uses (``conv_bwd``), and dgrad / wgrad alone with
the same plans.

    python tools/bwd_micro.py [--batch 256]
    python tools/bwd_micro.py --oneshot     # layer3 / layer4: the one-shot pair against the implicit-GEMM pair
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from kubeml_amd.ops import kernels as K
from conv_micro import gtime


def oneshot_pairs(B, dev):
    """Layer3 (unrolled 2x2 maps) and layer4 (centre tap on 1x1 maps): the grouped one-shot pair
    the step runs, layer3's dgrad panels in one 128 KB pass or two 64 KB halves, and the implicit-GEMM
    pair (+ the share of the fold launch for layer3) it replaces."""
    for (H, C) in [(2, 256), (1, 512)]:
        x = torch.randn(B, H, H, C, device=dev).to(torch.bfloat16)
        w = (torch.randn(C, 3, 3, C, device=dev) * 0.05).to(torch.bfloat16)
        dy = torch.randn(B, H, H, C, device=dev).to(torch.bfloat16)
        dw = torch.zeros(C, 3, 3, C, device=dev)
        args = (3, 3, (1, 1), (1, 1))
        u = H == 2
        wu = K.GATHER22 if u else None
        r = {"H": H, "C": C, "B": B}
        default = K._ONESHOT_PAIR_U22
        for name, plans in (("pair_us", K._ONESHOT_PAIR_U22_FULL), ("pair_halves_us", K._ONESHOT_PAIR_U22_HALF)):
            if not u and name != "pair_us":
                continue
            K._ONESHOT_PAIR_U22 = plans
            r[name.replace("_us", "_plans")] = K.bwd_plans(x.shape, C, *args, unroll=u)
            r[name] = round(gtime(lambda: K.conv_bwd(dy, w, x, dw, *args, wu=wu, accumulate=False)), 2)
        K._ONESHOT_PAIR_U22 = default
        K._ONESHOT_PAIR_ON = False
        r["old_plans"] = K.bwd_plans(x.shape, C, *args, unroll=u)
        if u:
            g = torch.empty(4 * C, 1, 1, 4 * C, device=dev)
            r["old_pair_us"] = round(gtime(lambda: K.conv_bwd(dy, w, x, g, *args, wu=wu)), 2)
            r["fold_us"] = round(gtime(lambda: K.fold22_multi([(g, dw, False)])), 2)
            r["fold11_us"] = round(gtime(lambda: K.fold22_multi([(g, dw, False)] * 11)), 2)
        else:
            r["old_pair_us"] = round(gtime(lambda: K.conv_bwd(dy, w, x, dw, *args, accumulate=False)), 2)
        K._ONESHOT_PAIR_ON = True
        print(json.dumps(r), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--oneshot", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda")
    B = a.batch
    if a.oneshot:
        return oneshot_pairs(B, dev)
    for (H, C, Co) in [(8, 64, 64), (4, 128, 128)]:
        x = torch.randn(B, H, H, C, device=dev).to(torch.bfloat16)
        w = (torch.randn(Co, 3, 3, C, device=dev) * 0.05).to(torch.bfloat16)
        dy = torch.randn(B, H, H, Co, device=dev).to(torch.bfloat16)
        dw = torch.zeros(Co, 3, 3, C, device=dev)
        dplan, wplan, grouped = K.bwd_plans(x.shape, Co, 3, 3, (1, 1), (1, 1))
        r = {"dplan": dplan, "wplan": wplan, "grouped": grouped}
        M = B * H * H
        base = K.plan_conv("dgrad", M, C, 9 * Co)
        r["base_dplan"] = base
        r["bwd_us"] = round(gtime(lambda: K.conv_bwd(dy, w, x, dw, 3, 3, (1, 1), (1, 1), accumulate=False)), 2)
        r["pair_base_us"] = round(gtime(lambda: K.conv_bwd(dy, w, x, dw, 3, 3, (1, 1), (1, 1), accumulate=False,
                                                           dcfg=base, wcfg=wplan)), 2)
        r["dgrad_us"] = round(gtime(lambda: K.conv_dgrad(dy, w, x.shape, 3, 3, (1, 1), (1, 1), cfg=dplan)), 2)
        r["dgrad_base_us"] = round(gtime(lambda: K.conv_dgrad(dy, w, x.shape, 3, 3, (1, 1), (1, 1), cfg=base)), 2)
        r["wgrad_us"] = round(gtime(lambda: K.conv_wgrad(x, dy, dw, 3, 3, (1, 1), (1, 1), cfg=wplan,
                                                         accumulate=False)), 2)
        r["gflop_each"] = round(2 * M * Co * 9 * C / 1e9, 3)
        print(json.dumps({"H": H, "C": C, "K": Co, **r}), flush=True)


if __name__ == "__main__":
    main()
