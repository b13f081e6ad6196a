"""Isolated timing of the bank head's reduce stage, over the concat and split by channel half
(cosnet_amd/head_split.py), per modality.

For P pairs of HW = 60 x 60 pixels and C = 256 channels (the head of a 473 x 473 sequence; P = 10 is
one head call at pair_chunk 10, P = 60 the whole T = 12, N = 5 sequence), operands cold as in
tools/gemm_cold.py (enough distinct operand sets that every launch reads from HBM), bf16, the BN
folded in both:

    cat      gate_cat_idx (gate + copy of the a-role frame per pair) + conv_fwd_affine over [P HW][2C]
    split    gate_fwd + conv_fwd_affine_add over [P HW][C], adding the frame's partial through the map
    partial  conv_fwd_partial over the T = P / N frames of the bank (once per bank, not per head call)

each timed REPEATS times alternating in a captured graph; spread = (max - min) / mean of a
variant's repeats.  The table gives us per launch group, and split + partial against cat.

usage: python tools/head_split_probe.py [--pairs 10,60] [--nref 5] [--repeats 3]
"""
import argparse
import os
import sys

import torch
import torch.nn as nn

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from cosnet_amd import _native as nv  # noqa: E402
from cosnet_amd import ops  # noqa: E402

sys.path.insert(0, os.path.join(REPO, "tools"))
from gemm_cold import gtime_sets  # noqa: E402

dev = torch.device("cuda:0")
dt = torch.bfloat16
H = W = 60
HW = H * W
C = 256


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", default="10,60")
    ap.add_argument("--nref", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("head_split_probe: needs the GPU (no timing without one)")
    print("# reduce stage of the a-side head, one modality: HW = %d, C = %d, N = %d references, bf16, BN folded; us per "
          "launch group, mean of %d repeats (spread)" % (HW, C, a.nref, a.repeats))
    print("# P T | cat: gate_cat_idx + conv_fwd_affine us (spread) | split: gate_fwd + conv_fwd_affine_add us (spread) | "
          "partial: conv_fwd_partial over T frames us (spread) | split/cat | (split + partial)/cat | verdict")
    torch.manual_seed(0)
    bn = nn.BatchNorm2d(C).to(dev).eval()
    bn.running_mean.normal_(0, 0.3)
    bn.running_var.uniform_(0.5, 1.5)
    sc, sf = ops.bn_fold_table(bn)
    g = torch.randn((C,), device=dev) * 0.05
    for p in [int(v) for v in a.pairs.split(",")]:
        t = max(1, p // a.nref)
        per = (p * HW * C * 6 + t * HW * C * 6 + 9 * 2 * C * C) * 2      # z, cat, y; bank, partial; weight
        nsets = max(2, min(16, int(600e6 // per) + 1))
        cat, spl, par = [], [], []
        for _ in range(nsets):
            z = torch.randn((p * HW, C), device=dev).to(dt)
            v = torch.randn((t * HW, C), device=dev).to(dt)
            ia = torch.randint(0, t, (p,), device=dev, dtype=torch.int32)
            wf = (torch.randn((C, 9 * 2 * C), device=dev) * 0.02).to(dt)
            wz, wv = ops.weight_halves(wf, 3)
            cbuf = torch.empty((p * HW, 2 * C), device=dev, dtype=dt)
            gbuf = torch.empty((p * HW, C), device=dev, dtype=dt)
            y = torch.empty((p * HW, C), device=dev, dtype=dt)
            u = torch.empty((t * HW, C), device=dev, dtype=torch.float32)
            ops.conv_fwd_partial(v, t, H, W, wv, C, 3, 1, 1, 1, out=u)

            def fc(z=z, v=v, ia=ia, wf=wf, cbuf=cbuf, y=y):
                ops.gate_cat_idx(z, v, ia, p, HW, g, out=cbuf)
                ops.conv_fwd_affine(cbuf, p, H, W, wf, C, 3, 1, 1, 1, sc, sf, out=y)

            def fs(z=z, ia=ia, wz=wz, gbuf=gbuf, y=y, u=u):
                ops.gate_fwd(z, g, out=gbuf)
                ops.conv_fwd_affine_add(gbuf, p, H, W, wz, C, 3, 1, 1, 1, sc, sf, u, HW, add_map=ia, out=y)

            def fp(v=v, wv=wv, u=u):
                ops.conv_fwd_partial(v, t, H, W, wv, C, 3, 1, 1, 1, out=u)
            cat.append(fc)
            spl.append(fs)
            par.append(fp)
        tc, ts, tp = [], [], []
        with torch.no_grad():
            for _ in range(a.repeats):        # alternating, one device
                tc.append(gtime_sets(cat, reps=2) * 1e6)
                ts.append(gtime_sets(spl, reps=2) * 1e6)
                tp.append(gtime_sets(par, reps=2) * 1e6)
        mean = lambda v: sum(v) / len(v)
        spread = lambda v: (max(v) - min(v)) / mean(v)
        mc, ms, mp = mean(tc), mean(ts), mean(tp)
        gain = (mc - ms - mp) / mc
        noise = max(spread(tc), spread(ts), spread(tp))
        verdict = "split" if gain > noise else ("cat" if -gain > noise else "within the spread")
        print("%d %d | %.1f (%.3f) | %.1f (%.3f) | %.1f (%.3f) | %.3f | %.3f | %s" % (
            p, t, mc, spread(tc), ms, spread(ts), mp, spread(tp), ms / mc, (ms + mp) / mc, verdict), flush=True)
        del cat, spl, par
        torch.cuda.empty_cache()
    print("# FLOP ratio of the reduce convs alone, (1 + 1/N) / 2 = %.3f" % ((1 + 1 / a.nref) / 2))
    print("# lib %s" % nv.build_info())
    return 0


if __name__ == "__main__":
    sys.exit(main())
