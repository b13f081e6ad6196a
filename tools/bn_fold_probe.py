"""Per-class timing of the eval-mode BN fold (cosnet_amd/bn_fold.py) against today's three launches.

For every distinct conv + BN class of both encoders at the bank's shape (473 x 473 frames,
encode_chunk 8; the classes are recorded from one folded walk), operands cold as in
tools/gemm_cold.py (enough distinct operand sets that every launch reads from HBM), bf16:

    unfolded   conv_fwd + bn_stats (eval: cn_bn_eval_params) + bn_apply, as encoder.features_nhwc
    folded     conv_fwd_affine on the generic GEMM epilogue (cn_gemm_ws_mode 0), or the split-K reduce
    folded ws  conv_fwd_affine as dispatched by default, where that is the weight-stationary kernel

each timed REPEATS times alternating; spread = (max - min) / mean of a variant's repeats.  A class
is 'folded' only where the folded mean is below the unfolded mean by more than the larger spread;
cosnet_amd/bn_fold.py fold_route encodes the result ('ws' after the unfolded time: today's conv
runs on the weight-stationary kernel).

usage: python tools/bn_fold_probe.py [--size 473] [--frames 8] [--repeats 3]
"""
import argparse
import os
import sys

import torch
import torch.nn as nn

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import cosnet_amd as C  # noqa: E402
from cosnet_amd import _native as nv  # noqa: E402
from cosnet_amd import bn_fold, ops  # noqa: E402
from cosnet_amd.init_recipe import recipe_state_dict  # noqa: E402

sys.path.insert(0, os.path.join(REPO, "tools"))
from gemm_cold import gtime_sets  # noqa: E402

dev = torch.device("cuda:0")
dt = torch.bfloat16


def classes(size, frames):
    """{(n, h, w, cin, cout, k, stride, pad, dil, act, has_res, has_bias, ldy): count} over both encoders."""
    m = C.build_model(dt)
    m.load_state_dict(recipe_state_dict(m.state_dict()))
    m = m.to(dev).eval()
    m.set_bn_fold()
    seen = {}
    real = bn_fold.conv_bn_folded

    def rec(T, x, n, h, w, wf, cout, k, stride, pad, dil, bn, act=0, prelu=None, res=None, bias=None, out=None):
        key = (n, h, w, wf.shape[1] // (k * k), cout, k, stride, pad, dil, act, res is not None,
               bias is not None, cout if out is None else out.stride(0))
        seen[key] = seen.get(key, 0) + 1
        return real(T, x, n, h, w, wf, cout, k, stride, pad, dil, bn, act=act, prelu=prelu, res=res, bias=bias, out=out)

    bn_fold.conv_bn_folded = rec
    try:
        with torch.no_grad():
            m._set_dtype()
            g = torch.Generator().manual_seed(0)
            bn_fold.encode_frames_folded(m.encoder, torch.rand((frames, 3, size, size), generator=g).to(dev))
            bn_fold.encode_frames_folded(m.depth_encoder, torch.rand((frames, 1, size, size), generator=g).to(dev))
        torch.cuda.synchronize()
    finally:
        bn_fold.conv_bn_folded = real
    return seen


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=473)
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=3)
    a = ap.parse_args()
    seen = classes(a.size, a.frames)
    torch.cuda.empty_cache()
    lib = nv.load()
    print("# %d classes, %d conv + BN pairs per pass of both encoders; %d frames of %d x %d, bf16; us per class "
          "instance, mean of %d repeats (spread)" % (len(seen), sum(seen.values()), a.frames, a.size, a.size, a.repeats))
    print("# n h w cin cout k stride pad dil act res bias ldy count | unfolded us (spread) ws | folded generic us "
          "(spread) | folded ws us (spread) | best folded/unfolded | verdict")
    tot_u = tot_f = 0.0
    for key in sorted(seen, key=lambda k: -seen[k]):
        n, h, w, cin, cout, k, stride, pad, dil, act, has_res, has_bias, ldy = key
        oh, ow = ops.out_hw(h, w, k, stride, pad, dil)
        M = n * oh * ow
        torch.manual_seed(0)
        bn = nn.BatchNorm2d(cout).to(dev).eval()
        bn.running_mean.normal_(0, 0.3)
        bn.running_var.uniform_(0.5, 1.5)
        sc, sf = ops.bn_fold_table(bn)
        prelu = torch.tensor([0.25], device=dev) if act == 2 else None
        bias = torch.randn((cout,), device=dev) if has_bias else None
        per = (n * h * w * cin + cout * k * k * cin + (3 + has_res) * M * cout) * 2
        nsets = max(2, min(16, int(600e6 // per) + 1))
        unf, fol = [], []
        for _ in range(nsets):
            x = torch.randn((n * h * w, cin), device=dev).to(dt)
            wf = (torch.randn((cout, k * k * cin), device=dev) * 0.05).to(dt)
            res = torch.randn((M, cout), device=dev).to(dt) if has_res else None
            ybuf = torch.empty((M, ldy), device=dev, dtype=dt)
            y = ybuf[:, :cout]

            def u(x=x, wf=wf, res=res, y=y):
                c, _, _ = ops.conv_fwd(x, n, h, w, wf, cout, k, stride, pad, dil, bias=bias)
                ops.bn_apply(c, ops.bn_stats(c, bn, False), bn, act=act, prelu=prelu, res=res, out=y)

            def f(x=x, wf=wf, res=res, y=y):
                ops.conv_fwd_affine(x, n, h, w, wf, cout, k, stride, pad, dil, sc, sf, act=act, prelu=prelu, res=res,
                                    bias=bias, out=y)
            unf.append(u)
            fol.append(f)
        ws0 = lib.cn_gemm_ws_launches()
        with torch.no_grad():
            unf[0]()
            ws = lib.cn_gemm_ws_launches() > ws0
            ws0 = lib.cn_gemm_ws_launches()
            fol[0]()
            fws = lib.cn_gemm_ws_launches() > ws0      # the folded conv is dispatched to the ws kernel
            tu, tf, tw = [], [], []
            for _ in range(a.repeats):        # alternating, one device
                tu.append(gtime_sets(unf, reps=2) * 1e6)
                lib.cn_gemm_ws_mode(0)
                try:
                    tf.append(gtime_sets(fol, reps=2) * 1e6)
                finally:
                    lib.cn_gemm_ws_mode(1)
                if fws:
                    tw.append(gtime_sets(fol, reps=2) * 1e6)
        mu, mf = sum(tu) / len(tu), sum(tf) / len(tf)
        su, sf_ = (max(tu) - min(tu)) / mu, (max(tf) - min(tf)) / mf
        wtxt = "-"
        if fws:
            mw = sum(tw) / len(tw)
            wtxt = "%.1f (%.3f)" % (mw, (max(tw) - min(tw)) / mw)
            if mw < mf:                        # the verdict is on the faster folded variant
                mf, sf_ = mw, (max(tw) - min(tw)) / mw
        gain = (mu - mf) / mu
        verdict = "folded" if gain > max(su, sf_) else ("unfolded" if -gain > max(su, sf_) else "within the spread")
        tot_u += mu * seen[key]
        tot_f += mf * seen[key]
        print("%d %d %d %d %d %d %d %d %d %d %d %d %d x%d | %.1f (%.3f) %s | %.1f (%.3f) | %s | %.3f | %s" % (
            n, h, w, cin, cout, k, stride, pad, dil, act, has_res, has_bias, ldy, seen[key], mu, su,
            "ws" if ws else "-", sum(tf) / len(tf), (max(tf) - min(tf)) / (sum(tf) / len(tf)), wtxt, mf / mu,
            verdict), flush=True)
        del unf, fol
        torch.cuda.empty_cache()
    print("# sum over the pairs of one pass of both encoders (isolated, cold): unfolded %.2f ms, folded %.2f ms" % (
        tot_u * 1e-3, tot_f * 1e-3))
    print("# lib %s" % nv.build_info())
    return 0


if __name__ == "__main__":
    sys.exit(main())
