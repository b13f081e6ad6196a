"""Per-class timing of the eval-mode BN fold on the static-scale fp8 encoder convs
(cosnet_amd/fp8_infer.py bottleneck_static_folded / aspp_static_folded) against the unfolded static
walk's launches; the fp8 sibling of tools/bn_fold_probe.py.

For every distinct fp8 conv + BN class of both encoders at the bank's shape (473 x 473 frames,
encode_chunk 8; the classes are recorded from one folded walk under a calibration of the same
frames), operands cold as in tools/gemm_cold.py (enough distinct operand sets that every launch
reads from HBM):

    unfolded   conv_fwd_fp8 + bn_stats (eval: cn_bn_eval_params) + bn_apply_q8, as bottleneck_static
    folded     conv_fwd_fp8_affine: one launch

The outputs are the class's own: the e4m3 image only (conv1, conv2, the ASPP branches' concat
slices), bf16 only (the downsample conv, the ASPP bottleneck conv) or both (conv3).  A downsample
conv has no apply of its own in the unfolded walk (conv3's apply reads the raw cd and applies both
BNs), so its unfolded form here is conv_fwd_fp8 + bn_stats, and conv3's unfolded form takes a bf16
residual either way -- the pair's sum is what the walk runs.

Each variant is timed REPEATS times alternating; spread = (max - min) / mean of a variant's
repeats.  A class is 'folded' only where the folded mean is below the unfolded mean by more than
the larger spread.

usage: python tools/fp8_fold_probe.py [--size 473] [--frames 8] [--repeats 3]
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
from cosnet_amd import fp8_infer, ops  # noqa: E402
from cosnet_amd.init_recipe import recipe_state_dict  # noqa: E402

sys.path.insert(0, os.path.join(REPO, "tools"))
from gemm_cold import gtime_sets  # noqa: E402

dev = torch.device("cuda:0")
bf = torch.bfloat16


def classes(size, frames):
    """{(n, h, w, cin, cout, k, stride, pad, dil, act, has_res, has_bias, has_y, has_y8, ldy8): count}
    over the fp8 launches of one folded pass of both encoders."""
    m = C.build_model(bf)
    m.load_state_dict(recipe_state_dict(m.state_dict()))
    m = m.to(dev).eval()
    g = torch.Generator().manual_seed(0)
    rgbs = torch.rand((frames, 3, size, size), generator=g).to(dev)
    deps = torch.rand((frames, 1, size, size), generator=g).to(dev)
    m.set_fp8_static(fp8_infer.calibrate(m, rgbs, deps, frames), fold_bn=True)
    seen = {}
    real = ops.conv_fwd_fp8_affine

    def rec(x8, n, h, w, wf8, cout, k, stride, pad, dil, x_state, w_state, scale, shift, act=0, prelu=None,
            res=None, bias=None, out=None, out8=None, out_state=None, want_y=True):
        has_y8 = out8 is not None or out_state is not None
        key = (n, h, w, wf8.shape[1] // (k * k), cout, k, stride, pad, dil, act, res is not None,
               bias is not None, out is not None or want_y, has_y8,
               (cout if out8 is None else out8.stride(0)) if has_y8 else 0)
        seen[key] = seen.get(key, 0) + 1
        return real(x8, n, h, w, wf8, cout, k, stride, pad, dil, x_state, w_state, scale, shift, act=act,
                    prelu=prelu, res=res, bias=bias, out=out, out8=out8, out_state=out_state, want_y=want_y)

    ops.conv_fwd_fp8_affine = rec
    try:
        with torch.no_grad():
            m._set_dtype()
            fp8_infer.encode_frames_static(m.encoder, rgbs)
            fp8_infer.encode_frames_static(m.depth_encoder, deps)
        torch.cuda.synchronize()
    finally:
        ops.conv_fwd_fp8_affine = real
    return seen


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=473)
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=3)
    a = ap.parse_args()
    seen = classes(a.size, a.frames)
    torch.cuda.empty_cache()
    print("# %d classes, %d fp8 conv + BN pairs per pass of both encoders; %d frames of %d x %d, static fp8; us per "
          "class instance, mean of %d repeats (spread)" % (len(seen), sum(seen.values()), a.frames, a.size, a.size,
                                                          a.repeats))
    print("# n h w cin cout k stride pad dil act res bias y y8 ldy8 count | unfolded us (spread) | folded us (spread) "
          "| folded/unfolded | verdict")
    tot_u = tot_f = 0.0
    state = lambda s: torch.tensor([s, 1.0 / s, 0.0, 448.0], device=dev)
    for key in sorted(seen, key=lambda k: -seen[k]):
        n, h, w, cin, cout, k, stride, pad, dil, act, has_res, has_bias, has_y, has_y8, ldy8 = key
        oh, ow = ops.out_hw(h, w, k, stride, pad, dil)
        M = n * oh * ow
        torch.manual_seed(0)
        bn = nn.BatchNorm2d(cout).to(dev).eval()
        bn.running_mean.normal_(0, 0.3)
        bn.running_var.uniform_(0.5, 1.5)
        sc, sf = ops.bn_fold_table(bn)
        prelu = torch.tensor([0.25], device=dev) if act == 2 else None
        bias = torch.randn((cout,), device=dev) if has_bias else None
        xs, ws, qs = state(4.0 / 448), state(0.2 / 448), state(8.0 / 448)
        per = n * h * w * cin + cout * k * k * cin + (4 + 2 * has_res + 2 * has_y + has_y8) * M * cout
        nsets = max(2, min(16, int(600e6 // per) + 1))
        unf, fol = [], []
        for _ in range(nsets):
            x8 = torch.randint(0, 0x78, (n * h * w, cin), device=dev, dtype=torch.uint8)
            w8 = torch.randint(0, 0x50, (cout, k * k * cin), device=dev, dtype=torch.uint8)
            res = torch.randn((M, cout), device=dev).to(bf) if has_res else None
            y = torch.empty((M, cout), device=dev, dtype=bf) if has_y else None
            y8 = torch.empty((M, ldy8), device=dev, dtype=torch.uint8)[:, :cout] if has_y8 else None

            def u(x8=x8, w8=w8, res=res, y=y, y8=y8):
                c, _, _ = ops.conv_fwd_fp8(x8, n, h, w, w8, cout, k, stride, pad, dil, xs, ws, bias=bias)
                st = ops.bn_stats(c, bn, False)
                if has_y8:
                    ops.bn_apply_q8(c, st, bn, qs, act=act, prelu=prelu, res=res, out=y, out8=y8)
                elif act or has_res:              # bf16 only, with an apply of its own (the ASPP bottleneck conv)
                    ops.bn_apply(c, st, bn, act=act, prelu=prelu, res=res, out=y)

            def f(x8=x8, w8=w8, res=res, y=y, y8=y8):
                ops.conv_fwd_fp8_affine(x8, n, h, w, w8, cout, k, stride, pad, dil, xs, ws, sc, sf, act=act,
                                        prelu=prelu, res=res, bias=bias, out=y, out8=y8,
                                        out_state=qs if has_y8 else None, want_y=has_y)
            unf.append(u)
            fol.append(f)
        with torch.no_grad():
            tu, tf = [], []
            for _ in range(a.repeats):        # alternating, one device
                tu.append(gtime_sets(unf, reps=2) * 1e6)
                tf.append(gtime_sets(fol, reps=2) * 1e6)
        mu, mf = sum(tu) / len(tu), sum(tf) / len(tf)
        su, sf_ = (max(tu) - min(tu)) / mu, (max(tf) - min(tf)) / mf
        gain = (mu - mf) / mu
        verdict = "folded" if gain > max(su, sf_) else ("unfolded" if -gain > max(su, sf_) else "within the spread")
        tot_u += mu * seen[key]
        tot_f += mf * seen[key]
        print("%d %d %d %d %d %d %d %d %d %d %d %d %d %d %d x%d | %.1f (%.3f) | %.1f (%.3f) | %.3f | %s" % (
            n, h, w, cin, cout, k, stride, pad, dil, act, has_res, has_bias, has_y, has_y8, ldy8, seen[key],
            mu, su, mf, sf_, mf / mu, verdict), flush=True)
        del unf, fol
        torch.cuda.empty_cache()
    print("# sum over the fp8 pairs of one pass of both encoders (isolated, cold): unfolded %.2f ms, folded %.2f ms"
          % (tot_u * 1e-3, tot_f * 1e-3))
    print("# lib %s" % nv.build_info())
    return 0


if __name__ == "__main__":
    sys.exit(main())
