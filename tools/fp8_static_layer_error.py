"""Per-layer error of the static-scale fp8 encoder walk (cosnet_amd/fp8_infer.py) against the
bf16 walk, on the seeded recipe with a fixture's calibrated BN statistics.

    python tools/fp8_static_layer_error.py [--size 473 | --size 65x81] [--frames 4]

For every bottleneck and for the ASPP, r = ||y_fp8 - y_bf16|| / ||y_bf16|| of the block's output:
  local        the static block fed the bf16 walk's input (the error one block adds);
  accumulated  both walks from the image (what the next block sees).
Also the calibrated amax of the block's input, the bf16 output's max and mean |y| and the share of
saturated bytes (|code| = 448) in the output's e4m3 image.  Calibrated on the frames it encodes.
"""
import argparse
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import cosnet_amd as C  # noqa: E402
from cosnet_amd import encoder_fn as E  # noqa: E402
from cosnet_amd import fp8_infer as FI  # noqa: E402
from cosnet_amd import ops  # noqa: E402
from cosnet_amd.init_recipe import BGR_MEAN, recipe_state_dict  # noqa: E402


def rel(a, b):
    a, b = a.double(), b.double()
    return ((a - b).norm() / b.norm()).item()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="473")
    ap.add_argument("--frames", type=int, default=4)
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("fp8_static_layer_error: needs the GPU")
    H, W = (int(v) for v in (a.size.split("x") if "x" in a.size else (a.size, a.size)))
    dev = torch.device("cuda:0")
    m = C.build_model(torch.bfloat16)
    sd = recipe_state_dict(m.state_dict())
    fixture = "bn_calibration_473.npz" if (H, W) == (473, 473) else "bn_calibration.npz"
    z = np.load(os.path.join(REPO, "tests", "golden", fixture), allow_pickle=False)
    for k in z.files:
        sd[k[len("calib/"):]] = torch.from_numpy(z[k])
    m.load_state_dict(sd)
    m = m.to(dev).eval()
    g = torch.Generator().manual_seed(a.seed)
    mean = torch.tensor(BGR_MEAN, dtype=torch.float32).view(1, 3, 1, 1)
    rgbs = (torch.rand((a.frames, 3, H, W), generator=g) * 255.0 - mean).to(dev)
    deps = (torch.rand((a.frames, 1, H, W), generator=g) * 255.0).to(dev)
    calib = FI.calibrate(m, rgbs, deps)
    m.set_fp8_static(calib)
    m._set_dtype()
    print("# %d frames of %d x %d, seed %d, BN statistics of %s" % (a.frames, H, W, a.seed, fixture))
    for key, imgs in (("encoder", rgbs), ("depth_encoder", deps)):
        enc = getattr(m, key)
        S = enc._cn_fp8_static
        blocks = E.blocks(enc)
        with torch.no_grad(), E.no_fp8():
            xb, geo = E.stem_fwd(enc.backbone, (imgs,), 1, torch.bfloat16, None)
            xs, gs = xb, geo
            xs8 = ops.fp8_quant_static(xb, S.st(S.paths[id(blocks[0])] + ".x"))
            for i, blk in enumerate(blocks):
                nm = S.paths[id(blk)]
                nxt = S.st(S.paths[id(blocks[i + 1] if i + 1 < len(blocks) else enc.aspp)] + ".x")
                yl, _, _ = FI.bottleneck_static(blk, xb, ops.fp8_quant_static(xb, S.st(nm + ".x")), geo, S, nxt)
                xs, xs8, gs = FI.bottleneck_static(blk, xs, xs8, gs, S, nxt)
                xb, geo = E.bottleneck_fwd(blk, xb, geo, 1, None)
                sat = (xs8 & 0x7f).eq(0x7e).float().mean().item()
                print("%s %-20s local %.4f accumulated %.4f  amax(in) %.3g  bf16 out max %.3g mean %.3g  "
                      "saturated %.4f" % (key, nm, rel(yl, xb), rel(xs, xb), calib.amax[key][nm + ".x"],
                                          xb.float().abs().max().item(), xb.float().abs().mean().item(), sat),
                      flush=True)
            ob = E.aspp_fwd(enc.aspp, xb, geo, 1, None)
            ol = FI.aspp_static(enc.aspp, xb, ops.fp8_quant_static(xb, S.st("aspp.x")), geo, S)
            oa = FI.aspp_static(enc.aspp, xs, xs8, gs, S)
            print("%s %-20s local %.4f accumulated %.4f  amax(in) %.3g  amax(concat) %.3g" % (
                key, "aspp", rel(ol, ob), rel(oa, ob), calib.amax[key]["aspp.x"], calib.amax[key]["aspp.cat"]),
                flush=True)
    torch.cuda.synchronize()
    return 0


if __name__ == "__main__":
    sys.exit(main())
