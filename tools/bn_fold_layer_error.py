"""The eval-mode BN fold (cosnet_amd/bn_fold.py) against the default walk, block by block.

    python tools/bn_fold_layer_error.py [size, default 473]

* fp32: is the folded walk of both encoders bitwise encoder.features_nhwc at this size?
* bf16: x1 of the default and of the folded bank against the fp32 default path, and against each
  other (T = 4 frames, 3 references each);
* bf16, RGB encoder, per block: r = ||a - b|| / ||b|| of the folded block fed the default walk's
  input (local), of both walks from the image (accumulated), and of either walk against fp32.
Seeded recipe weights with the BN statistics of tests/golden/bn_calibration_473.npz.
"""
import os
import random
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import cosnet_amd as C  # noqa: E402
from cosnet_amd import bn_fold as BF  # noqa: E402
from cosnet_amd import encoder_fn as E  # noqa: E402
from cosnet_amd.inference import segment_sequence  # noqa: E402
from cosnet_amd.init_recipe import recipe_state_dict  # noqa: E402

dev = torch.device("cuda:0")
H = int(sys.argv[1]) if len(sys.argv) > 1 else 473
T = 4


def model(dt):
    m = C.build_model(dt)
    sd = recipe_state_dict(m.state_dict())
    z = np.load(os.path.join(REPO, "tests", "golden", "bn_calibration_473.npz"), allow_pickle=False)
    for k in z.files:
        sd[k[len("calib/"):]] = torch.from_numpy(z[k])
    m.load_state_dict(sd)
    return m.to(dev).eval()


g = torch.Generator().manual_seed(0)
mean = torch.tensor([104.00698793, 116.66876762, 122.67891434]).view(1, 3, 1, 1)
rgbs = (torch.rand((T, 3, H, H), generator=g) * 255.0 - mean).to(dev)
deps = (torch.rand((T, 1, H, H), generator=g) * 255.0).to(dev)
rel = lambda a, b: ((a.float() - b.float()).norm() / b.float().norm()).item()

with torch.no_grad():
    m32 = model(torch.float32)
    m32._set_dtype()
    m32.set_bn_fold()
    for name, enc, x in (("encoder", m32.encoder, rgbs[:2]), ("depth_encoder", m32.depth_encoder, deps[:2])):
        ref, geo = enc.features_nhwc(x)
        got, _ = BF.encode_frames_folded(enc, x)
        torch.cuda.synchronize()
        print("fp32 %s %s: bitwise %s, rel %.3e" % (name, geo, torch.equal(ref, got), rel(got, ref)), flush=True)
    m32.set_bn_fold(False)
    rng = random.Random(0)
    refs = [rng.sample(range(T), 3) for _ in range(T)]
    truth = segment_sequence(m32, rgbs, deps, refs).double().cpu()

    mb = model(torch.bfloat16)
    mb._set_dtype()
    default = segment_sequence(mb, rgbs, deps, refs).double().cpu()
    mb.set_bn_fold()
    fold = segment_sequence(mb, rgbs, deps, refs).double().cpu()
    for tag, x in (("default bf16", default), ("folded bf16", fold)):
        print("%s bank vs fp32: mean |d| %.4e, mask agreement %.5f" % (
            tag, (x - truth).abs().mean().item(), ((x > 0.5) == (truth > 0.5)).double().mean().item()))
    print("folded vs default bf16: mean |d| %.4e, mask agreement %.5f" % (
        (fold - default).abs().mean().item(), ((fold > 0.5) == (default > 0.5)).double().mean().item()), flush=True)

    # per block: the folded block fed the default walk's input (local), and both walks from the image
    enc, T_ = mb.encoder, mb.bn_fold.encoders["encoder"]
    x = rgbs[:2]
    xd, geo = E.stem_fwd(enc.backbone, (x,), 1, torch.bfloat16, None)
    xf, _ = BF.stem_folded(enc.backbone, x, torch.bfloat16, T_)
    x32, g32 = E.stem_fwd(m32.encoder.backbone, (x,), 1, torch.float32, None)
    print("stem: folded vs default %.3e; vs fp32: default %.3e folded %.3e" % (rel(xf, xd), rel(xd, x32), rel(xf, x32)))
    for blk, b32 in zip(E.blocks(enc), E.blocks(m32.encoder)):
        loc, _ = BF.bottleneck_folded(blk, xd, geo, T_)
        xf, _ = BF.bottleneck_folded(blk, xf, geo, T_)
        xd, geo2 = E.bottleneck_fwd(blk, xd, geo, 1, None)
        x32, _ = E.bottleneck_fwd(b32, x32, geo, 1, None)
        print("%-22s local %.3e accumulated %.3e | vs fp32: default %.3e folded %.3e" % (
            T_.paths[id(blk.bn1)][:-4], rel(loc, xd), rel(xf, xd), rel(xd, x32), rel(xf, x32)), flush=True)
        geo = geo2
    ad, af = E.aspp_fwd(enc.aspp, xd, geo, 1, None), BF.aspp_folded(enc.aspp, xf, geo, T_)
    a32 = E.aspp_fwd(m32.encoder.aspp, x32, geo, 1, None)
    print("aspp: local %.3e accumulated %.3e | vs fp32: default %.3e folded %.3e" % (
        rel(BF.aspp_folded(enc.aspp, xd, geo, T_), ad), rel(af, ad), rel(ad, a32), rel(af, a32)))
torch.cuda.synchronize()
