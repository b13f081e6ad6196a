"""Whole-sequence inference with the MX-fp8 co-attention (FeatureBank(coatt="mxfp8"),
RGBDSegmentation_RAA.head_a_indexed over bank.mx / bank.dmx, test.py --feature-bank --coatt mxfp8)
at the 65 x 81 input (map 9 x 11, HW = 99).

* wiring, exact: the head over an MX bank is bitwise the same head with ops.coatt_f8_idx replaced
  by the dense ops.coatt_f8 on gathered stacks; one call carries both modalities and the bf16
  indexed co-attention is not run;
* accuracy, measured: mean |x1 - x1_fp32| of the MX-fp8 bank against that of the bf16 bank;
* refusals; test.py with and without --coatt mxfp8 on a written SBM-RGBD tree.
"""
import os
import re

import pytest
import torch

from conftest import golden
import cosnet_amd as C
from cosnet_amd import ops
from cosnet_amd.inference import FeatureBank, segment_sequence
from cosnet_amd.init_recipe import recipe_state_dict, synthetic_inputs

pytestmark = pytest.mark.gpu

SIZE, HW, N = (65, 81), 99, 3

_SD = {}


def state_dict(calib_name, like):
    """The seeded recipe plus a fixture's calibrated BN statistics (computed once per fixture)."""
    if calib_name not in _SD:
        sd = recipe_state_dict(like.state_dict())
        calib = golden(calib_name)
        for k in calib.files:
            sd[k[len("calib/"):]] = torch.from_numpy(calib[k])
        _SD[calib_name] = sd
    return _SD[calib_name]


def make_model(cuda, dtype, calib_name="bn_calibration.npz"):
    m = C.build_model(dtype)
    m.load_state_dict(state_dict(calib_name, m))
    return m.to(cuda).eval() if cuda is not None else m


@pytest.fixture(scope="module")
def bf16_model(cuda):
    return make_model(cuda, torch.bfloat16)


@pytest.fixture(scope="module")
def fp32_model(cuda):
    return make_model(cuda, torch.float32)


def four_frames(cuda, seed):
    """1 target + 3 references, distinct frames."""
    ra, rb, da, db, _, _ = synthetic_inputs(N, SIZE[0], SIZE[1], seed=seed, correlated=False)
    return torch.cat([ra[:1], rb]).to(cuda), torch.cat([da[:1], db]).to(cuda)


# ---- wiring ---------------------------------------------------------------------------------------
def test_mx_bank_head_is_the_dense_fp8_coattention_on_gathered_stacks(cuda, monkeypatch, bf16_model):
    m = bf16_model
    rgbs, deps = four_frames(cuda, 21)
    ia, ib = [0, 0, 0], [1, 2, 3]
    with torch.no_grad():
        m._set_dtype()
        va, geo = m.encoder.features_nhwc(rgbs)
        dd, _ = m.depth_encoder.features_nhwc(deps)
        assert geo == (4, 9, 11)
        bank = FeatureBank.from_features(m, va, dd, geo, SIZE, coatt="mxfp8")
        assert bank.mx is not None and bank.dmx is not None and bank.mx.dtype == torch.uint8
        assert FeatureBank.from_features(m, va, dd, geo, SIZE).mx is None       # default: no images
        fused = []
        real_fused = ops.coatt_fused_idx
        monkeypatch.setattr(ops, "coatt_fused_idx", lambda *a, **k: fused.append(1) or real_fused(*a, **k))
        x1 = m.head_a_indexed(bank, ia, ib)
        wrong = m.head_a_indexed(bank, ia, [1, 1, 1])

        calls = []
        rows = lambda idx: torch.cat([torch.arange(f * HW, (f + 1) * HW) for f in idx]).to(cuda)

        def stand_in(img, img2, t, ia_d, ib_d, p, hw, za, za2=None):
            calls.append((img is bank.mx, img2 is bank.dmx, t, p, hw, za2 is not None))
            ra, rb = rows(ia_d.tolist()), rows(ib_d.tolist())
            for (vt, v), out in (((bank.vat, bank.va), za), ((bank.dat, bank.da), za2)):
                z_a, z_b = torch.empty_like(out), torch.empty_like(out)
                ops.coatt_f8(vt[ra].contiguous(), v[ra].contiguous(), v[rb].contiguous(), p, hw, z_a, z_b)
                out.copy_(z_a)                                                    # z_b is discarded
            return za, za2

        monkeypatch.setattr(ops, "coatt_f8_idx", stand_in)
        ref = m.head_a_indexed(bank, ia, ib)
    torch.cuda.synchronize()
    assert calls == [(True, True, 4, N, HW, True)], calls      # once, both modalities
    assert fused == [], "the bf16 indexed co-attention ran on an MX bank"
    assert x1.shape == (N, 1) + SIZE and x1.dtype == torch.float32
    assert torch.isfinite(x1).all() and x1.min() >= 0 and x1.max() <= 1
    assert torch.equal(x1.view(torch.int32), ref.view(torch.int32)), (x1 - ref).abs().max().item()
    assert not torch.equal(wrong[1], x1[1]) and not torch.equal(wrong[2], x1[2])


# ---- accuracy -------------------------------------------------------------------------------------
# 1.5 x the largest of the three measured ratios (docstring of the test below).  Caveat: at
# HW = 99 both banks' error is the bf16 encoders', so this bound hardly sees the fp8 affinity; the
# bitwise wiring test above and the kernel-level fp64 test carry that weight, and the difference
# shows at 473 x 473 (masks agree with the bf16 bank's on 99.40 % of the pixels).
K = 1.5 * 1.0007


def bank_errors(cuda, bf16_model, fp32_model, seed):
    """(e_bf16, e_mx, agreement_bf16, agreement_mx, x1_bf16, x1_mx): mean |x1 - x1_fp32| and mask
    agreement at 0.5 of the bf16 bank and of the MX-fp8 bank against the fp32 path, one target
    with three references."""
    rgbs, deps = four_frames(cuda, seed)
    run = lambda m, coatt: segment_sequence(m, rgbs, deps, [[1, 2, 3]], targets=[0], coatt=coatt).double().cpu()
    truth = run(fp32_model, "bf16")
    xb, xm = run(bf16_model, "bf16"), run(bf16_model, "mxfp8")
    err = lambda x: (x - truth).abs().mean().item()
    agree = lambda x: ((x > 0.5) == (truth > 0.5)).double().mean().item()
    return err(xb), err(xm), agree(xb), agree(xm), xb, xm


def test_mx_bank_accuracy_against_fp32(cuda, bf16_model, fp32_model):
    """Truth: the fp32 path (pinned to the oracle and the reference by
    tests/test_gpu_feature_bank.py).  The MX-fp8 bank's mean error may exceed the bf16 bank's by
    at most K = 1.5 x the largest ratio measured over three seeds (the margin for seed-to-seed
    spread).  Measured on an MI355X, e_mx / e_bf16 (e_bf16, e_mx; mask agreement 1.0 for both in
    every case):
        seed 21: 1.0007 (3.0432e-04, 3.0452e-04)
        seed 22: 0.9985 (5.3933e-06, 5.3850e-06)
        seed 23: 1.0000 (5.4401e-04, 5.4398e-04)
    so K = 1.5 x 1.0007 = 1.501.  At this input both banks' error is the bf16 encoders': the fp8
    affinity moves x1 by far less (the printed mean |mxfp8 - bf16|), so the ratio sits at 1."""
    eb, em, ab, am, xb, xm = bank_errors(cuda, bf16_model, fp32_model, 21)
    print("65x81, 1 target x 3 references vs fp32: bf16 bank mean |d| %.4e agreement %.5f; "
          "mxfp8 bank mean |d| %.4e agreement %.5f; ratio %.4f (K %.4f); mean |mxfp8 - bf16| %.3e" % (
              eb, ab, em, am, em / eb, K, (xm - xb).abs().mean().item()))
    for x in (xb, xm):
        assert x.shape == (1, 1) + SIZE and torch.isfinite(x).all() and x.min() >= 0 and x.max() <= 1
    assert em <= K * eb, (em, eb, em / eb, K)


# ---- refusals -------------------------------------------------------------------------------------
def test_mx_bank_refusals(cuda, bf16_model, fp32_model):
    g = torch.Generator().manual_seed(3)
    feats = [(torch.randn((2 * HW, 256), generator=g) * 0.5).to(cuda) for _ in range(2)]
    rgbs, deps = four_frames(cuda, 21)
    with torch.no_grad():
        fp32_model._set_dtype()
        with pytest.raises(ValueError):
            FeatureBank.from_features(fp32_model, feats[0], feats[1], (2, 9, 11), SIZE, coatt="mxfp8")
        with pytest.raises(ValueError):
            segment_sequence(fp32_model, rgbs, deps, [[1, 2, 3]], targets=[0], coatt="mxfp8")
        m = bf16_model
        m._set_dtype()
        fb = [f.to(torch.bfloat16) for f in feats]
        with pytest.raises(ValueError):
            FeatureBank.from_features(m, fb[0], fb[1], (2, 9, 11), SIZE, coatt="int4")
        with pytest.raises(ValueError):
            segment_sequence(m, rgbs, deps, [[1, 2, 3]], targets=[0], coatt="int4")
        with pytest.raises(ValueError):   # C = 256 only
            FeatureBank.from_features(m, fb[0][:, :128].contiguous(), fb[1][:, :128].contiguous(),
                                      (2, 9, 11), SIZE, coatt="mxfp8")
        bank = FeatureBank.from_features(m, fb[0], fb[1], (2, 9, 11), SIZE, coatt="mxfp8")
        m.set_fp8(True)
        try:
            with pytest.raises(RuntimeError):   # fp8 encoder convs: a bank would not be well defined
                m.head_a_indexed(bank, [0], [1])
        finally:
            m.set_fp8(False)
        assert m.head_a_indexed(bank, [0], [1]).shape == (1, 1) + SIZE
        half = FeatureBank(bank.va, bank.vat, bank.da, bank.dat, bank.geo, bank.input_size, mx=bank.mx)
        with pytest.raises(ValueError):   # the images of one modality only
            m.head_a_indexed(half, [0], [1])


# ---- test.py --feature-bank --coatt mxfp8 -----------------------------------------------------------
@pytest.fixture(scope="module")
def cli_env(tmp_path_factory):
    """A written SBM-RGBD tree (three sequences of 4-5 frames), a config for it (sample_range 2,
    65 x 81 model input) and a calibrated checkpoint."""
    import yaml
    from test_sbm import _write_tree
    from cosnet_amd.checkpoint import save_snapshot
    root = str(tmp_path_factory.mktemp("feature_bank_mxfp8_cli"))
    data = os.path.join(root, "sbm")
    _write_tree(data, seqs=(("Shadows", "s1", 4), ("OutOfRange", "s2", 5), ("OutOfRange", "s3", 4)))
    ds = {"output_WH": "52,40", "image_HW_4_model": "65, 81", "sample_range": 2, "subset": {},
          "data_path": data}
    cfg = os.path.join(root, "config.yaml")
    with open(cfg, "w") as f:
        yaml.safe_dump({"test": {"model": {"resnet_aspp_add": {"pretrained_params": ""}},
                                 "dataset": {"sbmrgbd": ds}}}, f)
    m = make_model(None, torch.float32)
    return root, cfg, save_snapshot(os.path.join(root, "snapshot.pth"), 1, m)


def _run_cli(env, name, extra):
    import test as test_cli
    top, cfg, ckpt = env
    root = os.path.join(top, name)
    rc = test_cli.main(["--dataset", "sbmrgbd", "--model", "raa", "--gpus", "0", "--feature-bank",
                        "--dtype", "bf16", "--config", cfg, "--checkpoint", ckpt, "--result-root", root] + extra)
    assert rc == 0
    logs, pngs = [], []
    for d, _, files in os.walk(root):
        logs += [os.path.join(d, f) for f in files if f.endswith("_test_log.txt")]
        pngs += [os.path.relpath(os.path.join(d, f), root).split(os.sep, 4)[-1] for f in files if f.endswith(".png")]
    assert len(logs) == 1
    text = open(logs[0]).read()
    frames = re.findall(r"##== seq: (\S+) frame: (\S+) IOU: ([0-9.eE+-]+)==##", text)
    final = re.findall(r"##== final IOU: ([0-9.eE+-]+)==##", text)
    assert len(final) == 1
    return [(s, f) for s, f, _ in frames], [float(v) for _, _, v in frames], float(final[0]), sorted(pngs)


def test_cli_coatt_mxfp8_keeps_lines_order_and_pngs(cuda, cli_env):
    """test.py --feature-bank --dtype bf16 with and without --coatt mxfp8: rc 0, the same seq / frame
    lines in the same order, the same PNG layout, one final-IoU line each.  The IoU difference is
    printed, not asserted (the accuracy of the fp8 affinity is test_mx_bank_accuracy_against_fp32's)."""
    a = _run_cli(cli_env, "bf16", [])
    b = _run_cli(cli_env, "mxfp8", ["--coatt", "mxfp8"])
    assert len(a[0]) == 13 and a[0] == b[0]
    assert a[3] == b[3] and len(a[3]) == 13
    print("sbmrgbd 13 frames: final IOU bf16 bank %.6f, mxfp8 bank %.6f; max per-frame |d| %.2e" % (
        a[2], b[2], max(abs(x - y) for x, y in zip(a[1], b[1]))))
