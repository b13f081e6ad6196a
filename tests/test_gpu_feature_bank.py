"""Whole-sequence inference (cosnet_amd.inference.FeatureBank / segment_sequence,
RGBDSegmentation_RAA.head_a_indexed, test.py --feature-bank): every frame encoded once, the
(target, reference) pairs of test.py:287-305 formed by index.

* cn_gate_cat_idx and cn_mean_groups bitwise against the kernels they stand in for;
* the bf16 indexed head against head_nhwc on stacked copies of the same features;
* segment_sequence in fp32 against the CPU oracle's loop mean in fp64 (the project's rule: 8 x the
  oracle's own fp32-vs-fp64 floor) and against the reference's configs[3] fixture;
* test.py with and without --feature-bank on a written SBM-RGBD tree.
"""
import os
import re
import zlib

import numpy as np
import pytest
import torch

from conftest import golden
import cosnet_amd as C
from cosnet_amd import _native as nv
from cosnet_amd import ops
from cosnet_amd.inference import FeatureBank, segment_sequence
from cosnet_amd.init_recipe import recipe_state_dict, synthetic_inputs

pytestmark = pytest.mark.gpu


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


def make_model(cuda, dtype, calib_name):
    m = C.build_model(dtype)
    m.load_state_dict(state_dict(calib_name, m))
    return m.to(cuda).eval() if cuda is not None else m


@pytest.fixture(scope="module")
def bf16_model(cuda):
    return make_model(cuda, torch.bfloat16, "bn_calibration.npz")


# ---- cn_gate_cat_idx -------------------------------------------------------------------------------
@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_gate_cat_idx_is_bitwise_gate_then_copy(cuda, dtype, bias):
    """P = 3 pairs of a 9 x 11 map (the 65 x 81 input's), strided z and bank rows, a bank with an
    unused NaN frame, a repeated frame and a non-monotone map, output in a sentinel buffer."""
    p, hw, c, t = 3, 99, 256, 4
    iv = [2, 0, 2]
    g = torch.Generator().manual_seed(17 + bias)
    zbuf = torch.full((p * hw, c + 64), float("nan")).to(dtype).to(cuda)
    z = zbuf[:, 32:32 + c]
    z.copy_(torch.randn((p * hw, c), generator=g).to(dtype))
    bbuf = torch.full((t * hw, 2 * c), float("nan")).to(dtype).to(cuda)
    bank = bbuf[:, c:]
    x = torch.randn((t * hw, c), generator=g).to(dtype)
    x[1 * hw:2 * hw] = float("nan")          # frame 1 is named by no pair
    bank.copy_(x)
    gw = (torch.randn((1, c, 1, 1), generator=g) * 0.1).to(cuda)
    gb = torch.tensor([0.3], device=cuda) if bias else None
    # the kernels it stands in for: cn_gate_fwd, then a copy of the gathered rows
    ref = torch.empty((p * hw, 2 * c), dtype=dtype, device=cuda)
    nv.call("cn_gate_fwd", nv.dtype_code(dtype), z.data_ptr(), ops.ld(z), p * hw, c,
            gw.reshape(-1).data_ptr(), nv.ptr(gb), ref.data_ptr(), 2 * c, None, nv.stream())
    for i, f in enumerate(iv):
        ops.cast_copy(bank[f * hw:(f + 1) * hw], ref[i * hw:(i + 1) * hw, c:])
    sent = 77.0
    obuf = torch.full((p * hw + 4, 2 * c + 16), sent, dtype=dtype, device=cuda)
    out = obuf[2:2 + p * hw, :2 * c]
    r = ops.gate_cat_idx(z, bank, torch.tensor(iv, dtype=torch.int32, device=cuda), p, hw, gw, gb, out=out)
    torch.cuda.synchronize()
    assert r is out and torch.isfinite(ref.float()).all()
    it = torch.int16 if dtype == torch.bfloat16 else torch.int32
    assert torch.equal(out.contiguous().view(it), ref.view(it))
    assert (obuf[:2] == sent).all() and (obuf[2 + p * hw:] == sent).all() and (obuf[:, 2 * c:] == sent).all()
    # NULL map: frame p
    dense = torch.nan_to_num(bank[:p * hw].float(), nan=1.0).to(dtype)
    out2 = ops.gate_cat_idx(z, dense, None, p, hw, gw, gb)
    torch.cuda.synchronize()
    assert torch.equal(out2[:, :c].contiguous().view(it), ref[:, :c].contiguous().view(it))
    assert torch.equal(out2[:, c:], dense)


# ---- cn_mean_groups ---------------------------------------------------------------------------------
@pytest.mark.parametrize("groups,n,c", [(1, 5, 4097), (3, 2, 5265)])
def test_mean_groups_is_bitwise_mean_rows_per_group(cuda, groups, n, c):
    g = torch.Generator().manual_seed(c)
    x = torch.rand((groups * n, c), generator=g).to(cuda)
    got = ops.mean_groups(x, groups, n)
    ref = torch.empty((groups, c), dtype=torch.float32, device=cuda)
    for k in range(groups):
        nv.call("cn_mean_rows", x[k * n:(k + 1) * n].data_ptr(), n, c, ref[k].data_ptr(), nv.stream())
    torch.cuda.synchronize()
    assert torch.equal(got.view(torch.int32), ref.view(torch.int32))


# ---- the indexed head, bf16 --------------------------------------------------------------------------
def test_head_a_indexed_bf16_matches_head_nhwc_on_stacked_copies(cuda, monkeypatch, bf16_model):
    """1 target + 3 references at 65 x 81 encoded once; the bank is built from those very tensors,
    so only the head differs: indexed a-side kernels vs head_nhwc on a 3-way stack.  Bound of the
    same comparison at configs[3] (test_nref5_473_bf16_fused_in_pipeline).  A wrong b map must
    show in the output (the comparison is not blind to the frames a pair names)."""
    m = bf16_model
    ra, rb, da, db, _, _ = synthetic_inputs(3, 65, 81, seed=21, correlated=False)
    rgbs = torch.cat([ra[:1], rb]).to(cuda)
    deps = torch.cat([da[:1], db]).to(cuda)
    n, hw, size = 3, 99, (65, 81)
    calls = []
    real = ops.coatt_fused_idx
    monkeypatch.setattr(ops, "coatt_fused_idx",
                        lambda *a, **k: calls.append((a[5], k.get("za") is not None, k.get("zb"))) or real(*a, **k))
    with torch.no_grad():
        m._set_dtype()
        va, geo = m.encoder.features_nhwc(rgbs)
        dd, _ = m.depth_encoder.features_nhwc(deps)
        assert geo == (4, 9, 11)
        bank = FeatureBank.from_features(m, va, dd, geo, size)
        x1 = m.head_a_indexed(bank, torch.tensor([0, 0, 0], dtype=torch.int32),
                              torch.tensor([1, 2, 3], dtype=torch.int32))
        got = ops.mean_groups(x1.view(n, size[0] * size[1]), 1, n)
        wrong = m.head_a_indexed(bank, [0, 0, 0], [1, 1, 1])
        va_n, da_n = (torch.cat([x[:hw]] * n).contiguous() for x in (va, dd))
        r1, _ = m.head_nhwc(va_n, va[hw:].contiguous(), da_n, dd[hw:].contiguous(), (n, 9, 11), size)
        ref = torch.empty_like(got)
        nv.call("cn_mean_rows", r1.contiguous().data_ptr(), n, size[0] * size[1], ref.data_ptr(), nv.stream())
    torch.cuda.synchronize()
    assert calls[:2] == [(n, True, None), (n, True, None)] and len(calls) == 4, calls   # RGB, depth: a side only
    assert not torch.equal(wrong[1], x1[1]) and not torch.equal(wrong[2], x1[2])
    assert x1.shape == (n, 1) + size and x1.dtype == torch.float32
    f, g = got.double().cpu(), ref.double().cpu()
    assert torch.isfinite(f).all() and f.min() >= 0 and f.max() <= 1
    agree = ((f > 0.5) == (g > 0.5)).double().mean().item()
    mad = (f - g).abs().mean().item()
    print("indexed head vs head_nhwc, bf16 65x81: mask agreement %.5f, mean |d| %.3e" % (agree, mad))
    assert agree >= 0.999 and mad <= 1e-2, (agree, mad)


def test_head_a_indexed_refuses_training_grad_fp8_and_bad_maps(cuda, bf16_model):
    m = bf16_model
    g = torch.Generator().manual_seed(2)
    feats = [(torch.randn((2 * 99, 256), generator=g) * 0.5).to(torch.bfloat16).to(cuda) for _ in range(2)]
    with torch.no_grad():
        m._set_dtype()
        bank = FeatureBank.from_features(m, feats[0], feats[1], (2, 9, 11), (65, 81))
    with pytest.raises(RuntimeError):
        m.head_a_indexed(bank, [0], [1])                 # grad mode
    with torch.no_grad():
        with pytest.raises(ValueError):
            m.head_a_indexed(bank, [0], [2])             # outside the bank
        with pytest.raises(ValueError):
            m.head_a_indexed(bank, [0, 1], [1])
        m.set_fp8(True)
        with pytest.raises(RuntimeError):
            m.head_a_indexed(bank, [0], [1])
        m.set_fp8(False)
        m.train()
        try:
            with pytest.raises(RuntimeError):
                m.head_a_indexed(bank, [0], [1])
        finally:
            m.eval()


# ---- segment_sequence, fp32, against the oracle ------------------------------------------------------
def test_segment_sequence_fp32_matches_oracle_loop_mean(cuda):
    """T = 4 frames at 65 x 81, refs with a repeat (target 1) and a self-reference (target 2).
    Truth: oracle.model_ref.RefModel in eval mode in fp64 on the CPU, the reference's loop per
    target (test.py:287-305: x1 of each (target, reference) forward summed in order, / N).  Floor:
    the same oracle in fp32 against its fp64; bound 8 x floor + 1e-5, masks equal outside it."""
    from oracle.model_ref import RefModel
    refs = [[1, 2], [0, 0], [3, 2], [2, 1]]
    ra, rb, da, db, _, _ = synthetic_inputs(2, 65, 81, seed=33, correlated=False)
    rgbs, deps = torch.cat([ra, rb]), torch.cat([da, db])          # 4 distinct frames
    m = make_model(cuda, torch.float32, "bn_calibration.npz")
    sd = _SD["bn_calibration.npz"]
    got = segment_sequence(m, rgbs.to(cuda), deps.to(cuda), refs, encode_chunk=3, pair_chunk=4)
    torch.cuda.synchronize()
    assert got.shape == (4, 1, 65, 81) and got.dtype == torch.float32
    ta = [t for t, r in enumerate(refs) for _ in r]
    tb = [j for r in refs for j in r]
    truth = {}
    for dt in (torch.float64, torch.float32):
        ref = RefModel(sd, dtype=dt, requires_grad=False)
        ref.training = False
        with torch.no_grad():   # eval mode is per-sample: the 8 forwards as one batch
            x1, _, _ = ref.forward(rgbs[ta].to(dt), rgbs[tb].to(dt), deps[ta].to(dt), deps[tb].to(dt))
        x1 = x1.reshape(4, 2, 65 * 81)
        acc = x1[:, 0].clone()
        acc += x1[:, 1]
        truth[dt] = (acc / 2).double().numpy()
    r64 = truth[torch.float64]
    floor = float(np.abs(truth[torch.float32] - r64).max())
    tol = 8 * floor + 1e-5
    g = got.double().cpu().numpy().reshape(4, -1)
    for t in range(4):                                              # every target, none skipped
        err = float(np.abs(g[t] - r64[t]).max())
        print("segment_sequence fp32 target %d: max err %.3e (tol %.3e, oracle floor %.3e)" % (t, err, tol, floor))
        assert err <= tol, (t, err, tol, floor)
        amb = np.abs(r64[t] - 0.5) <= tol
        flips = ((g[t] > 0.5) != (r64[t] > 0.5)) & ~amb
        assert not flips.any(), (t, int(flips.sum()))


def test_segment_sequence_fp32_nref5_473_matches_reference(cuda):
    """configs[3] through the bank: [target, five references], refs [[1..5]], against the reference's
    loop mean in fp64 (the fixture, inputs, bound and flip check of
    test_gpu_configs.py::test_nref5_473_fp32_matches_reference)."""
    z = golden("nref5_473.npz")
    ra, rb, da, db, _, _ = synthetic_inputs(5, 473, 473, seed=5)
    crc = [zlib.crc32(t.numpy().tobytes()) for t in (ra, rb, da, db)]
    assert crc == list(z["in_crc32"]), "synthetic input generator drifted"
    m = make_model(cuda, torch.float32, "bn_calibration_473.npz")
    got = segment_sequence(m, torch.cat([ra[:1], rb]).to(cuda), torch.cat([da[:1], db]).to(cuda),
                           [[1, 2, 3, 4, 5]], targets=[0])
    torch.cuda.synchronize()
    g = got.double().cpu().numpy().reshape(z["f64r/x1mean"].shape)
    ref = z["f64r/x1mean"].astype(np.float64)
    floor = float(z["floor/x1mean"][0])
    tol = 8 * floor + 1e-5
    err = float(np.abs(g - ref).max())
    print("segment_sequence fp32 configs[3]: max err %.3e (tol %.3e)" % (err, tol))
    assert err <= tol, (err, tol, floor)
    amb = np.abs(ref - 0.5) <= tol
    flips = ((g > 0.5) != (ref > 0.5)) & ~amb
    assert not flips.any(), int(flips.sum())


# ---- test.py --feature-bank ----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cli_env(tmp_path_factory):
    """A written SBM-RGBD tree (three sequences of 4-5 frames), a config for it and for a small
    synthetic set (sample_range 2, 65 x 81 model input) and a calibrated checkpoint."""
    import yaml
    from test_sbm import _write_tree
    from cosnet_amd.checkpoint import save_snapshot
    root = str(tmp_path_factory.mktemp("feature_bank_cli"))
    data = os.path.join(root, "sbm")
    _write_tree(data, seqs=(("Shadows", "s1", 4), ("OutOfRange", "s2", 5), ("OutOfRange", "s3", 4)))
    ds = {"output_WH": "52,40", "image_HW_4_model": "65, 81", "sample_range": 2, "subset": {}}
    cfg = os.path.join(root, "config.yaml")
    with open(cfg, "w") as f:
        yaml.safe_dump({"test": {"model": {"resnet_aspp_add": {"pretrained_params": ""}},
                                 "dataset": {"sbmrgbd": dict(ds, data_path=data),
                                             "synthetic": dict(ds, data_path="", frames=3)}}}, f)
    m = make_model(None, torch.float32, "bn_calibration.npz")
    return root, cfg, save_snapshot(os.path.join(root, "snapshot.pth"), 1, m)


def _run_cli(env, dataset, name, extra):
    import test as test_cli
    top, cfg, ckpt = env
    root = os.path.join(top, dataset + "_" + name)
    rc = test_cli.main(["--dataset", dataset, "--model", "raa", "--gpus", "0", "--dtype", "fp32",
                        "--config", cfg, "--checkpoint", ckpt, "--result-root", root] + extra)
    assert rc == 0
    logs, pngs = [], []
    for d, _, files in os.walk(root):
        logs += [os.path.join(d, f) for f in files if f.endswith("_test_log.txt")]
        pngs += [os.path.relpath(os.path.join(d, f), root).split(os.sep, 4)[-1] for f in files if f.endswith(".png")]
    text = open(logs[0]).read()
    frames = re.findall(r"##== seq: (\S+) frame: (\S+) IOU: ([0-9.eE+-]+)==##", text)
    final = re.findall(r"##== final IOU: ([0-9.eE+-]+)==##", text)
    assert len(final) == 1
    return [(s, f) for s, f, _ in frames], [float(v) for _, _, v in frames], float(final[0]), sorted(pngs)


@pytest.mark.parametrize("dataset,nframes", [("sbmrgbd", 13), ("synthetic", 3)])
def test_cli_feature_bank_matches_per_target_path(cuda, cli_env, dataset, nframes):
    """test.py with and without --feature-bank, fp32, sample_range 2: the same seq / frame lines in
    the same order, the same PNG layout, and final IoUs within 0.002 (0.2 J points on the x100
    scale).  sbmrgbd: every sequence's frames loaded and encoded once; synthetic: each target forms
    a bank of itself and its own search frames."""
    a = _run_cli(cli_env, dataset, "per_target", [])
    b = _run_cli(cli_env, dataset, "bank", ["--feature-bank"])
    assert len(a[0]) == nframes and a[0] == b[0]
    assert a[3] == b[3] and len(a[3]) == nframes
    print("%s: final IOU per-target %.6f, feature bank %.6f; max per-frame |d| %.2e" % (
        dataset, a[2], b[2], max(abs(x - y) for x, y in zip(a[1], b[1]))))
    assert abs(a[2] - b[2]) <= 0.002, (a[2], b[2])
