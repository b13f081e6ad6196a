"""The split bank head (model.set_head_split, head_a_indexed(split=True), segment_sequence(head=
"split"), test.py --split-reduce) on the GPU:

* wiring, bitwise: the head equals its composition written out with the ops calls on gathered
  stacks -- co-attention, cn_gate_fwd, conv_fwd_partial over the bank, conv_fwd_affine_add through
  the map -- in bf16 and fp32, on an MX bank and with the BN fold active;
* the per-frame partials do not depend on how the frames are chunked;
* fp32 against the fp64 oracle's loop mean, the bound and flip check of
  test_gpu_feature_bank.py::test_segment_sequence_fp32_matches_oracle_loop_mean;
* the bf16 split head against the default bf16 head on the same bank, the bound between two bf16
  heads of test_head_a_indexed_bf16_matches_head_nhwc_on_stacked_copies;
* the refusals, and the command line on the 13-frame SBM-RGBD tree.
"""
import numpy as np
import pytest
import torch

from cosnet_amd import _native as nv
from cosnet_amd import functions as fn
from cosnet_amd import ops
from cosnet_amd.inference import FeatureBank, plan_pairs, segment_sequence
from cosnet_amd.init_recipe import synthetic_inputs
from cosnet_amd.rgbd_segmentation_RAA import _gather_frames

import test_gpu_feature_bank as B
from test_gpu_feature_bank import _run_cli, cli_env, make_model   # noqa: F401  (cli_env: a fixture)

pytestmark = pytest.mark.gpu

REFS = [[1, 2], [0, 0], [3, 2], [2, 1]]      # a repeat (target 1) and a self-reference (target 2)
SIZE, GEO, HW = (65, 81), (4, 9, 11), 99


@pytest.fixture(scope="module")
def frames():
    ra, rb, da, db, _, _ = synthetic_inputs(2, 65, 81, seed=33, correlated=False)
    return torch.cat([ra, rb]), torch.cat([da, db])          # 4 distinct frames


def written_out(m, bank, ia, ib, tables):
    """head_a_indexed(split=True) as its ops calls on gathered stacks."""
    t, h, w = bank.geo
    hw = h * w
    p = ia.shape[0]
    dev = bank.va.device
    ia_d, ib_d = ia.to(dev), ib.to(dev)
    ia_h, ib_h = ia.tolist(), ib.tolist()
    geo = (p, h, w)
    zs = []
    sides = ((bank.va, bank.vat, m.gate, m.reduce_channels_A, m.bn_A),
             (bank.da, bank.dat, m.depth_gate, m.depth_reduce_channels, m.depth_bn))
    if bank.mx is not None:
        zas = [torch.empty((p * hw, 256), dtype=torch.bfloat16, device=dev) for _ in sides]
        ops.coatt_f8_idx(bank.mx, bank.dmx, t, ia_d, ib_d, p, hw, zas[0], zas[1])
    for k, (v, vt, gate, reduce, bn) in enumerate(sides):
        c = v.shape[1]
        cout = reduce.weight.shape[0]
        va_s, vat_s, vb_s = (_gather_frames(x, idx, hw) for x, idx in ((v, ia_h), (vt, ia_h), (v, ib_h)))
        if bank.mx is not None:
            za = zas[k]
        elif v.dtype == torch.bfloat16:
            za = torch.empty((p * hw, c), dtype=v.dtype, device=dev)
            ops.coatt_fused_idx(vat_s, va_s, vb_s, None, None, p, hw, za=za, zb=None)
        else:
            za = fn.coatt_a_materialised(vat_s, vb_s, p, hw)
        gz = torch.empty_like(za)
        nv.call("cn_gate_fwd", nv.dtype_code(za.dtype), za.data_ptr(), c, p * hw, c, gate.weight.reshape(-1).data_ptr(),
                nv.ptr(gate.bias), gz.data_ptr(), c, None, nv.stream())
        wf, _ = ops.WCACHE.get(reduce.weight, v.dtype)
        w3 = wf.view(cout, 9, 2 * c)
        wz, wv = (w3[:, :, i * c:(i + 1) * c].reshape(cout, 9 * c).contiguous() for i in range(2))
        u, _, _ = ops.conv_fwd_partial(v, t, h, w, wv, cout, 3, 1, 1, 1)
        sc, sf = tables(bn)
        zs.append(ops.conv_fwd_affine_add(gz, p, h, w, wz, cout, 3, 1, 1, 1, sc, sf, u, hw, add_map=ia_d, act=0)[0])
    z_a, dz_a = zs
    dz_a = fn.ConvFn.apply(dz_a, m.depth_weights.weight, m.depth_weights.bias, geo, 1, 1, 0, 1)
    la = fn.HeadFn.apply(z_a, dz_a, m.segmentation_classifier_A.weight, m.segmentation_classifier_A.bias, True)
    return fn.UpSigFn.apply(la, geo, bank.input_size)


# ---- wiring -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,coatt,fold", [(torch.bfloat16, "bf16", False), (torch.float32, "bf16", False),
                                              (torch.bfloat16, "mxfp8", False), (torch.bfloat16, "bf16", True),
                                              (torch.float32, "bf16", True)],
                         ids=["bf16", "fp32", "bf16-mx-bank", "bf16-bn-fold", "fp32-bn-fold"])
def test_split_head_is_bitwise_its_written_out_composition(cuda, frames, dtype, coatt, fold):
    m = make_model(cuda, dtype, "bn_calibration.npz")
    if fold:
        m.set_bn_fold()
    m.set_head_split()
    ia, ib = plan_pairs(4, list(range(4)), REFS)
    with torch.no_grad():
        bank = FeatureBank.encode(m, frames[0].to(cuda), frames[1].to(cuda), encode_chunk=3, coatt=coatt)
        assert bank.geo == GEO and bank.partials is None and (bank.mx is not None) == (coatt == "mxfp8")
        x1 = m.head_a_indexed(bank, ia, ib, split=True)
        assert bank.partials is not None and all(u.dtype == torch.float32 and u.shape == (4 * HW, 256)
                                                 for u in bank.partials)
        if fold:
            assert m.head_split.tables() is m.bn_fold.head
            tables = m.bn_fold.head.get
        else:
            tables = ops.bn_fold_table
        want = written_out(m, bank, ia, ib, tables)
        wrong = m.head_a_indexed(bank, torch.roll(ia, 2), ib, split=True)     # another a-role frame per pair
    torch.cuda.synchronize()
    assert x1.shape == (8, 1) + SIZE and x1.dtype == torch.float32 and torch.isfinite(x1).all()
    assert torch.equal(x1, want)
    assert not torch.equal(wrong, x1)


def test_partials_do_not_depend_on_the_chunking(cuda):
    m = make_model(cuda, torch.bfloat16, "bn_calibration.npz").set_head_split()
    g = torch.Generator().manual_seed(5)
    va, da = ((torch.randn((4 * HW, 256), generator=g) * 0.5).to(torch.bfloat16).to(cuda) for _ in range(2))
    with torch.no_grad():
        m._set_dtype()
        one = FeatureBank.from_features(m, va, da, GEO, SIZE).reduce_partials(m, frame_chunk=8)
        bank3 = FeatureBank.from_features(m, va, da, GEO, SIZE)
        three = bank3.reduce_partials(m, frame_chunk=3)
        assert bank3.reduce_partials(m) is three                   # kept on the bank
    torch.cuda.synchronize()
    for a, b in zip(one, three):
        assert torch.isfinite(a).all() and a.abs().max() > 0 and torch.equal(a, b)


# ---- fp32 against the oracle -----------------------------------------------------------------------------
def test_segment_sequence_split_fp32_matches_oracle_loop_mean(cuda, frames):
    """test_segment_sequence_fp32_matches_oracle_loop_mean with head="split": the fp64 oracle's loop
    mean per target, bound 8 x the oracle's own fp32 floor + 1e-5, masks equal outside that band."""
    from oracle.model_ref import RefModel
    rgbs, deps = frames
    m = make_model(cuda, torch.float32, "bn_calibration.npz").set_head_split()
    sd = B._SD["bn_calibration.npz"]
    got = segment_sequence(m, rgbs.to(cuda), deps.to(cuda), REFS, encode_chunk=3, pair_chunk=4, head="split")
    torch.cuda.synchronize()
    assert got.shape == (4, 1, 65, 81) and got.dtype == torch.float32
    ta = [t for t, r in enumerate(REFS) for _ in r]
    tb = [j for r in REFS for j in r]
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
        print("segment_sequence fp32 split head, target %d: max err %.3e (tol %.3e, oracle floor %.3e)" % (
            t, err, tol, floor))
        assert err <= tol, (t, err, tol, floor)
        amb = np.abs(r64[t] - 0.5) <= tol
        flips = ((g[t] > 0.5) != (r64[t] > 0.5)) & ~amb
        assert not flips.any(), (t, int(flips.sum()))


# ---- bf16: split head against the default head --------------------------------------------------------------
@pytest.mark.parametrize("coatt", ["bf16", "mxfp8"])
def test_split_head_bf16_matches_the_default_head_on_the_same_bank(cuda, frames, coatt):
    """The same bank, the two heads: mask agreement >= 0.999 and mean |d| <= 1e-2 on the per-target
    means (the bound between two bf16 heads on the same features)."""
    m = make_model(cuda, torch.bfloat16, "bn_calibration.npz").set_head_split()
    ia, ib = plan_pairs(4, list(range(4)), REFS)
    with torch.no_grad():
        bank = FeatureBank.encode(m, frames[0].to(cuda), frames[1].to(cuda), coatt=coatt)
        n = SIZE[0] * SIZE[1]
        f = ops.mean_groups(m.head_a_indexed(bank, ia, ib, split=True).view(8, n), 4, 2)
        g = ops.mean_groups(m.head_a_indexed(bank, ia, ib).view(8, n), 4, 2)
    torch.cuda.synchronize()
    f, g = f.double().cpu(), g.double().cpu()
    assert torch.isfinite(f).all() and f.min() >= 0 and f.max() <= 1
    agree = ((f > 0.5) == (g > 0.5)).double().mean().item()
    mad = (f - g).abs().mean().item()
    print("split head vs default head, bf16 65x81 %s: mask agreement %.5f, mean |d| %.3e, max |d| %.3e" % (
        coatt, agree, mad, (f - g).abs().max().item()))
    assert agree >= 0.999 and mad <= 1e-2, (agree, mad)


# ---- refusals -------------------------------------------------------------------------------------------------
def test_split_head_refusals(cuda, frames):
    m = make_model(cuda, torch.bfloat16, "bn_calibration.npz")
    g = torch.Generator().manual_seed(2)
    feats = [(torch.randn((2 * HW, 256), generator=g) * 0.5).to(torch.bfloat16).to(cuda) for _ in range(2)]
    with torch.no_grad():
        m._set_dtype()
        bank = FeatureBank.from_features(m, feats[0], feats[1], (2, 9, 11), SIZE)
        with pytest.raises(RuntimeError, match="set_head_split"):
            m.head_a_indexed(bank, [0], [1], split=True)
        with pytest.raises(RuntimeError, match="set_head_split"):
            segment_sequence(m, frames[0].to(cuda), frames[1].to(cuda), REFS, head="split")
    with pytest.raises(ValueError, match="head"):
        segment_sequence(m, frames[0].to(cuda), frames[1].to(cuda), REFS, head="halves")
    m.train()
    try:
        with pytest.raises(RuntimeError, match="eval"):
            m.set_head_split()
    finally:
        m.eval()
    assert m.set_head_split().head_split is not None
    with pytest.raises(RuntimeError):
        m.head_a_indexed(bank, [0], [1], split=True)                 # grad mode
    with torch.no_grad():
        with pytest.raises(ValueError):
            m.head_a_indexed(bank, [0], [2], split=True)             # outside the bank
        m.set_fp8(True)
        try:
            with pytest.raises(RuntimeError, match="fp8"):
                m.head_a_indexed(bank, [0], [1], split=True)
        finally:
            m.set_fp8(False)
        m.train()
        try:
            with pytest.raises(RuntimeError):
                m.head_a_indexed(bank, [0], [1], split=True)
        finally:
            m.eval()
        x1 = m.head_a_indexed(bank, [0], [1], split=True)            # the same call, valid: runs
        assert m.set_head_split(False).head_split is None
        assert torch.isfinite(x1).all() and torch.isfinite(m.head_a_indexed(bank, [0], [1])).all()


# ---- test.py --feature-bank --split-reduce -----------------------------------------------------------------------
def test_cli_split_reduce_matches_the_default_bank(cuda, cli_env):
    """The 13-frame SBM-RGBD tree, fp32: the same seq / frame lines in the same order, the same PNG
    layout, and final IoUs within 0.002 of the default bank's."""
    a = _run_cli(cli_env, "sbmrgbd", "bank_cat", ["--feature-bank"])
    b = _run_cli(cli_env, "sbmrgbd", "bank_split", ["--feature-bank", "--split-reduce"])
    assert len(a[0]) == 13 and a[0] == b[0]
    assert a[3] == b[3] and len(a[3]) == 13
    print("sbmrgbd: final IOU default bank %.6f, split head %.6f; max per-frame |d| %.2e" % (
        a[2], b[2], max(abs(x - y) for x, y in zip(a[1], b[1]))))
    assert abs(a[2] - b[2]) <= 0.002, (a[2], b[2])
