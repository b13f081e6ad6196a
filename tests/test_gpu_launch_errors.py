"""The status codes with which the elementwise, BatchNorm, fp8-quantise and co-attention entry
points (csrc/ew.hip, bn.hip, coatt*.hip, fp8.hip) refuse a call.

As in test_gpu_conv_errors.py every case is refused by the host code BEFORE its first launch, so
nothing runs on the device; what is pinned is the code and, where two things are wrong at once,
which check comes first.  The first group is the contract for the fp32 and bf16 codes.  The second
group is the dtype contract: an entry with only fp32 and bf16 kernels refuses every other dtype
code (fp8 is a matrix operand only) before it looks at anything else.  Its calls pass fp32 tensors
for every operand and output, so each buffer covers the widest reading of the stated shape.

Shapes: 16 rows (N = 1, 4 x 4 pixels) of 16 channels; co-attention B = 1, HW = 32, 256 channels.
"""
import types

import pytest
import torch

from cosnet_amd import _native as nv

pytestmark = pytest.mark.gpu

F32, BF = nv.DT_F32, nv.DT_BF16
SHAPE, ALIGN, UNSUPPORTED = r"shape \(-1\)", r"alignment \(-2\)", r"unsupported \(-3\)"
P, C, HW, D = 16, 16, 32, 256
A, F, W = "a", "f", "w"      # a pointer argument: the bf16, the fp32, the byte tensor of `t`


def off(name, nbytes):
    """Pointer `nbytes` past the start of a tensor (a misaligned operand)."""
    return (name, nbytes)


@pytest.fixture(scope="module")
def t(cuda):
    """a: any bf16 operand or output, f: any fp32 one (parameters, statistics, workspaces), w: byte
    images and workspaces.  Each covers the largest shape of this file."""
    return types.SimpleNamespace(
        a=torch.zeros((65536,), dtype=torch.bfloat16, device=cuda),
        f=torch.zeros((65536,), dtype=torch.float32, device=cuda),
        w=torch.zeros((1 << 20,), dtype=torch.uint8, device=cuda))


def build(t, spec, over, wide=False):
    """Arguments of one call: the entry's valid defaults with `over` replacing some.  wide: every
    tensor argument is the fp32 tensor."""
    assert not set(over) - set(spec), set(over) - set(spec)
    out = []
    for v in {**spec, **over}.values():
        name, nbytes = v if isinstance(v, tuple) else (v, 0)
        if name in (A, F, W):
            v = getattr(t, F if wide else name).data_ptr() + nbytes
        out.append(v)
    return out


def refused(words, t, name, spec, **over):
    with pytest.raises(nv.NativeError, match=words):
        nv.call(name, *build(t, spec, over), nv.stream())


# ---- valid calls (bf16), by entry -------------------------------------------------------------------
NHWC = dict(dt=BF, x=F, N=1, C=3, H=4, W=4, Cp=8, y=A)
WPREP = dict(dt=BF, w=F, Cout=C, KHW=1, Cin=C, Cp=C, wf=A, wt=A)
POOL_FWD = dict(dt=BF, x=A, N=1, H=4, W=4, C=C, OH=2, OW=2, k=3, s=2, pad=1, y=A, argmax=W)
POOL_BWD = dict(dt=BF, dy=A, argmax=W, N=1, H=4, W=4, C=C, OH=2, OW=2, k=3, s=2, pad=1, dx=A)
AVGPOOL = dict(dt=BF, x=A, ld=C, N=1, HW=P, C=C, scale=1.0, y=A, ws=F)
BCAST = dict(dt=BF, src=A, N=1, HW=P, C=C, scale=1.0, dst=A, ld=C, accumulate=0)
GATE_FWD = dict(dt=BF, z=A, ldz=C, P=P, C=C, g=F, gb=F, out=A, ldo=C, mask=F)
GATE_CAT = dict(dt=BF, z=A, ldz=C, vbank=A, ldv=C, iv=F, P=1, HW=P, C=C, g=F, gb=F, out=A, ldo=2 * C)
GATE_BWD = dict(dt=BF, z=A, ldz=C, dout=A, lddo=C, mask=F, P=P, C=C, g=F, through_mask=0, dz=A,
                lddz=C, dg=F, dgb=F, ws=F)
HEAD_FWD = dict(dt=BF, a=A, lda=C, b=A, ldb=C, P=P, C=C, relu=1, w=F, bias=F, zout=A, ldz=C, logit=F)
HEAD_BWD = dict(dt=BF, z=A, ldz=C, dlogit=F, P=P, C=C, relu=1, w=F, dz=A, lddz=C, dw=F, db=F, ws=F)
ROWDOT_SEG = dict(dt=BF, a=A, lda=C, b=A, ldb=C, P=P, C=C, seg=P, seg_ld=P, out=F)
ROWDOT = dict(dt=BF, a=A, lda=C, b=A, ldb=C, P=P, C=C, out=F)
COLSUM = dict(dt=BF, x=A, ld=C, P=P, C=C, out=F, ws=F)
CAST = dict(dt_in=F32, dt_out=BF, x=F, ldx=C, P=P, C=C, y=A, ldy=C, accumulate=0)
BN_STATS = dict(dt=BF, x=A, ldx=C, P=P, nseg=1, C=C, mean=F, invstd=F, run_mean=F, run_var=F,
                momentum=0.1, eps=1e-5, ws=F)
BN_BWD_APPLY = dict(dt=BF, x=A, ldx=C, dy=A, lddy=C, P=P, C=C, mean=F, invstd=F, gamma=F, beta=F,
                    sum_dz=F, sum_dzxh=F, dx=A, lddx=C)
BN_APPLY = dict(dt=BF, x=A, ldx=C, P=P, nseg=1, C=C, mean=F, invstd=F, gamma=F, beta=F, res=None,
                ldr=0, xr=None, ldxr=0, rmean=None, rinvstd=None, rgamma=None, rbeta=None, act=1,
                prelu=None, y=A, ldy=C)
BN_APPLY_FP8 = dict(BN_APPLY, y8=None, ldy8=0, qstate=None)
BN_APPLY_EX = dict(BN_APPLY_FP8, mask=None, ldm=0)
BN_BWD = dict(dt=BF, x=A, ldx=C, dy=A, lddy=C, y=A, ldy=C, P=P, C=C, mean=F, invstd=F, gamma=F,
              beta=F, act=1, prelu=None, dgamma=F, dbeta=F, dprelu_c=None, dx=A, lddx=C, dres=None,
              lddres=0, ws=F)
SOFTMAX = dict(dt=BF, S=F, B=1, HW=HW, ld=HW, Pc=A, PT=A, ws=F)
DSCORE = dict(dt=BF, Pc=A, dPc=F, d1=F, PT=A, dPr=F, d2=F, B=1, HW=HW, ld=HW, dS=A)
QUANT_FMT = dict(dt=BF, fmt=0, x=A, ldx=C, P=P, C=C, y8=W, ldy=C, state=F, mode=0)
QUANT = dict(dt=BF, x=A, ldx=C, P=P, C=C, y8=W, ldy=C, state=F, mode=0)
FUSED_WS = dict(vat=A, ld_vat=D, va=A, ld_va=D, vb=A, ld_vb=D, B=1, HW=HW, C=D, za=A, zb=A, ld_z=D,
                ws=None, ws_bytes=0)
FUSED_IDX = dict(vat=A, ld_vat=D, va=A, ld_va=D, vb=A, ld_vb=D, ia=F, ib=F, P=1, HW=HW, C=D, za=A,
                 zb=A, ld_z=D, ws=None, ws_bytes=0)
FLASH_PV = dict(q=A, ldq=D, k=A, ldk=D, v=A, ldv=D, klse=F, B=1, HW=HW, C=D, o=A, ldo=D,
                accumulate=0, ws=None, ws_bytes=0)
FLASH_DVAT = dict(vat=A, ld_vat=D, va=A, ld_va=D, dza=A, ld_dza=D, vb=A, ld_vb=D, dzb=A, ld_dzb=D,
                  lse_a=F, d0=F, lse_b=F, d1=F, B=1, HW=HW, C=D, out=A, ld_out=D, accumulate=0,
                  ws=None, ws_bytes=0)
F8_FWD = dict(vat=A, ld_vat=D, va=A, ld_va=D, vb=A, ld_vb=D, B=1, HW=HW, C=D, za=A, zb=A, ld_z=D,
              lse_a=None, lse_b=None, ws=W, ws_bytes=1 << 20)
F8_TRAIN = dict(vat=A, ld_vat=D, va=A, ld_va=D, vb=A, ld_vb=D, B=1, HW=HW, C=D, za=A, zb=A, ld_z=D,
                lse_a=F, lse_b=F, vat_q=A, va_q=A, vb_q=A, ld_q=D, ws=W, ws_bytes=1 << 20)
F8_BANK = dict(vat=A, ld_vat=D, va=A, ld_va=D, T=1, HW=HW, C=D, img=W, img_bytes=1 << 20)
F8_IDX = dict(img0=W, img1=None, T=1, ia=None, ib=None, P=1, HW=HW, C=D, za0=A, za1=None, ld_z=D)


# ==== group 1: the contract for fp32 and bf16 ===========================================================
# ---- channels that are no multiple of the 16-byte vector -----------------------------------------------
@pytest.mark.parametrize("name, spec, field", [
    ("cn_nchw_to_nhwc", NHWC, "Cp"), ("cn_maxpool_fwd", POOL_FWD, "C"), ("cn_maxpool_bwd", POOL_BWD, "C"),
    ("cn_avgpool", AVGPOOL, "C"), ("cn_bcast_rows", BCAST, "C"), ("cn_gate_fwd", GATE_FWD, "C"),
    ("cn_gate_bwd", GATE_BWD, "C"), ("cn_head_fwd", HEAD_FWD, "C"), ("cn_head_bwd", HEAD_BWD, "C"),
    ("cn_rowdot_seg", ROWDOT_SEG, "C"), ("cn_rowdot", ROWDOT, "C"), ("cn_colsum", COLSUM, "C"),
    ("cn_bn_stats", BN_STATS, "C"), ("cn_bn_bwd_apply", BN_BWD_APPLY, "C"),
    ("cn_bn_apply_ex", BN_APPLY_EX, "C"), ("cn_bn_apply", BN_APPLY, "C"), ("cn_bn_bwd", BN_BWD, "C")])
def test_channels_not_a_vector_multiple(t, name, spec, field):
    refused(ALIGN, t, name, spec, **{field: 12})            # bf16: 8 per chunk
    refused(ALIGN, t, name, spec, dt=F32, **{field: 10})    # fp32: 4 per chunk (12 would pass)


def test_nchw_to_nhwc_misaligned_output(t):
    refused(ALIGN, t, "cn_nchw_to_nhwc", NHWC, y=off(A, 8))


@pytest.mark.parametrize("name, spec, field", [
    ("cn_bn_stats", BN_STATS, "ldx"), ("cn_bn_bwd_apply", BN_BWD_APPLY, "lddy"),
    ("cn_bn_bwd_apply", BN_BWD_APPLY, "lddx"), ("cn_bn_apply_ex", BN_APPLY_EX, "ldy"),
    ("cn_bn_bwd", BN_BWD, "lddy"), ("cn_bn_bwd", BN_BWD, "ldy"), ("cn_bn_bwd", BN_BWD, "lddx")])
def test_bn_row_stride_not_a_vector_multiple(t, name, spec, field):
    refused(ALIGN, t, name, spec, **{field: 20})
    refused(ALIGN, t, name, spec, dt=F32, **{field: 18})


@pytest.mark.parametrize("name, spec, field", [
    ("cn_bn_bwd_apply", BN_BWD_APPLY, "mean"), ("cn_bn_bwd_apply", BN_BWD_APPLY, "sum_dzxh"),
    ("cn_bn_apply_ex", BN_APPLY_EX, "beta"), ("cn_bn_apply_ex", BN_APPLY_EX, "rgamma"),
    ("cn_bn_bwd", BN_BWD, "invstd"), ("cn_bn_bwd", BN_BWD, "dbeta")])
def test_bn_misaligned_parameter_vector(t, name, spec, field):
    refused(ALIGN, t, name, spec, **{field: off(F, 4)})


def test_bn_empty_problem(t):
    refused(SHAPE, t, "cn_bn_stats", BN_STATS, P=0)
    refused(SHAPE, t, "cn_bn_stats", BN_STATS, nseg=0)
    refused(SHAPE, t, "cn_bn_bwd_apply", BN_BWD_APPLY, P=0)
    refused(SHAPE, t, "cn_bn_apply_ex", BN_APPLY_EX, P=0)
    refused(SHAPE, t, "cn_bn_apply_ex", BN_APPLY_EX, nseg=0)
    refused(SHAPE, t, "cn_bn_bwd", BN_BWD, P=0)


def test_bn_alignment_is_checked_before_the_row_count(t):
    refused(ALIGN, t, "cn_bn_stats", BN_STATS, C=12, P=0)
    refused(ALIGN, t, "cn_bn_bwd_apply", BN_BWD_APPLY, mean=off(F, 4), P=0)
    refused(ALIGN, t, "cn_bn_apply_ex", BN_APPLY_EX, mean=off(F, 4), P=0)
    refused(ALIGN, t, "cn_bn_bwd", BN_BWD, mean=off(F, 4), P=0)


def test_bn_apply_fp8_copy_is_bf16_only(t):
    refused(ALIGN, t, "cn_bn_apply_ex", BN_APPLY_EX, dt=F32, y8=W, ldy8=C, qstate=F)
    refused(ALIGN, t, "cn_bn_apply_fp8", BN_APPLY_FP8, dt=F32, y8=W, ldy8=C, qstate=F)


def test_bn_apply_fp8_copy_needs_state_stride_and_alignment(t):
    refused(ALIGN, t, "cn_bn_apply_ex", BN_APPLY_EX, y8=W, ldy8=C, qstate=None)
    refused(ALIGN, t, "cn_bn_apply_ex", BN_APPLY_EX, y8=W, ldy8=24, qstate=F)
    refused(ALIGN, t, "cn_bn_apply_ex", BN_APPLY_EX, y8=off(W, 4), ldy8=C, qstate=F)


def test_bn_apply_mask_rows_too_short(t):
    refused(SHAPE, t, "cn_bn_apply_ex", BN_APPLY_EX, mask=W, ldm=1)    # C / 8 = 2 bytes per row
    refused(SHAPE, t, "cn_bn_apply_ex", BN_APPLY_EX, dt=F32, x=F, y=F, mask=W, ldm=3)


def test_bn_apply_order_of_checks(t):
    # the fp8 copy, then the mask, then the channel count
    refused(ALIGN, t, "cn_bn_apply_ex", BN_APPLY_EX, dt=F32, y8=W, ldy8=C, qstate=F, mask=W, ldm=1)
    refused(SHAPE, t, "cn_bn_apply_ex", BN_APPLY_EX, C=12, mask=W, ldm=0)


def test_bn_bwd_mask_activation_needs_its_mask(t):
    refused(SHAPE, t, "cn_bn_bwd", BN_BWD, act=4, y=None, ldy=0)
    refused(SHAPE, t, "cn_bn_bwd", BN_BWD, act=4, y=W, ldy=1)
    # ... which is looked at after the strides and before the parameter vectors
    refused(ALIGN, t, "cn_bn_bwd", BN_BWD, act=4, y=None, ldy=0, lddy=20)
    refused(SHAPE, t, "cn_bn_bwd", BN_BWD, act=4, y=None, ldy=0, mean=off(F, 4))


# ---- gate and head ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name, spec", [("cn_gate_bwd", GATE_BWD), ("cn_head_bwd", HEAD_BWD)])
def test_backward_takes_one_chunk_per_lane(t, name, spec):
    big = dict(C=8 * 65, ldz=8 * 65, lddz=8 * 65)
    refused(UNSUPPORTED, t, name, spec, **big)
    refused(UNSUPPORTED, t, name, spec, dt=F32, C=4 * 65, ldz=4 * 65, lddz=4 * 65)
    refused(UNSUPPORTED, t, name, spec, ws=None, **big)     # before the missing workspace
    refused(ALIGN, t, name, spec, C=8 * 65 + 4)             # after the vector multiple


def test_backward_parameter_gradients_need_the_workspace(t):
    refused(SHAPE, t, "cn_gate_bwd", GATE_BWD, ws=None)
    refused(SHAPE, t, "cn_gate_bwd", GATE_BWD, ws=None, dg=None)
    refused(SHAPE, t, "cn_head_bwd", HEAD_BWD, ws=None)
    refused(SHAPE, t, "cn_head_bwd", HEAD_BWD, ws=None, dw=None)


def test_gate_cat_idx(t):
    refused(SHAPE, t, "cn_gate_cat_idx", GATE_CAT, ldo=C)
    refused(SHAPE, t, "cn_gate_cat_idx", GATE_CAT, P=0)
    refused(SHAPE, t, "cn_gate_cat_idx", GATE_CAT, C=12, ldo=C)       # shape before alignment
    refused(ALIGN, t, "cn_gate_cat_idx", GATE_CAT, ldv=20)
    refused(ALIGN, t, "cn_gate_cat_idx", GATE_CAT, vbank=off(A, 8))
    refused(ALIGN, t, "cn_gate_cat_idx", GATE_CAT, iv=off(F, 2))
    wide = dict(C=8 * 65, ldz=8 * 65, ldv=8 * 65, ldo=16 * 65)
    refused(UNSUPPORTED, t, "cn_gate_cat_idx", GATE_CAT, **wide)
    refused(ALIGN, t, "cn_gate_cat_idx", GATE_CAT, z=off(A, 8), **wide)  # alignment before the width
    refused(SHAPE, t, "cn_gate_cat_idx", GATE_CAT, P=1 << 20, HW=1 << 12)


def test_rowdot_segments(t):
    refused(SHAPE, t, "cn_rowdot_seg", ROWDOT_SEG, seg=8, seg_ld=4)
    refused(SHAPE, t, "cn_rowdot_seg", ROWDOT_SEG, seg=0)
    refused(ALIGN, t, "cn_rowdot_seg", ROWDOT_SEG, C=12, seg=8, seg_ld=4)   # alignment first


# ---- co-attention scores and fp8 quantisation --------------------------------------------------------------
def test_coatt_softmax_row_stride(t):
    refused(ALIGN, t, "cn_coatt_softmax", SOFTMAX, ld=HW + 4)
    refused(ALIGN, t, "cn_coatt_softmax", SOFTMAX, ld=HW - 8)
    refused(ALIGN, t, "cn_coatt_softmax", SOFTMAX, dt=F32, Pc=F, PT=F, ld=HW - 8)


def test_fp8_quant(t):
    refused(ALIGN, t, "cn_fp8_quant_fmt", QUANT_FMT, C=12)
    refused(ALIGN, t, "cn_fp8_quant_fmt", QUANT_FMT, dt=F32, x=F, ldx=12)
    refused(ALIGN, t, "cn_fp8_quant_fmt", QUANT_FMT, state=None)
    refused(ALIGN, t, "cn_fp8_quant", QUANT, ldy=12)
    refused(UNSUPPORTED, t, "cn_fp8_quant_fmt", QUANT_FMT, fmt=2)
    refused(SHAPE, t, "cn_fp8_quant_fmt", QUANT_FMT, mode=3)
    refused(ALIGN, t, "cn_fp8_quant_fmt", QUANT_FMT, C=12, fmt=2)          # alignment, format, mode
    refused(UNSUPPORTED, t, "cn_fp8_quant_fmt", QUANT_FMT, fmt=2, mode=3)


# ---- fused / flash co-attention ------------------------------------------------------------------------------
@pytest.mark.parametrize("name, spec, q, ldq", [
    ("cn_coatt_fused_fwd_ws", FUSED_WS, "vat", "ld_vat"), ("cn_coatt_fused_fwd_idx", FUSED_IDX, "vb", "ld_vb"),
    ("cn_coatt_flash_pv_ws", FLASH_PV, "k", "ldk")])
def test_fused_operands(t, name, spec, q, ldq):
    refused(SHAPE, t, name, spec, C=128)
    refused(SHAPE, t, name, spec, **{"B" if "B" in spec else "P": 0})
    refused(ALIGN, t, name, spec, **{ldq: D + 4})
    refused(ALIGN, t, name, spec, **{ldq: D - 8})
    refused(ALIGN, t, name, spec, **{q: off(A, 8)})
    refused(SHAPE, t, name, spec, C=128, **{ldq: D + 4})      # the channel count first


def test_fused_outputs(t):
    refused(ALIGN, t, "cn_coatt_fused_fwd_ws", FUSED_WS, za=off(A, 4))
    refused(ALIGN, t, "cn_coatt_fused_fwd_ws", FUSED_WS, ld_z=D + 2)
    refused(SHAPE, t, "cn_coatt_fused_fwd_ws", FUSED_WS, za=None, zb=None)
    refused(ALIGN, t, "cn_coatt_fused_fwd_idx", FUSED_IDX, ia=off(F, 2))
    refused(SHAPE, t, "cn_coatt_flash_pv_ws", FLASH_PV, klse=None)
    refused(SHAPE, t, "cn_coatt_flash_pv_ws", FLASH_PV, o=None)
    refused(ALIGN, t, "cn_coatt_flash_pv_ws", FLASH_PV, klse=off(F, 8))
    refused(ALIGN, t, "cn_coatt_flash_pv_ws", FLASH_PV, o=off(A, 4))


def test_flash_dvat(t):
    refused(SHAPE, t, "cn_coatt_flash_dvat_ws", FLASH_DVAT, C=128)
    refused(SHAPE, t, "cn_coatt_flash_dvat_ws", FLASH_DVAT, out=None)
    refused(SHAPE, t, "cn_coatt_flash_dvat_ws", FLASH_DVAT, dza=None, dzb=None)
    refused(SHAPE, t, "cn_coatt_flash_dvat_ws", FLASH_DVAT, lse_a=None)
    refused(SHAPE, t, "cn_coatt_flash_dvat_ws", FLASH_DVAT, va=None)
    refused(ALIGN, t, "cn_coatt_flash_dvat_ws", FLASH_DVAT, ld_dza=D + 4)
    refused(ALIGN, t, "cn_coatt_flash_dvat_ws", FLASH_DVAT, ld_out=D + 2)
    refused(ALIGN, t, "cn_coatt_flash_dvat_ws", FLASH_DVAT, dzb=off(A, 8))
    refused(ALIGN, t, "cn_coatt_flash_dvat_ws", FLASH_DVAT, d1=off(F, 8))
    refused(ALIGN, t, "cn_coatt_flash_dvat_ws", FLASH_DVAT, out=off(A, 4))
    refused(SHAPE, t, "cn_coatt_flash_dvat_ws", FLASH_DVAT, lse_a=None, ld_dza=D + 4)   # nulls first


# ---- MX-fp8 co-attention ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name, spec, ws, nbytes, need", [
    ("cn_coatt_f8_fwd", F8_FWD, "ws", "ws_bytes", "cn_coatt_f8_workspace_bytes"),
    ("cn_coatt_f8_train_fwd", F8_TRAIN, "ws", "ws_bytes", "cn_coatt_f8_train_workspace_bytes"),
    ("cn_coatt_f8_bank_build", F8_BANK, "img", "img_bytes", "cn_coatt_f8_bank_bytes")])
def test_f8_workspace(t, name, spec, ws, nbytes, need):
    need = int(nv.query(need, 1, HW))
    assert 0 < need <= t.w.numel() - 256
    refused(SHAPE, t, name, spec, **{ws: None})
    refused(SHAPE, t, name, spec, **{ws: off(W, 16)})
    refused(SHAPE, t, name, spec, **{nbytes: need - 1})
    refused(ALIGN, t, name, spec, **{ws: None, "ld_vat": D + 4})     # the operands first
    refused(SHAPE, t, name, spec, **{ws: None, "C": 128})


@pytest.mark.parametrize("name, spec", [("cn_coatt_f8_fwd", F8_FWD), ("cn_coatt_f8_train_fwd", F8_TRAIN),
                                        ("cn_coatt_f8_bank_build", F8_BANK)])
def test_f8_operands(t, name, spec):
    refused(SHAPE, t, name, spec, C=128)
    refused(SHAPE, t, name, spec, HW=0)
    refused(ALIGN, t, name, spec, ld_va=D + 4)
    refused(ALIGN, t, name, spec, vat=off(A, 8))


def test_f8_outputs_and_copies(t):
    refused(SHAPE, t, "cn_coatt_f8_fwd", F8_FWD, zb=None)
    refused(ALIGN, t, "cn_coatt_f8_fwd", F8_FWD, za=off(A, 4))
    refused(ALIGN, t, "cn_coatt_f8_fwd", F8_FWD, ld_z=D + 2)
    refused(SHAPE, t, "cn_coatt_f8_train_fwd", F8_TRAIN, lse_b=None)
    refused(SHAPE, t, "cn_coatt_f8_train_fwd", F8_TRAIN, va_q=None)
    refused(ALIGN, t, "cn_coatt_f8_train_fwd", F8_TRAIN, ld_q=D - 8)
    refused(ALIGN, t, "cn_coatt_f8_train_fwd", F8_TRAIN, vb_q=off(A, 8))
    refused(SHAPE, t, "cn_coatt_f8_bank_build", F8_BANK, va=None)
    refused(ALIGN, t, "cn_coatt_f8_bank_build", F8_BANK, ld_vat=D - 8)


def test_f8_fwd_idx(t):
    refused(SHAPE, t, "cn_coatt_f8_fwd_idx", F8_IDX, img0=None)
    refused(SHAPE, t, "cn_coatt_f8_fwd_idx", F8_IDX, za1=A)           # a second output without its bank
    refused(SHAPE, t, "cn_coatt_f8_fwd_idx", F8_IDX, P=2)             # no maps: pair p is frame p
    refused(ALIGN, t, "cn_coatt_f8_fwd_idx", F8_IDX, ld_z=D - 4)
    refused(ALIGN, t, "cn_coatt_f8_fwd_idx", F8_IDX, img0=off(W, 16))
    refused(ALIGN, t, "cn_coatt_f8_fwd_idx", F8_IDX, za0=off(A, 4))
    refused(SHAPE, t, "cn_coatt_f8_fwd_idx", F8_IDX, P=2, img0=off(W, 16))


# ==== group 2: dtype codes other than fp32 and bf16 ========================================================
TYPED = [("cn_nchw_to_nhwc", NHWC), ("cn_weight_prep", WPREP), ("cn_maxpool_fwd", POOL_FWD),
         ("cn_maxpool_bwd", POOL_BWD), ("cn_avgpool", AVGPOOL), ("cn_bcast_rows", BCAST),
         ("cn_gate_fwd", GATE_FWD), ("cn_gate_cat_idx", GATE_CAT), ("cn_gate_bwd", GATE_BWD),
         ("cn_head_fwd", HEAD_FWD), ("cn_head_bwd", HEAD_BWD), ("cn_rowdot_seg", ROWDOT_SEG),
         ("cn_rowdot", ROWDOT), ("cn_colsum", COLSUM), ("cn_bn_stats", BN_STATS),
         ("cn_bn_bwd_apply", BN_BWD_APPLY), ("cn_bn_apply", BN_APPLY), ("cn_bn_apply_fp8", BN_APPLY_FP8),
         ("cn_bn_apply_ex", BN_APPLY_EX), ("cn_bn_bwd", BN_BWD), ("cn_coatt_softmax", SOFTMAX),
         ("cn_coatt_dscore", DSCORE), ("cn_fp8_quant_fmt", QUANT_FMT), ("cn_fp8_quant", QUANT)]


@pytest.mark.parametrize("dt", [2, 7])
@pytest.mark.parametrize("name, spec", TYPED, ids=[n for n, _ in TYPED])
def test_only_fp32_and_bf16(t, name, spec, dt):
    with pytest.raises(nv.NativeError, match=UNSUPPORTED):
        nv.call(name, *build(t, spec, dict(dt=dt), wide=True), nv.stream())


def test_only_fp32_and_bf16_is_the_first_check(t):
    for name, spec, over in [("cn_maxpool_fwd", POOL_FWD, dict(C=10)), ("cn_bn_stats", BN_STATS, dict(P=0)),
                             ("cn_gate_cat_idx", GATE_CAT, dict(P=0)), ("cn_fp8_quant_fmt", QUANT_FMT, dict(C=12))]:
        with pytest.raises(nv.NativeError, match=UNSUPPORTED):
            nv.call(name, *build(t, spec, dict(over, dt=2), wide=True), nv.stream())


@pytest.mark.parametrize("dt_in, dt_out", [(0, 2), (2, 0), (1, 2), (2, 2), (0, 7), (7, 1), (3, 3), (-1, 0)])
def test_cast2d_pairs_off_the_table(t, dt_in, dt_out):
    with pytest.raises(nv.NativeError, match=UNSUPPORTED):
        nv.call("cn_cast2d", *build(t, CAST, dict(dt_in=dt_in, dt_out=dt_out), wide=True), nv.stream())
