"""The kernels of static-scale fp8 inference (cosnet_amd/fp8_infer.py): cn_fp8_quant_static,
cn_bn_apply_q8 and cn_bcast_rows_u8.

* cn_fp8_quant_static: the bytes of torch's e4m3fn conversion of x * state[1] and bitwise those of
  the delayed mode on a copy of the state; the state (with a sentinel in its amax slot) untouched;
* cn_bn_apply_q8: y8 bitwise that of cn_bn_apply_fp8 for a copy of the state, y (when asked for)
  bitwise that of cn_bn_apply, nothing written where a NULL y would be, qstate untouched;
* the refusals of both entries.
"""
import pytest
import torch

from cosnet_amd import _native as nv
from cosnet_amd import ops

pytestmark = pytest.mark.gpu

SENTINEL = 123.0
SHAPE, ALIGN, UNSUPPORTED = -1, -2, -3


def frozen_state(cuda, scale, fmt=ops.FP8_E4M3):
    """[scale, 1/scale, sentinel, format max]: a frozen state whose amax slot would show a write."""
    inv = (torch.tensor(1.0) / torch.tensor(scale, dtype=torch.float32)).item()
    return torch.tensor([scale, inv, SENTINEL, ops.FMT_MAX[fmt]], dtype=torch.float32, device=cuda)


def bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else
                               torch.int16 if t.dtype == torch.bfloat16 else torch.uint8)


# ---- cn_fp8_quant_static ---------------------------------------------------------------------------
@pytest.mark.parametrize("p,c,pad,dt,fmt,big", [
    (1, 8, 0, torch.bfloat16, 0, False),
    (1, 8, 0, torch.float32, 0, False),
    (67, 320, 24, torch.bfloat16, 0, False),
    (67, 320, 24, torch.float32, 0, False),
    (67, 320, 24, torch.bfloat16, 1, False),     # e5m2
    (67, 320, 24, torch.float32, 0, True),       # |x| above the scale's range
])
def test_quant_static_bytes_and_readonly_state(cuda, p, c, pad, dt, fmt, big):
    g = torch.Generator().manual_seed(100 * p + c + fmt)
    x = torch.randn((p, c), generator=g) * 3.0
    scale = 0.03125 if not big else 1e-5          # big: |x| / scale far above 448 almost everywhere
    xbuf = torch.zeros((p, c + pad), dtype=dt, device=cuda)
    xv = xbuf[:, :c]
    xv.copy_(x.to(dt))
    st = frozen_state(cuda, scale, fmt)
    before = st.clone()
    poison = 0xA5
    ybuf = torch.full((p, c + pad), poison, dtype=torch.uint8, device=cuda)
    yv = ybuf[:, :c]
    r = ops.fp8_quant_static(xv, st, out=yv, fmt=fmt)
    # the delayed mode on a copy of the state
    st2 = before.clone()
    ref = ops.fp8_quant(xv, st2, ops.FP8_DELAYED, fmt=fmt)
    torch.cuda.synchronize()
    assert r is yv
    assert torch.equal(bits(st), bits(before)), "cn_fp8_quant_static wrote its state"
    assert torch.equal(yv.contiguous(), ref)
    if pad:
        assert (ybuf[:, c:] == poison).all()
    tdt, fmax = (torch.float8_e4m3fn, 448.0) if fmt == 0 else (torch.float8_e5m2, 57344.0)
    emu = (xv.float().cpu() * before[1].cpu()).clamp(-fmax, fmax).to(tdt)
    got = yv.contiguous().cpu().view(tdt)
    assert torch.equal(got.view(torch.uint8), emu.view(torch.uint8))
    assert not torch.isnan(got.float()).any()
    if big:
        assert (got.float().abs() == fmax).float().mean().item() > 0.99
        assert got.float().min().item() == -fmax and got.float().max().item() == fmax


# ---- cn_bn_apply_q8 ----------------------------------------------------------------------------------
class _BN:
    """What ops.bn_apply reads of a BatchNorm module."""

    def __init__(self, c, g, cuda):
        self.affine = True
        self.weight = (torch.rand((c,), generator=g) + 0.5).to(cuda)
        self.bias = (torch.randn((c,), generator=g) * 0.3).to(cuda)


def _stats(c, g, cuda):
    return ((torch.randn((c,), generator=g) * 0.2).to(cuda), (torch.rand((c,), generator=g) + 0.5).to(cuda))


@pytest.mark.parametrize("p,c,act,extra", [
    (5, 64, 1, None),
    (99, 320, 0, None),          # 256 % (320 / 8) != 0: threads past the chunk columns
    (99, 320, 2, None),          # PReLU
    (700, 2048, 1, "res"),
    (99, 256, 1, "xr"),
])
def test_bn_apply_q8_matches_the_delayed_kernel(cuda, p, c, act, extra):
    g = torch.Generator().manual_seed(7 * p + c + act)
    x = (torch.randn((p, c), generator=g) * 2.0).to(torch.bfloat16).to(cuda)
    bn, stats = _BN(c, g, cuda), _stats(c, g, cuda)
    kw = {}
    if extra == "res":
        kw["res"] = torch.randn((p, c), generator=g).to(torch.bfloat16).to(cuda)
    if extra == "xr":
        kw.update(xr=torch.randn((p, c), generator=g).to(torch.bfloat16).to(cuda), rstats=_stats(c, g, cuda),
                  rbn=_BN(c, g, cuda))
    prelu = torch.tensor([0.25], device=cuda) if act == 2 else None
    st = frozen_state(cuda, 0.0234375)
    before = st.clone()
    # the existing kernels: cn_bn_apply (y) and cn_bn_apply_fp8 on a copy of the state (y8)
    y_ref = ops.bn_apply(x, stats, bn, act=act, prelu=prelu, **kw)
    ref8 = torch.empty((p, c), dtype=torch.uint8, device=cuda)
    y_ref2 = ops.bn_apply(x, stats, bn, act=act, prelu=prelu, out8=ref8, qstate=before.clone(), **kw)
    # with y
    y = torch.full((p, c), 7.0, dtype=torch.bfloat16, device=cuda)
    ry, y8 = ops.bn_apply_q8(x, stats, bn, st, act=act, prelu=prelu, out=y, **kw)
    # without: a poisoned buffer where y would be (same shape and stride) stays as it is
    poison = torch.full((p, c), 7.0, dtype=torch.bfloat16, device=cuda)
    rn, y8n = ops.bn_apply_q8(x, stats, bn, st, act=act, prelu=prelu, **kw)
    torch.cuda.synchronize()
    assert ry is y and rn is None
    assert torch.equal(bits(y_ref), bits(y_ref2))
    assert torch.equal(bits(y), bits(y_ref))
    assert torch.equal(y8, ref8) and torch.equal(y8n, ref8)
    assert (poison == 7.0).all()
    assert torch.equal(bits(st), bits(before)), "cn_bn_apply_q8 wrote qstate"
    assert len(torch.unique(ref8)) > 16          # the comparison is not of constant bytes


def test_bn_apply_q8_into_a_slice_of_the_concat_image(cuda):
    """y8 as the 512-column slice at column 512 of a [99][2560] byte buffer; y = NULL."""
    p, c = 99, 512
    g = torch.Generator().manual_seed(5)
    x = (torch.randn((p, c), generator=g) * 2.0).to(torch.bfloat16).to(cuda)
    bn, stats = _BN(c, g, cuda), _stats(c, g, cuda)
    st = frozen_state(cuda, 0.0234375)
    before = st.clone()
    ref8 = torch.empty((p, c), dtype=torch.uint8, device=cuda)
    ops.bn_apply(x, stats, bn, act=1, out8=ref8, qstate=before.clone())
    poison = 0x5A
    cat8 = torch.full((p, 2560), poison, dtype=torch.uint8, device=cuda)
    _, y8 = ops.bn_apply_q8(x, stats, bn, st, act=1, out8=cat8[:, 512:1024])
    torch.cuda.synchronize()
    assert ops.ld(y8) == 2560
    assert torch.equal(cat8[:, 512:1024].contiguous(), ref8)
    assert (cat8[:, :512] == poison).all() and (cat8[:, 1024:] == poison).all()
    assert torch.equal(bits(st), bits(before))


def test_bcast_rows_u8(cuda):
    n, hw, c = 3, 99, 512
    g = torch.Generator().manual_seed(9)
    src = torch.randint(0, 256, (n, c), generator=g, dtype=torch.uint8).to(cuda)
    poison = 0x5A
    cat8 = torch.full((n * hw, 2560), poison, dtype=torch.uint8, device=cuda)
    ops.bcast_rows_u8(src, n, hw, cat8[:, :512])
    torch.cuda.synchronize()
    assert torch.equal(cat8[:, :512].contiguous(), src.repeat_interleave(hw, dim=0))
    assert (cat8[:, 512:] == poison).all()


# ---- refusals ----------------------------------------------------------------------------------------
def test_refusals(cuda):
    p, c = 8, 64
    xb = torch.zeros((p + 1, c), dtype=torch.bfloat16, device=cuda)
    xf = torch.zeros((p + 1, c), dtype=torch.float32, device=cuda)
    y8 = torch.zeros((p + 1, c), dtype=torch.uint8, device=cuda)
    yb = torch.zeros((p + 1, c), dtype=torch.bfloat16, device=cuda)
    st = frozen_state(cuda, 1.0)
    f = torch.zeros((c + 4,), dtype=torch.float32, device=cuda)
    s = nv.stream()

    def quant(dt=nv.DT_BF16, fmt=0, x=xb.data_ptr(), ldx=c, P=p, C=c, y=y8.data_ptr(), ldy=c,
              state=st.data_ptr()):
        return nv.query("cn_fp8_quant_static", dt, fmt, x, ldx, P, C, y, ldy, state, s)

    assert quant() == 0
    assert quant(C=12) == ALIGN
    assert quant(ldx=c + 4) == ALIGN
    assert quant(ldy=c + 4) == ALIGN
    assert quant(state=None) == ALIGN
    assert quant(x=xb.data_ptr() + 2) == ALIGN
    assert quant(y=y8.data_ptr() + 4) == ALIGN
    assert quant(fmt=2) == UNSUPPORTED
    assert quant(dt=2) == UNSUPPORTED
    assert quant(ldx=c - 8) == SHAPE
    assert quant(P=0) == 0

    def apply(dt=nv.DT_BF16, x=xb.data_ptr(), ldx=c, P=p, nseg=1, C=c, mean=f.data_ptr(),
              y=yb.data_ptr(), ldy=c, out8=y8.data_ptr(), ldy8=c, q=st.data_ptr(), res=None, ldr=0):
        return nv.query("cn_bn_apply_q8", dt, x, ldx, P, nseg, C, mean, f.data_ptr(), None, None, res, ldr,
                        None, 0, None, None, None, None, 1, None, y, ldy, out8, ldy8, q, s)

    assert apply() == 0
    assert apply(y=None, ldy=0) == 0
    assert apply(dt=nv.DT_F32, x=xf.data_ptr()) == ALIGN          # fp32 input
    assert apply(q=None) == ALIGN
    assert apply(out8=None) == ALIGN
    assert apply(ldy8=c + 8) == ALIGN                               # ldy8 % 16
    assert apply(out8=y8.data_ptr() + 4) == ALIGN
    assert apply(C=c - 4) == ALIGN
    assert apply(ldx=c + 4) == ALIGN
    assert apply(ldy=c + 4) == ALIGN
    assert apply(res=xb.data_ptr(), ldr=c + 4) == ALIGN
    assert apply(mean=f.data_ptr() + 4) == ALIGN
    assert apply(P=0) == SHAPE
    assert apply(nseg=0) == SHAPE
    assert apply(dt=2) == UNSUPPORTED
    torch.cuda.synchronize()
