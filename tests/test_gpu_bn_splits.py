"""Batch norm (bn.hip) past one row split, on channel-slice views: P = 2 * 31 * 37 = 2294 rows
gives every pass several row blocks (gridDim.y > 1), so the UNR-rows-in-flight tails, the S > 1
partial planes and -- at C = 320 -- the 32-lane stride over more than 32 splits all run against
the fp64 reference.  Every activation operand is the column slice [V, V + C) of a buffer with
ld = C + 3 V; outputs go into sentinel-filled buffers whose other columns must not change.
"""
import pytest
import torch
import torch.nn.functional as F

import test_gpu_kernels as K
from cosnet_amd import _native as nv
from cosnet_amd import ops

pytestmark = pytest.mark.gpu

TOL, close, rnd, nhwc, nchw = K.TOL, K.close, K.rnd, K.nhwc, K.nchw
DTS = [torch.float32, torch.bfloat16]
N, H, W = 2, 31, 37
P = N * H * W
SENT = 123.0


def vec(dt):
    return 8 if dt == torch.bfloat16 else 4


def sliced(vals, dt, dev, fill=SENT):
    """vals [P, C] (CPU) as the column slice [V, V + C) of a [P, C + 3 V] buffer of `fill`."""
    p, c = vals.shape
    v = vec(dt)
    buf = torch.full((p, c + 3 * v), fill, dtype=dt, device=dev)
    view = buf[:, v:v + c]
    view.copy_(vals.to(dt))
    return buf, view


def blank(p, c, dt, dev):
    return sliced(torch.full((p, c), SENT, dtype=torch.float64), dt, dev)


def outside_unchanged(buf, c, dt):
    v = vec(dt)
    return bool((buf[:, :v] == SENT).all()) and bool((buf[:, v + c:] == SENT).all())


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("c", [64, 320])
def test_the_shapes_are_multi_split(dt, c, cuda):
    """cn_bn_workspace_floats = C * max(2 * statistics splits, 3 * backward splits)."""
    per_c = int(nv.query("cn_bn_workspace_floats", nv.dtype_code(dt), P, c, 1)) / c
    assert per_c > 3
    if c == 320:
        assert per_c > 3 * 32   # more than 32 splits in at least one of the two reductions


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("act", [0, 1, 2])
@pytest.mark.parametrize("c", [64, 320])
def test_batchnorm_train_multi_split_slices(cuda, dt, act, c):
    """test_batchnorm_train's checks with x and dy read from slices, y and dx written into slices.
    act 1: the reference backward takes the GPU's own ReLU mask, dz = gy * (y_gpu > 0), so that no
    tolerance has to absorb a flipped mask bit; the mask itself may differ from the fp64 one only
    where |t_ref| <= TOL * max |t_ref|, which is what the forward tolerance allows."""
    x = (rnd((N, c, H, W), dt, 9, scale=2.0) + 0.5).to(dt).double()
    bn = K._bn_mod(c, cuda, 10)
    rm, rv = bn.running_mean.double().cpu().clone(), bn.running_var.double().cpu().clone()
    xr = x.clone().requires_grad_(True)
    gw = bn.weight.detach().double().cpu().requires_grad_(True)
    gb = bn.bias.detach().double().cpu().requires_grad_(True)
    pw = torch.tensor([0.25], dtype=torch.float64, requires_grad=True)
    t = F.batch_norm(xr, rm, rv, gw, gb, True, 0.1, 1e-5)
    y_ref = F.relu(t) if act == 1 else (F.prelu(t, pw) if act == 2 else t)
    gy = rnd(t.shape, dt, 11)

    _, xg = sliced(nhwc(x), dt, cuda, fill=1000.0)
    st = ops.bn_stats(xg, bn, True)
    prelu = torch.tensor([0.25], dtype=torch.float32, device=cuda)
    ybuf, yg = blank(P, c, dt, cuda)
    ops.bn_apply(xg, st, bn, act=act, prelu=prelu, out=yg)
    torch.cuda.synchronize()
    close(nchw(yg, N, H, W), y_ref.detach(), dt)
    assert outside_unchanged(ybuf, c, dt)
    close(bn.running_mean, rm, torch.float32, scale=1.0)
    close(bn.running_var, rv, torch.float32, scale=1.0)

    if act == 1:
        m_gpu = (nchw(yg, N, H, W) > 0).cpu()
        td = t.detach()
        flips = m_gpu != (td > 0)
        if flips.any():
            assert td[flips].abs().max().item() <= TOL[dt] * td.abs().max().item()
        (t * m_gpu.double()).backward(gy)
    else:
        y_ref.backward(gy)

    _, gyg = sliced(nhwc(gy), dt, cuda, fill=1000.0)
    dxbuf, dxv = blank(P, c, dt, cuda)
    dx, dgam, dbet, dpr = ops.bn_bwd(xg, gyg, yg, st, bn, act=act, prelu=prelu, dx=dxv)
    torch.cuda.synchronize()
    assert dx.data_ptr() == dxv.data_ptr()
    close(nchw(dx, N, H, W), xr.grad, dt)
    assert outside_unchanged(dxbuf, c, dt)
    close(dgam, gw.grad, dt)
    close(dbet, gb.grad, dt)
    if act == 2:
        close(dpr, pw.grad, dt)
    if act == 1:
        # the ReLU mask recomputed from x (no read of the activation) is bit-identical
        dxbuf3, dxv3 = blank(P, c, dt, cuda)
        _, dgam3, dbet3, _ = ops.bn_bwd(xg, gyg, None, st, bn, act=1, dx=dxv3)
        torch.cuda.synchronize()
        assert torch.equal(dxbuf3, dxbuf) and torch.equal(dgam3, dgam) and torch.equal(dbet3, dbet)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("c", [64, 320])
def test_batchnorm_segments_multi_split_into_slice(cuda, dt, c):
    """The nseg = 2 downsample-residual apply of test_batchnorm_segments at 2294 rows a segment,
    written into a slice."""
    xa = (rnd((N, c, H, W), dt, 30) + 3.0).to(dt).double()
    xb = (rnd((N, c, H, W), dt, 31, scale=0.5) - 1.0).to(dt).double()
    da, db = rnd((N, c, H, W), dt, 32), rnd((N, c, H, W), dt, 33, scale=2.0)
    bn, bnd = K._bn_mod(c, cuda, 34), K._bn_mod(c, cuda, 35)
    rm, rv = bn.running_mean.double().cpu().clone(), bn.running_var.double().cpu().clone()
    cpu = lambda m: (m.weight.detach().double().cpu(), m.bias.detach().double().cpu())
    ya = F.batch_norm(xa, rm, rv, *cpu(bn), True, 0.1, 1e-5)
    yb = F.batch_norm(xb, rm, rv, *cpu(bn), True, 0.1, 1e-5)
    ra = F.batch_norm(da, None, None, *cpu(bnd), True, 0.1, 1e-5)
    rb = F.batch_norm(db, None, None, *cpu(bnd), True, 0.1, 1e-5)
    _, x = sliced(torch.cat([nhwc(xa), nhwc(xb)]), dt, cuda, fill=1000.0)
    _, d = sliced(torch.cat([nhwc(da), nhwc(db)]), dt, cuda, fill=1000.0)
    st = ops.bn_stats(x, bn, True, nseg=2)
    std = ops.bn_stats(d, bnd, True, nseg=2)
    ybuf, y = blank(2 * P, c, dt, cuda)
    ops.bn_apply(x, st, bn, act=1, xr=d, rstats=std, rbn=bnd, nseg=2, out=y)
    torch.cuda.synchronize()
    close(nchw(y[:P], N, H, W), F.relu(ya + ra), dt)
    close(nchw(y[P:], N, H, W), F.relu(yb + rb), dt)
    assert outside_unchanged(ybuf, c, dt)
    close(bn.running_mean, rm, torch.float32, scale=1.0)
    close(bn.running_var, rv, torch.float32, scale=1.0)
    assert bn._cn_nbt == 2


@pytest.mark.parametrize("dt", DTS)
def test_conv_dgrad_bn_and_bwd_apply_multi_split(cuda, dt):
    """cn_conv_dgrad_bn + cn_bn_bwd_apply at P = 2294, k = 1, cin = 320, with the checks of
    test_conv_dgrad_bn_epilogue_reduce."""
    K.test_conv_dgrad_bn_epilogue_reduce(cuda, dt, (N, 320, H, W, 64, 1, 0, 1))


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("nseg", [3, 4])
def test_bn_stats_three_and_four_segments(cuda, dt, nseg):
    """Per-segment mean / invstd against fp64 (test_batchnorm_stats_large's bounds) and the
    running statistics updated once per segment, in segment order (the segment means differ by
    whole units, so another order moves running_mean by ~0.1 against a bound of 2e-5)."""
    c = 64
    off, sc = [3.0, -1.0, 0.5, 7.0], [1.0, 0.5, 2.0, 1.5]
    segs = [(rnd((P, c), dt, 40 + i, scale=sc[i]) + off[i]).to(dt).double() for i in range(nseg)]
    bn = K._bn_mod(c, cuda, 44)
    rm, rv = bn.running_mean.double().cpu().clone(), bn.running_var.double().cpu().clone()
    _, x = sliced(torch.cat(segs), dt, cuda, fill=1000.0)
    mean, invstd = ops.bn_stats(x, bn, True, nseg=nseg)
    torch.cuda.synchronize()
    for i, s in enumerate(segs):
        m_ref, v_ref = s.mean(0), s.var(0, unbiased=False)
        is_ref = (v_ref + 1e-5).rsqrt()
        m, iv = ops.seg_of((mean, invstd), i, c)
        assert (m.double().cpu() - m_ref).abs().max().item() <= 1e-5 * (1 + m_ref.abs().max().item())
        assert ((iv.double().cpu() - is_ref) / is_ref).abs().max().item() <= 1e-4
        rm = 0.9 * rm + 0.1 * m_ref
        rv = 0.9 * rv + 0.1 * v_ref * P / (P - 1)
    close(bn.running_mean, rm, torch.float32, scale=1.0)
    close(bn.running_var, rv, torch.float32, scale=1.0)
    assert bn._cn_nbt == nseg


def test_bn_stats_five_segments_are_refused(cuda):
    x = torch.randn((5 * 16, 8), device=cuda)
    with pytest.raises(nv.NativeError):
        ops.bn_stats(x, K._bn_mod(8, cuda, 45), True, nseg=5)
    torch.cuda.synchronize()


def test_bn_apply_fp8_copy(cuda):
    """bn_apply(out8=, qstate=): the e4m3 copy of the output, written into a slice, with its amax.

    C = 320 in bf16 is 40 chunk columns x 6 rows = 240 working threads a block: the other 16 do no
    rows and must still take part in the block's amax reduction.  The kernel quantises the fp32
    activation (before its bf16 rounding), so the bytes are e4m3fn(clamp(t_ref / s)) of the fp64
    activation t_ref except where t_ref / s lies within the fp32 evaluation error (relative 1e-5)
    of the midpoint between two codes, where the neighbouring code is allowed."""
    dt, c = torch.bfloat16, 320
    x = (rnd((N, c, H, W), dt, 50, scale=2.0) + 0.5).to(dt).double()
    bn = K._bn_mod(c, cuda, 51)
    cpu = lambda m: (m.weight.detach().double().cpu(), m.bias.detach().double().cpu())
    t_ref = nhwc(F.relu(F.batch_norm(x, None, None, *cpu(bn), True, 0.1, 1e-5)))
    xg = nhwc(x).to(dt).to(cuda).contiguous()
    st = ops.bn_stats(xg, bn, True)
    y_plain = ops.bn_apply(xg, st, bn, act=1)
    # about 1 % of the outputs saturate
    s = torch.tensor(t_ref.flatten().kthvalue(int(0.99 * t_ref.numel())).values.item() / 448.0,
                     dtype=torch.float32)
    q = torch.stack([s, 1.0 / s, torch.tensor(0.0), torch.tensor(448.0)]).to(cuda)
    buf8 = torch.full((P, c + 32), 0x5A, dtype=torch.uint8, device=cuda)    # ld % 16 == 0
    y8 = buf8[:, 16:16 + c]
    y = ops.bn_apply(xg, st, bn, act=1, out8=y8, qstate=q)
    torch.cuda.synchronize()
    assert torch.equal(y, y_plain)
    assert bool((buf8[:, :16] == 0x5A).all()) and bool((buf8[:, 16 + c:] == 0x5A).all())

    v = (t_ref / s.double()).clamp(-448, 448)
    sat = (v == 448).double().mean().item()
    assert 0.005 <= sat <= 0.02, sat
    code_ref = v.to(torch.float8_e4m3fn).view(torch.uint8).to(torch.int32)
    code_got = y8.cpu().contiguous().to(torch.int32)
    bad = code_got != code_ref
    # outputs are >= 0 (ReLU): codes 0..0x7e ascend with the value, neighbours differ by one
    assert bool((code_got[bad] < 0x7f).all()) and bool(((code_got - code_ref)[bad].abs() == 1).all())
    dec = lambda cd: cd.to(torch.uint8).view(torch.float8_e4m3fn).double()
    mid = (dec(code_got[bad]) + dec(code_ref[bad])) / 2
    assert bool(((v[bad] - mid).abs() <= 1e-5 * mid).all())
    assert bad.double().mean().item() <= 1e-3

    amax = t_ref.abs().max().item()
    assert abs(q[2].item() - amax) <= 1e-6 * amax
    assert q[:2].cpu().tolist() == [s.item(), (1.0 / s).item()]     # untouched until the update
    got_amax = q[2].item()
    ops.fp8_update(q)
    torch.cuda.synchronize()
    assert abs(q[0].item() - got_amax / 448) <= 1e-6 * got_amax / 448
    assert abs(q[1].item() * q[0].item() - 1) <= 1e-6 and q[2].item() == 0.0
