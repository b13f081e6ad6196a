"""cn_conv_fwd_fp8_affine (include/cosnet_hip_infer_fp8.h): the static-scale fp8 conv with an
eval-mode BatchNorm, the residual add and the activation in its GEMM epilogue, writing the bf16
result and / or its e4m3 image under a frozen output state.

Exact part -- bitwise, no tolerance.  The problem is tests/test_cpu_fp8_fold.py's fold_problem
(which checks its guards without a GPU): tests/test_gpu_exact_gemm.py's fp8 forward operands
behind tests/test_gpu_conv_affine.py's affine.  Every partial sum is an exact fp32 value, so
  y  is ONE round-to-nearest-even rounding of t = act(fma(acc * sx * sw + bias, scale, shift) + res)
  y8 is e4m3(clamp(t * qinv, +-448)) of the fp32 t -- not of the stored bf16: at qinv = 1/8 most
     values are inexact in e4m3 and some are exact ties, where a conversion of the rounded bf16
     lands on another byte; at qinv = 1/2 a quarter to a half saturate.
Operands, the residual and both outputs are strided views in NaN / sentinel-filled buffers.
The three cases run the three A loaders: 1x1 stride 1 the dense one, Cin = 256 (stride 2) the
buffer-descriptor gather, Cin = 32 the per-thread-pointer gather (Cin % 128 != 0).

Random part: e4m3 bytes under the scales a calibrated tensor would have, against fp64 of the
folded math on the decoded operands, on bounds derived from the number formats.
"""
import pytest
import torch
import torch.nn.functional as F

from cosnet_amd import _native as nv
from cosnet_amd import ops

import test_gpu_exact_gemm as E
import test_gpu_conv_affine as A
import test_cpu_fp8_fold as G
from test_gpu_exact_gemm import FP8_SX, FP8_SW, bf, f32, operand, output, rows_of, same, untouched

pytestmark = pytest.mark.gpu

E4M3 = torch.float8_e4m3fn
U8 = torch.uint8
SENT8 = int(E.SENTINEL)
STATE_SENTINELS = (1234.5, -77.0)      # slots 2 / 3 of every state: never read, never written


def state(scale, dev):
    return torch.tensor([scale, 1.0 / scale, STATE_SENTINELS[0], STATE_SENTINELS[1]], dtype=f32, device=dev)


def output8(p, c, dev):
    """(buffer, view [p, c]) of bytes: SENT8 outside the view, the e4m3 NaN inside."""
    return output(p, c, U8, dev, old=torch.full((p, c), E.FP8_NAN, dtype=U8))


def untouched8(buf, p, c, what):
    b = buf.detach().cpu()
    inside = torch.zeros(b.shape, dtype=torch.bool)
    inside[:p, E.ROWPAD:E.ROWPAD + c] = True
    assert bool((b[~inside] == SENT8).all()), "%s: written outside the view" % what


def same8(got, want, what):
    got = got.detach().cpu()
    assert got.dtype == U8 and want.dtype == U8 and got.shape == want.shape, (what, got.shape, want.shape)
    ne = got != want
    if ne.any():
        raise AssertionError("%s: %d of %d bytes differ, first at %s: got %s, want %s" % (
            what, int(ne.sum()), ne.numel(), ne.nonzero()[:4].tolist(), got[ne][:4].tolist(), want[ne][:4].tolist()))


class Operands:
    """The device operands of one case (shared by its launches; never written)."""

    def __init__(self, case, dev):
        n, cin, h, w, cout, k, s, p, d = case
        pr = E.fp8_fwd_problem(case)
        self.case, self.pr, self.dev = case, pr, dev
        self.m = n * pr.oh * pr.ow
        self.x8 = operand(E.fp8_bytes(rows_of(pr.xb), E4M3), U8, dev)
        self.w8 = E.fp8_bytes(pr.wb.permute(0, 2, 3, 1).reshape(cout, k * k * cin), E4M3).to(dev).contiguous()
        self.xs, self.ws = state(FP8_SX, dev), state(FP8_SW, dev)
        self.bias = pr.bias.to(f32).to(dev)
        self.scale = A.affine_scale(cout, G.SEED_SCALE).to(f32).to(dev)
        self.shift = E.offset_bias(cout, G.SEED_SHIFT).to(f32).to(dev)
        self.res = operand(rows_of(E.old_c((n, cout, pr.oh, pr.ow), G.SEED_RES)), bf, dev)
        self.prelu = torch.tensor([A.PRELU_SLOPE], dtype=f32, device=dev)
        self.states_before = [t.clone() for t in (self.xs, self.ws)]

    def launch(self, act, with_res, with_bias, qinv, want_y=True, want_y8=True):
        """-> (ybuf, yv, y8buf, y8v, out_state); an absent output keeps its sentinel buffer."""
        n, cin, h, w, cout, k, s, p, d = self.case
        ybuf, yv = output(self.m, cout, bf, self.dev)
        y8buf, y8v = output8(self.m, cout, self.dev)
        qs = state(1.0 / qinv, self.dev)
        ops.conv_fwd_fp8_affine(self.x8, n, h, w, self.w8, cout, k, s, p, d, self.xs, self.ws, self.scale,
                                self.shift, act=act, prelu=self.prelu if act == 2 else None,
                                res=self.res if with_res else None, bias=self.bias if with_bias else None,
                                out=yv if want_y else None, out8=y8v if want_y8 else None,
                                out_state=qs if want_y8 else None, want_y=want_y)
        torch.cuda.synchronize()
        return ybuf, yv, y8buf, y8v, qs

    def states_intact(self, qs, qinv):
        for t, ref in zip((self.xs, self.ws), self.states_before):
            assert torch.equal(t.view(torch.int32), ref.view(torch.int32)), "an operand state was written"
        assert torch.equal(qs.view(torch.int32), state(1.0 / qinv, self.dev).view(torch.int32)), \
            "the output state was written"


def check_exact(op, act, with_res, with_bias, qinv, what):
    n, cin, h, w, cout, k, s, p, d = op.case
    _, _, _, _, t, bound = G.fold_problem(op.case, act, with_res, with_bias)
    assert bound < 2 ** 24
    ybuf, yv, y8buf, y8v, qs = op.launch(act, with_res, with_bias, qinv)
    label = "%s %s act %d res %d bias %d qinv %g" % (what, op.case, act, with_res, with_bias, qinv)
    same(yv, rows_of(E.rne_bf16(t)), label + " y")
    same8(y8v, rows_of(G.e4m3_of(t, qinv).view(U8)), label + " y8")
    untouched(ybuf, op.m, cout, label + " y")
    untouched8(y8buf, op.m, cout, label + " y8")
    op.states_intact(qs, qinv)
    return yv, y8v


# ---- the contract, every loader ---------------------------------------------------------------------
@pytest.mark.parametrize("case", E.FP8_FWD_CASES)
def test_conv_fwd_fp8_affine_exact(cuda, case):
    """act 0 / 1 / 2 x residual / none x bias / none x qinv 1/2, 1/8: y and y8 bitwise, nothing
    outside the views written, no state written (slots 2 / 3 carry sentinels)."""
    op = Operands(case, cuda)
    for act in A.ACTS:
        for with_res in (False, True):
            for with_bias in (False, True):
                for qinv in G.QINVS:
                    check_exact(op, act, with_res, with_bias, qinv, "exact")


@pytest.mark.parametrize("case", [E.FP8_FWD_CASES[0], E.FP8_FWD_CASES[1]])
def test_output_combinations_are_bitwise_the_same(cuda, case):
    """(y, y8) in one launch = the y-only launch and the y8-only launch; the absent buffer keeps
    every sentinel (NaN inside its view included)."""
    op = Operands(case, cuda)
    cout = case[4]
    for act, with_res, qinv in ((1, True, 0.125), (2, False, 0.5)):
        _, yv, _, y8v, _ = op.launch(act, with_res, True, qinv)
        ybuf1, yv1, y8buf1, _, _ = op.launch(act, with_res, True, qinv, want_y8=False)
        ybuf2, _, y8buf2, y8v2, qs = op.launch(act, with_res, True, qinv, want_y=False)
        assert torch.equal(yv.view(torch.int16), yv1.view(torch.int16))
        assert torch.equal(y8v, y8v2)
        fresh8, fresh = output8(op.m, cout, cuda)[0], output(op.m, cout, bf, cuda)[0]
        assert torch.equal(y8buf1, fresh8), "y-only launch wrote the absent e4m3 buffer"
        assert torch.equal(ybuf2.view(torch.int16), fresh.view(torch.int16)), "y8-only launch wrote the absent bf16 buffer"
        untouched(ybuf1, op.m, cout, "y only")
        untouched8(y8buf2, op.m, cout, "y8 only")
        op.states_intact(qs, qinv)


# ---- tiles ----------------------------------------------------------------------------------------------
@pytest.fixture
def force_cfg():
    lib = nv.load()
    yield lib.cn_gemm_force_config
    lib.cn_gemm_force_config(-1)


@pytest.mark.parametrize("cfg", (11, 12, 13))
def test_every_fp8_tile(cuda, force_cfg, cfg):
    """The three tiles launch_f8 instantiates, on the 1x1 (dense loader) and the 3x3 (per-thread
    pointer gather) case."""
    force_cfg(cfg)
    for case in (E.FP8_FWD_CASES[0], E.FP8_FWD_CASES[1]):
        op = Operands(case, cuda)
        check_exact(op, 1, True, True, 0.125, "tile %d" % cfg)
        check_exact(op, 2, False, True, 0.5, "tile %d" % cfg)


@pytest.mark.parametrize("cfg", (0, 20))
def test_refuses_a_forced_tile_without_the_epilogue(cuda, force_cfg, cfg):
    op = Operands(E.FP8_FWD_CASES[0], cuda)
    force_cfg(cfg)
    with pytest.raises(nv.NativeError, match="unsupported"):
        op.launch(1, True, True, 0.5)


# ---- random data against fp64 of the folded math ---------------------------------------------------
def test_random_e4m3_against_fp64(cuda):
    """Random e4m3 bytes (every finite code) under calibrated scales, a layer-3-like 3x3 conv
    (256 -> 256, dilation 2) at 13 x 11, K = 2304, with a residual and the ReLU.
      y   within 1.2e-2 of the output scale (the project's bf16 kernel bound);
      y8  |dec(y8) - u| <= 2^-4 |u| + 2^-10 + 1e-4 max|u|,  u = clamp(t64 * qinv, +-448):
          e4m3's half-ulp for normals (3 mantissa bits: ulp <= 2^-3 |u|), its half-ulp for
          subnormals (ulp 2^-9), and an allowance for fp32 accumulation over K <= 2304 (each of
          the K additions rounds at 2^-24 relative to partial sums that random signs keep at the
          scale of the result: K * 2^-24 = 1.4e-4 worst case, 1e-4 taken of the largest |u|)."""
    n, cin, h, w, cout, k, s, p, d = 2, 256, 13, 11, 256, 3, 1, 2, 2
    g = torch.Generator().manual_seed(8013)

    def codes(shape):
        b = torch.randint(0, 256, shape, generator=g, dtype=torch.int64)
        b = torch.where((b & 0x7F) == 0x7F, b & 0x80, b)       # the two NaN codes -> +-0
        return b.to(U8)

    xb, wb = codes((n * h * w, cin)), codes((cout, k * k * cin))
    # the scales of calibrated tensors: amax / 448 for an activation of amax 6 and a weight of 0.2
    sx, sw = 6.0 / 448.0, 0.2 / 448.0
    x64 = xb.view(E4M3).double().view(n, h, w, cin).permute(0, 3, 1, 2) * float(torch.tensor(sx, dtype=f32))
    w64 = wb.view(E4M3).double().view(cout, k, k, cin).permute(0, 3, 1, 2) * float(torch.tensor(sw, dtype=f32))
    bn_scale = (torch.rand((cout,), generator=g) + 0.5).to(f32)
    bn_shift = (torch.randn((cout,), generator=g) * 0.3).to(f32)
    res = (torch.randn((n * h * w, cout), generator=g) * 2.0).to(bf)
    t = F.conv2d(x64, w64, None, s, p, d) * bn_scale.double().view(1, -1, 1, 1) + bn_shift.double().view(1, -1, 1, 1)
    t = torch.relu(rows_of(t) + res.double())
    amax_out = t.abs().max().item()
    qs = state(0.5 * amax_out / 448.0, cuda)                  # half the range: the top values saturate
    qinv = float(qs[1].item())
    x8 = operand(xb, U8, cuda)
    y, y8, _, _ = ops.conv_fwd_fp8_affine(x8, n, h, w, wb.to(cuda), cout, k, s, p, d, state(sx, cuda), state(sw, cuda),
                                          bn_scale.to(cuda), bn_shift.to(cuda), act=1, res=operand(res, bf, cuda),
                                          out_state=qs)
    torch.cuda.synchronize()
    err = (y.double().cpu() - t).abs().max().item() / amax_out
    u = (t * qinv).clamp(-448.0, 448.0)
    dec = y8.cpu().view(E4M3).double()
    bound = u.abs() * 2.0 ** -4 + 2.0 ** -10 + 1e-4 * u.abs().max()
    over = ((dec - u).abs() - bound).max().item()
    print("random e4m3: y %.3e of the output scale (bound 1.2e-2); y8 worst (|dec - u| - bound) %.3e, "
          "%.1f %% saturated" % (err, over, 100 * (u.abs() == 448.0).double().mean().item()))
    assert torch.isfinite(dec).all() and amax_out > 0
    assert err <= 1.2e-2, err
    assert over <= 0.0, over


# ---- error codes ---------------------------------------------------------------------------------------
def test_error_codes(cuda):
    case = E.FP8_FWD_CASES[0]
    n, cin, h, w, cout, k, s, p, d = case
    op = Operands(case, cuda)
    m = op.m
    _, yv = output(m, cout, bf, cuda)
    _, y8v = output8(m, cout, cuda)
    qs = state(2.0, cuda)
    tab = torch.ones((cout + 4,), dtype=f32, device=cuda)
    ok, off = tab[:cout], tab[1:cout + 1]                     # off: 4 bytes past a 16-byte boundary
    S = nv.stream()

    def raw(x8=op.x8, ldx=None, w8=op.w8, scale=ok, shift=ok, act=1, prelu=None, y=yv, y8=y8v, ldy8=None,
            out_state=qs, cout_=cout, oh=op.pr.oh):
        nv.call("cn_conv_fwd_fp8_affine", x8.data_ptr(), ops.ld(op.x8) if ldx is None else ldx, n, h, w, cin,
                w8.data_ptr(), cout_, k, k, s, p, d, None, op.xs.data_ptr(), op.ws.data_ptr(), nv.ptr(scale),
                nv.ptr(shift), None, 0, act, nv.ptr(prelu), nv.ptr(y), ops.ld(yv), nv.ptr(y8),
                ops.ld(y8v) if ldy8 is None else ldy8, nv.ptr(out_state), oh, op.pr.ow, S)

    # cn_conv_fwd_fp8's operand codes
    with pytest.raises(nv.NativeError, match="alignment"):
        raw(ldx=ops.ld(op.x8) + 8)                            # rows of whole 16-byte chunks
    with pytest.raises(nv.NativeError, match="alignment"):
        raw(x8=op.x8[:, 8:])                                  # a base 8 bytes past a 16-byte boundary
    with pytest.raises(nv.NativeError, match="shape"):
        raw(oh=op.pr.oh + 1)
    # the fold table
    with pytest.raises(nv.NativeError, match="shape"):
        raw(scale=None)
    with pytest.raises(nv.NativeError, match="shape"):
        raw(shift=None)
    with pytest.raises(nv.NativeError, match="alignment"):
        raw(scale=off)
    with pytest.raises(nv.NativeError, match="alignment"):
        raw(shift=off)
    # the outputs
    with pytest.raises(nv.NativeError, match="shape"):
        raw(y=None, y8=None)
    with pytest.raises(nv.NativeError, match="shape"):
        raw(out_state=None)
    with pytest.raises(nv.NativeError, match="alignment"):
        raw(ldy8=ops.ld(y8v) + 4)
    with pytest.raises(nv.NativeError, match="alignment"):
        raw(y8=y8v[:, 4:])                                    # base 4 bytes past an 8-byte boundary
    with pytest.raises(nv.NativeError, match="alignment"):
        raw(cout_=cout - 4)                                   # Cout % 8
    # the activation
    with pytest.raises(nv.NativeError, match="unsupported"):
        raw(act=2)                                            # PReLU without its slope
    with pytest.raises(nv.NativeError, match="unsupported"):
        raw(act=3)
    with pytest.raises(nv.NativeError, match="unsupported"):
        raw(act=-1)
    # the wrapper's own refusals
    with pytest.raises(ValueError):
        ops.conv_fwd_fp8_affine(op.x8, n, h, w, op.w8, cout, k, s, p, d, op.xs, op.ws, ok, ok, want_y=False)
    with pytest.raises(ValueError):
        ops.conv_fwd_fp8_affine(op.x8, n, h, w, op.w8, cout, k, s, p, d, op.xs, op.ws, ok, ok, out8=y8v)
    with pytest.raises(ValueError):
        ops.conv_fwd_fp8_affine(op.x8, n, h, w, op.w8, cout, k, s, p, d, op.xs, op.ws, ok[:cout - 8], ok)
    raw()                                                     # the same call with valid arguments runs
    raw(y8=None, out_state=None)
    raw(y=None)
    torch.cuda.synchronize()
