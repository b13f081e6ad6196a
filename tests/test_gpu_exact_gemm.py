"""Exact-arithmetic parity of every implicit-GEMM path (gemm.hip, gemm_ws.hip, conv.hip and the fp8
conv / dgrad / wgrad paths) -- bitwise, no tolerance.

Integer-valued operands make every product and every partial sum an integer below 2^24, so the
MFMA results, the fp32 accumulators, the split-K slabs and the atomics are exact and independent
of the summation order.  The contract of include/cosnet_hip.h then reads bitwise: fp32 outputs
equal the exact result, bf16 outputs equal ONE round-to-nearest-even rounding (torch's CPU cast)
of the fp32 value alpha * acc (+ bias) (+ old C).  Scales and alpha are powers of two, bias and
old C integers.

Two regimes (the generators below; tests/test_cpu_exact_inputs.py checks them without a GPU):
  rounding       x in [-4, 4], w in [-3, 3], bias = +-384 (alternating) + [-8, 8], old C an even
                 integer in +-[256, 510]: the outputs sit where bf16's spacing is >= 2, so odd
                 results are exact ties; every comparison with such an offset must hold >= 10 %
                 ties (launches without bias or old C have no offset to put them there: their
                 outputs are compared all the same, against the one RNE rounding)
  representable  dy in {-1, 0, 1}, the rest in [-2, 2], |result| <= 256 asserted: every output is
                 bf16-exact, for the fused epilogues that consume the output around its rounding

Every operand and output lives in a wider buffer (row stride = channels + 16, the view starts at
column 16, ROWS_PAST rows after the last): the padding of the inputs is NaN (any read that reaches
the MACs turns the output NaN), the outputs are NaN inside the view before a store (the old C
before an accumulation) and SENTINEL everywhere outside, which must come back bitwise.
"""
import decimal
import functools
import math
from fractions import Fraction
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from cosnet_amd import _native as nv
from cosnet_amd import ops

import test_gpu_kernels as K
from test_gpu_gemm_cfgs import CFGS

pytestmark = pytest.mark.gpu

bf = torch.bfloat16
f32 = torch.float32
ROWPAD = 16       # row stride = channels + ROWPAD; the view starts at column ROWPAD
ROWS_PAST = 3     # rows after the last row of a view
SENTINEL = 7.0
MIN_TIES = 0.10
ROUND, REPR = "rounding", "representable"

# n, cin, h, w, cout, k, stride, pad, dil
CONV_CASES = [
    (2, 64, 13, 11, 128, 1, 1, 0, 1),
    (2, 64, 13, 11, 64, 3, 1, 1, 1),
    (2, 32, 15, 9, 64, 3, 1, 2, 2),
    (2, 256, 7, 9, 128, 1, 2, 0, 1),     # stride-2 row map: forward, and dgrad with 1x1 / pad 0
    (2, 8, 29, 31, 64, 7, 2, 3, 1),      # stem: forward and wgrad only
    (1, 64, 9, 9, 512, 3, 1, 6, 6),
    (1, 320, 5, 6, 256, 3, 1, 1, 1),
    (3, 16, 4, 4, 8, 3, 1, 1, 1),
    (1, 8, 5, 141, 16, 3, 2, 1, 1),
    (4, 2048, 1, 1, 512, 1, 1, 0, 1),    # the ASPP pooling branch, M = 4
]
WGRAD_SPLIT_CASE = (4, 64, 30, 30, 128, 1, 1, 0, 1)
SPLIT_K_CASE = (2, 2048, 9, 9, 256, 3, 1, 1, 1)
CFG_CASES = [(2, 96, 21, 23, 320, 1, 1, 0, 1), (2, 128, 19, 21, 192, 3, 1, 2, 2)]
WS_CASE = (3, 128, 17, 19, 328, 1, 1, 0, 1)
WS_CASE_T = (3, 328, 17, 19, 128, 1, 1, 0, 1)   # its transpose: the dgrad's K = 128 is eligible
# n per segment, cin, h, w, cout, k, stride, pad, dil, nseg
BN_CASES = [(2, 64, 13, 11, 64, 3, 1, 2, 2, 2), (1, 256, 30, 20, 256, 1, 1, 0, 1, 2)]
# n, cin, h, w, cout, k, pad, dil (test_conv_dgrad_bn_epilogue_reduce's layout)
DGRAD_BN_CASES = [(2, 64, 13, 11, 64, 3, 2, 2), (1, 128, 9, 9, 256, 1, 0, 1)]
FP8_FWD_CASES = [(2, 64, 13, 11, 128, 1, 1, 0, 1), (2, 32, 15, 9, 64, 3, 1, 2, 2),
                 (2, 256, 7, 9, 128, 1, 2, 0, 1)]
# n, cout, h, w, cin, k, pad, dil (test_conv_dgrad_fp8's layout)
FP8_DGRAD_CASES = [(2, 256, 13, 11, 128, 3, 1, 1), (2, 128, 15, 9, 64, 1, 0, 1)]
FP8_WGRAD_CASES = [(2, 256, 13, 11, 128, 3, 1, 2, 2), (2, 128, 15, 9, 64, 1, 1, 0, 1),
                   (2, 96, 17, 19, 48, 3, 2, 1, 1)]
FP8_SCALES = (0.5, 0.25, 0.125)
GEMM_BMNK = (3, 77, 136, 200)
GEMM_LAYOUTS = [(0, 0), (0, 2), (2, 2)]
GEMM_ATOMIC_MNK = (256, 192, 4000)
GEMM_KB_LIM = 169


# ---- generators and guards (CPU, fp64) ------------------------------------------------------
def ints(shape, lo, hi, seed):
    """Uniform integers in [lo, hi] as fp64."""
    g = torch.Generator().manual_seed(seed)
    return torch.randint(lo, hi + 1, tuple(shape), generator=g).double()


def offset_bias(c, seed):
    """+-384 alternating by channel + an integer in [-8, 8]."""
    sign = (1 - 2 * (torch.arange(c) % 2)).double()
    return sign * 384 + ints((c,), -8, 8, seed)


def old_c(shape, seed):
    """An even integer in +-[256, 510] (bf16-exact)."""
    return 2 * ints(shape, 128, 255, seed) * (2 * ints(shape, 0, 1, seed + 7919) - 1)


def rne_bf16(ref):
    """fp64 (fp32-exact) -> bf16 by one round-to-nearest-even (torch's CPU cast)."""
    return ref.to(f32).to(bf)


def is_tie(ref):
    """ref (fp32-exact) lies exactly halfway between two bf16 neighbours."""
    return (ref.to(f32).contiguous().view(torch.int32) & 0xFFFF) == 0x8000


def tie_share(ref):
    return is_tie(ref).double().mean().item()


class Out:
    """One compared output: its exact fp64 value and the conditions it must meet."""

    def __init__(self, ref, bound, ties=False, repr_=False, step=1.0):
        self.ref, self.bound, self.ties, self.repr, self.step = ref, float(bound), ties, repr_, step

    def expect(self, dt):
        return self.ref.to(f32) if dt == f32 else rne_bf16(self.ref)


def amax(t):
    return 0.0 if t is None else t.abs().max().item()


def bound_of(k, a, b, bias=None, old=None):
    """The sufficient exactness bound K * max|a| * max|b| + max|bias| + max|old|."""
    return k * amax(a) * amax(b) + amax(bias) + amax(old)


def verify(out):
    """The guard conditions of one output (every GPU test calls this before launching, and the
    CPU self-check for every case): exact in fp32, integral, tied / representable as declared.
    Returns the tie share."""
    assert out.bound < 2 ** 24, out.bound
    q = out.ref / out.step
    assert torch.equal(q, q.round()), "reference is not a multiple of %g" % out.step
    assert torch.equal(out.ref.to(f32).double(), out.ref)
    share = tie_share(out.ref)
    if out.ties:
        t = is_tie(out.ref)
        assert not torch.equal(out.ref.to(f32)[t], rne_bf16(out.ref).to(f32)[t])
        assert share >= MIN_TIES, share
    if out.repr:
        assert out.ref.abs().max().item() <= 256
        assert torch.equal(rne_bf16(out.ref).double(), out.ref)
    return share


def conv_problem(case, regime=ROUND, seed=0, bwd=True):
    return _conv_problem(case, regime, seed, bwd)


@functools.lru_cache(maxsize=None)
def _conv_problem(case, regime, seed, bwd):
    """Operands and exact results of one conv (never written; shared by the tests of a shape):
    forward with bias, input gradient (plain and onto an old C), weight gradient."""
    n, cin, h, w, cout, k, s, p, d = case
    sd = 100 * seed + 11
    lo = 4 if regime == ROUND else 2
    x = ints((n, cin, h, w), -lo, lo, sd + 1)
    wt = ints((cout, cin, k, k), -3 if regime == ROUND else -2, 3 if regime == ROUND else 2, sd + 2)
    bias = offset_bias(cout, sd + 3) if regime == ROUND else ints((cout,), -2, 2, sd + 3)
    xr, wr = x.clone().requires_grad_(bwd), wt.clone().requires_grad_(bwd)
    y0 = F.conv2d(xr, wr, None, s, p, d)
    oh, ow = y0.shape[2:]
    pr = SimpleNamespace(case=case, x=x, w=wt, bias=bias, oh=oh, ow=ow, outs={})
    rep = regime == REPR
    pr.outs["fwd"] = Out(y0.detach() + bias.view(1, -1, 1, 1), bound_of(k * k * cin, x, wt, bias),
                         ties=not rep, repr_=rep)
    if bwd:
        gy = ints(y0.shape, -4, 4, sd + 4) if regime == ROUND else ints(y0.shape, -1, 1, sd + 4)
        y0.backward(gy)
        pr.gy = gy
        pr.outs["dgrad"] = Out(xr.grad, bound_of(k * k * cout, gy, wt), repr_=rep)
        if not rep:
            pr.old = old_c(x.shape, sd + 5)
            pr.outs["dgrad_acc"] = Out(xr.grad + pr.old, bound_of(k * k * cout, gy, wt, old=pr.old), ties=True)
        pr.outs["wgrad"] = Out(wr.grad, bound_of(n * oh * ow, x, gy))
    return pr


def has_dgrad(case):
    n, cin, h, w, cout, k, s, p, d = case
    return s == 1 or (k == 1 and p == 0)


@functools.lru_cache(maxsize=None)
def gemm_problem(b, m, n, k, seed=0, kb_lim=None):
    """C[b] = A[b] . B[b]^T on rounding-regime integers, with a bias row and an old C."""
    a = ints((b, m, k), -4, 4, 900 + seed)
    bm = ints((b, n, k), -3, 3, 901 + seed)
    kk = k if kb_lim is None else kb_lim
    acc = torch.einsum("bmk,bnk->bmn", a[:, :, :kk], bm[:, :, :kk])
    bias = offset_bias(n, 902 + seed)
    old = old_c((b, m, n), 903 + seed)
    pr = SimpleNamespace(a=a, b=bm, acc=acc, bias=bias, old=old, outs={})
    for alpha in (1.0, 0.5):
        pr.outs["plain", alpha] = Out(alpha * acc, bound_of(k, a, bm), step=alpha)
        pr.outs["bias", alpha] = Out(alpha * acc + bias, bound_of(k, a, bm, bias), ties=True, step=alpha)
    pr.outs["acc", 1.0] = Out(acc + old, bound_of(k, a, bm, old=old), ties=True)
    return pr


BN_MEAN, BN_INVSTD, BN_BETA = 2.0, 0.5, 0.25


def bn_gamma(c):
    """+2 / -1 alternating by channel (a negative gamma flips the ReLU mask)."""
    return torch.where(torch.arange(c) % 2 == 0, 2.0, -1.0).double()


@functools.lru_cache(maxsize=None)
def dgrad_bn_problem(case):
    """Stride-1 dgrad fused with the BN + ReLU backward sums: dx = dgrad(dy, w) as written,
    dbeta = sum dx * mask, dgamma = sum dx * mask * xhat with xhat = (x - 2) / 2 (multiples of 0.5)
    and mask = gamma * xhat + 0.25 > 0 (a multiple of 0.25, never 0)."""
    n, cin, h, w, cout, k, p, d = case
    x = ints((n, cin, h, w), -2, 6, 401)
    wt = ints((cout, cin, k, k), -2, 2, 402)
    gy = ints((n, cout, h, w), -1, 1, 403)
    xr = torch.zeros_like(x).requires_grad_(True)
    F.conv2d(xr, wt, None, 1, p, d).backward(gy)
    dx = xr.grad
    gam = bn_gamma(cin)
    xhat = (x - BN_MEAN) * BN_INVSTD
    act = gam.view(1, -1, 1, 1) * xhat + BN_BETA
    assert (act != 0).all()
    dz = dx * (act > 0)
    pr = SimpleNamespace(x=x, w=wt, gy=gy, gamma=gam, outs={})
    pr.outs["dx"] = Out(dx, bound_of(k * k * cout, gy, wt), repr_=True)
    pr.outs["dbeta"] = Out(dz.sum(dim=(0, 2, 3)), n * h * w * amax(dx))
    # the kernel sums dz * (x - mean) and scales by invstd once per column
    pr.outs["dgamma"] = Out((dz * xhat).sum(dim=(0, 2, 3)), n * h * w * amax(dx) * amax(x - BN_MEAN), step=0.5)
    return pr


# fp8: the bytes are integers (e4m3 x = 2 * [-4, 4], w = 4 * [-3, 3]; e5m2 dy = [-4, 4]) and the
# states' dequantisation scales 0.5 (x, dy) and 0.25 (w), so x and w DECODE to the rounding regime's
# integers and dy to multiples of 0.5.  Those bytes leave e4m3's low mantissa bits clear, so the
# bias-free forward and the weight gradients (no offset, no ties to place) also run on e4m3
# integers in [-15, 15], every mantissa bit in use
FP8_SX, FP8_SW, FP8_SDY = 0.5, 0.25, 0.5


def fp8_bytes(vals, fmt):
    """Integer-valued fp64 -> fp8 bytes (uint8); the decode must round-trip."""
    q = vals.to(torch.float32).to(fmt)
    assert torch.equal(q.double(), vals), "not representable in %s" % fmt
    return q.view(torch.uint8)


@functools.lru_cache(maxsize=None)
def fp8_fwd_problem(case):
    n, cin, h, w, cout, k, s, p, d = case
    xb = 2 * ints((n, cin, h, w), -4, 4, 501)
    wb = 4 * ints((cout, cin, k, k), -3, 3, 502)
    bias = offset_bias(cout, 503)
    y = F.conv2d(xb * FP8_SX, wb * FP8_SW, bias, s, p, d)
    pr = SimpleNamespace(xb=xb, wb=wb, bias=bias, oh=y.shape[2], ow=y.shape[3], outs={})
    # the accumulator holds the byte products: bound on them; the scaled sum + bias is then exact
    pr.outs["fwd"] = Out(y, bound_of(k * k * cin, xb, wb, bias), ties=True)
    pr.xf = ints((n, cin, h, w), -15, 15, 504)
    pr.wf = ints((cout, cin, k, k), -15, 15, 505)
    pr.outs["fwd_full"] = Out(F.conv2d(pr.xf * FP8_SX, pr.wf * FP8_SW, None, s, p, d),
                              bound_of(k * k * cin, pr.xf, pr.wf), step=FP8_SX * FP8_SW)
    return pr


@functools.lru_cache(maxsize=None)
def fp8_dgrad_problem(case):
    n, cout, h, w, cin, k, p, d = case
    gb = ints((n, cout, h, w), -4, 4, 511)
    wb = 4 * ints((cout, cin, k, k), -3, 3, 512)
    dx = F.conv_transpose2d(gb * FP8_SDY, wb * FP8_SW, None, 1, p, 0, 1, d)
    old = old_c(dx.shape, 513)
    pr = SimpleNamespace(gb=gb, wb=wb, old=old, outs={})
    pr.outs["dgrad"] = Out(dx, bound_of(k * k * cout, gb, wb), step=0.5)
    pr.outs["dgrad_acc"] = Out(dx + old, bound_of(k * k * cout, gb, wb, old=old), ties=True, step=0.5)
    return pr


@functools.lru_cache(maxsize=None)
def fp8_wgrad_problem(case, g):
    n, cin, h, w, cout, k, s, p, d = case
    xb = ints((n, cin, h, w), -15, 15, 521 + g)
    sc = FP8_SCALES[g]
    wr = torch.zeros((cout, cin, k, k), dtype=torch.float64, requires_grad=True)
    y0 = F.conv2d(xb * sc, wr, None, s, p, d)
    gb = ints(y0.shape, -4, 4, 531 + g)
    y0.backward(gb * sc)
    pr = SimpleNamespace(xb=xb, gb=gb, scale=sc, oh=y0.shape[2], ow=y0.shape[3], outs={})
    pr.outs["wgrad"] = Out(wr.grad, bound_of(n * y0.shape[2] * y0.shape[3], xb, gb), step=sc * sc)
    return pr


def all_problems():
    """(label, Out) of every comparison of this file, for the CPU self-check."""
    def named(label, outs):
        items = outs.items() if isinstance(outs, dict) else enumerate(outs)
        return [("%s %s" % (label, key), o) for key, o in items]
    res = []
    for case in CONV_CASES:
        pr = conv_problem(case)
        outs = {k: o for k, o in pr.outs.items() if has_dgrad(case) or not k.startswith("dgrad")}
        res += named("conv %s" % (case,), outs)
        for g in (1, 2):
            res += named("wgrad-grouped g%d %s" % (g, case), {"wgrad": conv_problem(case, ROUND, g).outs["wgrad"]})
    for g in (0, 1):
        res += named("wgrad-split g%d" % g, {"wgrad": conv_problem(WGRAD_SPLIT_CASE, ROUND, g).outs["wgrad"]})
    res += named("split-k %s" % (SPLIT_K_CASE,), conv_problem(SPLIT_K_CASE, ROUND, 0, False).outs)
    for case in CFG_CASES + [WS_CASE, WS_CASE_T]:
        res += named("conv %s" % (case,), conv_problem(case).outs)
    res += named("gemm", gemm_problem(*GEMM_BMNK).outs)
    res += named("gemm kb_lim", gemm_problem(*GEMM_BMNK, seed=1, kb_lim=GEMM_KB_LIM).outs)
    res += named("gemm split", gemm_problem(1, *GEMM_ATOMIC_MNK, seed=2).outs)
    for case in BN_CASES:
        n, cin, h, w, cout, k, s, p, d, nseg = case
        res += named("fwd-bn %s" % (case,), {"fwd": conv_problem((nseg * n,) + case[1:9], REPR, 3, False).outs["fwd"]})
    for case in DGRAD_BN_CASES:
        res += named("dgrad-bn %s" % (case,), dgrad_bn_problem(case).outs)
    for case in FP8_FWD_CASES:
        res += named("fp8 fwd %s" % (case,), fp8_fwd_problem(case).outs)
    for case in FP8_DGRAD_CASES:
        res += named("fp8 dgrad %s" % (case,), fp8_dgrad_problem(case).outs)
    for case in FP8_WGRAD_CASES:
        for g in range(3):
            res += named("fp8 wgrad g%d %s" % (g, case), fp8_wgrad_problem(case, g).outs)
    return res


# ---- strided views and sentinels ------------------------------------------------------------
FP8_NAN = 0x7F    # NaN in e4m3fn and in e5m2


def operand(rows, dt, dev):
    """rows [.., P, C] (fp64, or uint8 fp8 bytes) -> its view in a NaN-filled [.., P + ROWS_PAST,
    C + ROWPAD] device buffer."""
    p, c = rows.shape[-2:]
    fill = FP8_NAN if dt == torch.uint8 else float("nan")
    buf = torch.full(tuple(rows.shape[:-2]) + (p + ROWS_PAST, c + ROWPAD), fill, dtype=dt)
    buf[..., :p, ROWPAD:] = rows.to(dt)
    buf = buf.to(dev)
    return buf[..., :p, ROWPAD:]


def output(p, c, dt, dev, old=None, lead=()):
    """(buffer, view [.., p, c]): SENTINEL outside the view, NaN (a store) or the old C inside."""
    buf = torch.full(tuple(lead) + (p + ROWS_PAST, c + ROWPAD), SENTINEL, dtype=dt)
    buf[..., :p, ROWPAD:] = float("nan") if old is None else old.to(dt)
    buf = buf.to(dev)
    return buf, buf[..., :p, ROWPAD:]


def flat_output(numel, dev, tail=64):
    """fp32 [numel] NaN + `tail` sentinels behind it (the dense weight gradients)."""
    buf = torch.full((numel + tail,), SENTINEL, dtype=f32)
    buf[:numel] = float("nan")
    buf = buf.to(dev)
    return buf, buf[:numel]


def bits(t):
    t = t.contiguous()
    return t.view(torch.int16) if t.dtype == bf else t.view(torch.int32)


def same(got, want, what):
    """got (device) is bitwise want (CPU, same dtype)."""
    got = got.detach().cpu()
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, got.shape, want.shape)
    ne = bits(got) != bits(want)
    if ne.any():
        idx = ne.nonzero()[:4].tolist()
        raise AssertionError("%s: %d of %d elements differ, first at %s: got %s, want %s" % (
            what, int(ne.sum()), ne.numel(), idx, got[ne][:4].tolist(), want[ne][:4].tolist()))


def untouched(buf, p, c, what):
    """Everything outside the [.., :p, ROWPAD:ROWPAD + c] view of buf is bitwise SENTINEL."""
    b = buf.detach().cpu()
    inside = torch.zeros(b.shape, dtype=torch.bool)
    inside[..., :p, ROWPAD:ROWPAD + c] = True
    want = torch.full((), SENTINEL, dtype=b.dtype)
    assert bool((bits(b)[~inside] == bits(want)).all()), "%s: written outside the view" % what


def rows_of(t4):
    return K.nhwc(t4)


def wf_of(wt, dt, dev):
    """[Cout, Cin, KH, KW] -> the forward operand [Cout][KH][KW][Cin]."""
    co, ci, kh, kw = wt.shape
    return wt.permute(0, 2, 3, 1).reshape(co, kh * kw * ci).to(dt).to(dev).contiguous()


def wt_of(wt, dt, dev):
    """[Cout, Cin, KH, KW] -> the dgrad operand [Cin][KH][KW][Cout]."""
    co, ci, kh, kw = wt.shape
    return wt.permute(1, 2, 3, 0).reshape(ci, kh * kw * co).to(dt).to(dev).contiguous()


def dw_rows(ref):
    """[Cout, Cin, KH, KW] -> [Cout * KH * KW * Cin] fp32 in the library's order."""
    return ref.permute(0, 2, 3, 1).reshape(-1).to(f32)


# ---- runners --------------------------------------------------------------------------------
def run_fwd(dev, dt, pr, bias=True, what="fwd"):
    n, cin, h, w, cout, k, s, p, d = pr.case
    out = pr.outs["fwd"] if bias else Out(pr.outs["fwd"].ref - pr.bias.view(1, -1, 1, 1), pr.outs["fwd"].bound)
    verify(out)
    m = n * pr.oh * pr.ow
    ybuf, yv = output(m, cout, dt, dev)
    ops.conv_fwd(operand(rows_of(pr.x), dt, dev), n, h, w, wf_of(pr.w, dt, dev), cout, k, s, p, d,
                 bias=pr.bias.to(f32).to(dev) if bias else None, out=yv)
    torch.cuda.synchronize()
    same(yv, rows_of(out.expect(dt)), "%s %s" % (what, pr.case))
    untouched(ybuf, m, cout, what)


def run_dgrad(dev, dt, pr, accumulate, what="dgrad"):
    n, cin, h, w, cout, k, s, p, d = pr.case
    out = pr.outs["dgrad_acc" if accumulate else "dgrad"]
    verify(out)
    dbuf, dv = output(n * h * w, cin, dt, dev, old=rows_of(pr.old) if accumulate else None)
    ops.conv_dgrad(operand(rows_of(pr.gy), dt, dev), n, pr.oh, pr.ow, wt_of(pr.w, dt, dev), cin, k, s, p, d,
                   h, w, out=dv, accumulate=accumulate)
    torch.cuda.synchronize()
    same(dv, rows_of(out.expect(dt)), "%s accumulate=%s %s" % (what, accumulate, pr.case))
    untouched(dbuf, n * h * w, cin, what)


def run_wgrad(dev, dt, pr, what="wgrad"):
    n, cin, h, w, cout, k, s, p, d = pr.case
    out = pr.outs["wgrad"]
    verify(out)
    wbuf, dw = flat_output(cout * k * k * cin, dev)
    ops.conv_wgrad(operand(rows_of(pr.x), dt, dev), n, h, w, cin, operand(rows_of(pr.gy), dt, dev),
                   pr.oh, pr.ow, cout, k, s, p, d, dw=dw)
    torch.cuda.synchronize()
    same(dw, dw_rows(out.ref), "%s %s" % (what, pr.case))
    same(wbuf[dw.numel():], torch.full((wbuf.numel() - dw.numel(),), SENTINEL), what + " tail")


def run_wgrad_grouped(dev, dt, case, seeds, split):
    n, cin, h, w, cout, k, s, p, d = case
    prs = [conv_problem(case, ROUND, sd) for sd in seeds]
    jobs, bufs = [], []
    for pr in prs:
        verify(pr.outs["wgrad"])
        wbuf, dw = flat_output(cout * k * k * cin, dev)
        bufs.append(wbuf)
        jobs.append((operand(rows_of(pr.x), dt, dev), operand(rows_of(pr.gy), dt, dev), dw))
    if split:
        assert nv.query("cn_conv_wgrad_grouped_workspace_floats", nv.dtype_code(dt), len(prs), n, prs[0].oh,
                        prs[0].ow, cout, k, k, cin) > 0
    ops.conv_wgrad_grouped(jobs, n, h, w, cin, prs[0].oh, prs[0].ow, cout, k, s, p, d, split=split)
    torch.cuda.synchronize()
    for g, (pr, job, wbuf) in enumerate(zip(prs, jobs, bufs)):
        what = "wgrad grouped g%d split=%s %s" % (g, split, case)
        same(job[2], dw_rows(pr.outs["wgrad"].ref), what)
        same(wbuf[job[2].numel():], torch.full((wbuf.numel() - job[2].numel(),), SENTINEL), what + " tail")


def run_conv_all(dev, dt, case):
    pr = conv_problem(case)
    run_fwd(dev, dt, pr)
    if has_dgrad(case):
        run_dgrad(dev, dt, pr, False)
        run_dgrad(dev, dt, pr, True)
    run_wgrad(dev, dt, pr)


# ---- 1. forward, dgrad, wgrad ---------------------------------------------------------------
@pytest.mark.parametrize("dt", [f32, bf])
@pytest.mark.parametrize("case", CONV_CASES)
def test_conv_fwd_dgrad_wgrad_exact(cuda, dt, case):
    """cn_conv_fwd (bias), cn_conv_dgrad (store and accumulate; the stride-2 row map on strided
    rows included), cn_conv_wgrad, and the same weight gradient as problem 0 of a whole-K group of
    three (cn_conv_wgrad_grouped)."""
    run_conv_all(cuda, dt, case)
    run_wgrad_grouped(cuda, dt, case, (0, 1, 2), split=False)


@pytest.mark.parametrize("dt", [f32, bf])
def test_conv_wgrad_grouped_split_exact(cuda, dt):
    """cn_conv_wgrad_grouped_ws: G = 2 problems split over K into slabs + one reduce launch."""
    run_wgrad_grouped(cuda, dt, WGRAD_SPLIT_CASE, (0, 1), split=True)


# ---- 2. split-K forward ---------------------------------------------------------------------
def test_conv_fwd_split_k_exact(cuda):
    """cn_conv_fwd_ws (K = 18432): the fp32 slabs are summed, the bias added and the sum rounded
    once; a reduce that rounded before the bias would miss the ties."""
    pr = conv_problem(SPLIT_K_CASE, ROUND, 0, False)
    n, cin, h, w, cout, k, s, p, d = SPLIT_K_CASE
    xv = operand(rows_of(pr.x), bf, cuda)
    assert ops.fwd_split_floats(xv, n * pr.oh * pr.ow, cout, k * k * cin) > 0
    run_fwd(cuda, bf, pr, what="split-K fwd")


# ---- 3. every tile configuration ------------------------------------------------------------
@pytest.fixture
def force_cfg():
    lib = nv.load()
    yield lib.cn_gemm_force_config
    lib.cn_gemm_force_config(-1)


@pytest.mark.parametrize("cfg", CFGS)
def test_every_tile_config_exact(cuda, force_cfg, cfg):
    assert force_cfg(cfg) > cfg
    for case in CFG_CASES:
        run_conv_all(cuda, bf, case)


# ---- 4. weight-stationary kernel ------------------------------------------------------------
@pytest.fixture
def ws_mode():
    lib = nv.load()
    prev = lib.cn_gemm_ws_mode(1)
    yield lib.cn_gemm_ws_mode
    lib.cn_gemm_force_config(-1)
    lib.cn_gemm_ws_mode(prev)


def test_weight_stationary_exact(cuda, ws_mode):
    """cn_gemm_ws_mode(2).  Of WS_CASE the kernel takes the bias-free forward (K = 128; a bias, and
    the dgrad's K = 328, stay on the generic kernel, exact all the same); of its transpose it takes
    both dgrads (K = 128), the accumulating one on old-C ties."""
    assert ws_mode(2) >= 0
    launches = lambda: int(nv.load().cn_gemm_ws_launches())
    pr = conv_problem(WS_CASE)
    before = launches()
    run_fwd(cuda, bf, pr)
    run_dgrad(cuda, bf, pr, False)
    run_dgrad(cuda, bf, pr, True)
    assert launches() == before
    run_fwd(cuda, bf, pr, bias=False, what="ws fwd")
    assert launches() == before + 1
    prt = conv_problem(WS_CASE_T)
    run_dgrad(cuda, bf, prt, False, what="ws dgrad")
    run_dgrad(cuda, bf, prt, True, what="ws dgrad")
    assert launches() == before + 3


# ---- 5. cn_gemm direct ----------------------------------------------------------------------
def gemm_operand(t, layout, dt, dev):
    """t [B, rows, K] -> (view, ld, batch stride) stored k-contiguous (0) or k-major (2: [K][rows],
    the row length rounded up to 8 so rows stay 16-byte aligned; the round-up columns are NaN)."""
    b, r, k = t.shape
    if layout == 0:
        v = operand(t, dt, dev)
    else:
        tt = t.transpose(1, 2)
        r8 = (r + 7) // 8 * 8
        wide = torch.full((b, k, r8), float("nan"), dtype=torch.float64)
        wide[:, :, :r] = tt
        v = operand(wide, dt, dev)
    return v, v.stride(1), v.stride(0)


@pytest.mark.parametrize("dt,odt", [(bf, bf), (bf, f32), (f32, f32)])
@pytest.mark.parametrize("la,lb", GEMM_LAYOUTS)
def test_gemm_exact(cuda, dt, odt, la, lb):
    """cn_gemm, batch 3, every layout pair: c_mode 0 with alpha in {1, 0.5}, with and without
    bias; c_mode 2 (bf16 C, alpha 1, no bias) onto an old C in the rounding regime."""
    B, M, N, Kd = GEMM_BMNK
    pr = gemm_problem(B, M, N, Kd)
    A, lda, abs_ = gemm_operand(pr.a, la, dt, cuda)
    Bt, ldb, bbs = gemm_operand(pr.b, lb, dt, cuda)
    bias = pr.bias.to(f32).to(cuda)
    modes = [("plain", a, 0) for a in (1.0, 0.5)] + [("bias", a, 0) for a in (1.0, 0.5)]
    if odt == bf:
        modes.append(("acc", 1.0, 2))
    for kind, alpha, c_mode in modes:
        out = pr.outs[kind, alpha]
        verify(out)
        cbuf, cv = output(M, N, odt, cuda, old=pr.old if c_mode == 2 else None, lead=(B,))
        ops.gemm(A, Bt, M, N, Kd, layout_a=la, layout_b=lb, lda=lda, ldb=ldb, a_bs=abs_, b_bs=bbs, out=cv,
                 ldc=cv.stride(1), c_bs=cv.stride(0), c_mode=c_mode, batch=B, alpha=alpha,
                 bias=bias if kind == "bias" else None)
        torch.cuda.synchronize()
        same(cv, out.expect(odt), "gemm %s alpha=%g" % (kind, alpha))
        untouched(cbuf, M, N, "gemm %s" % kind)


@pytest.mark.parametrize("dt", [bf, f32])
def test_gemm_split_k_exact(cuda, dt):
    """Split-K, both k-major operands (the weight-gradient form), nsplit 7: c_mode 1 (fp32 atomic
    adds onto an old C, strided rows) and the slab path of ops.gemm (dense C; store and add)."""
    M, N, Kd = GEMM_ATOMIC_MNK
    pr = gemm_problem(1, M, N, Kd, seed=2)
    A, lda, _ = gemm_operand(pr.a, 2, dt, cuda)
    Bt, ldb, _ = gemm_operand(pr.b, 2, dt, cuda)
    verify(pr.outs["acc", 1.0])
    verify(pr.outs["plain", 1.0])
    cbuf, cv = output(M, N, f32, cuda, old=pr.old[0])
    ops.gemm(A, Bt, M, N, Kd, layout_a=2, layout_b=2, lda=lda, ldb=ldb, out=cv, ldc=cv.stride(0), c_mode=1, nsplit=7)
    torch.cuda.synchronize()
    same(cv, pr.outs["acc", 1.0].expect(f32)[0], "gemm atomic")
    untouched(cbuf, M, N, "gemm atomic")
    for c_mode, key in ((0, "plain"), (1, "acc")):
        buf = torch.full((M + ROWS_PAST, N), SENTINEL, dtype=f32)
        buf[:M] = float("nan") if c_mode == 0 else pr.old[0].to(f32)
        buf = buf.to(cuda)
        ops.gemm(A, Bt, M, N, Kd, layout_a=2, layout_b=2, lda=lda, ldb=ldb, out=buf[:M], ldc=N, c_mode=c_mode, nsplit=7)
        torch.cuda.synchronize()
        same(buf[:M], pr.outs[key, 1.0].expect(f32)[0], "gemm slabs c_mode %d" % c_mode)
        same(buf[M:], torch.full((ROWS_PAST, N), SENTINEL), "gemm slabs tail")


@pytest.mark.parametrize("dt", [bf, f32])
def test_gemm_kb_lim_exact(cuda, dt):
    """The co-attention's P.V call form (A k-contiguous, B k-major, kb_lim < K): B holds NaN from
    row kb_lim on, so the result is finite and exact only if the bound is honoured."""
    B, M, N, Kd = GEMM_BMNK
    pr = gemm_problem(B, M, N, Kd, seed=1, kb_lim=GEMM_KB_LIM)
    bnan = pr.b.clone()
    bnan[:, :, GEMM_KB_LIM:] = float("nan")
    A, lda, abs_ = gemm_operand(pr.a, 0, dt, cuda)
    Bt, ldb, bbs = gemm_operand(bnan, 2, dt, cuda)
    out = pr.outs["bias", 1.0]
    verify(out)
    cbuf, cv = output(M, N, dt, cuda, lead=(B,))
    ops.gemm(A, Bt, M, N, Kd, layout_b=2, lda=lda, ldb=ldb, a_bs=abs_, b_bs=bbs, out=cv, ldc=cv.stride(1),
             c_bs=cv.stride(0), batch=B, kb_lim=GEMM_KB_LIM, bias=pr.bias.to(f32).to(cuda))
    torch.cuda.synchronize()
    same(cv, out.expect(dt), "gemm kb_lim")
    untouched(cbuf, M, N, "gemm kb_lim")


# ---- 6. BN-statistics epilogue --------------------------------------------------------------
# The statistics kernels sum in fp32 (exact on integer data below 2^24) and finish in double:
# mean, invstd and the running statistics are float roundings of a double evaluation.  On exact
# sums they equal the float rounding of the EXACT value wherever that value lies further from a
# float32 rounding boundary than the double evaluation can err, which stats_reference proves per
# channel on the CPU (the margin condition) -- so the comparison is bitwise.
BN_MOMENTUM32 = float(torch.tensor(0.1, dtype=f32))    # the float arguments, widened to double
BN_EPS32 = float(torch.tensor(1e-5, dtype=f32))
MARGIN = 8                 # x the measured fp64-vs-exact difference
ULP64 = 2.0 ** -52         # floor of that difference, relative: 2 ulp for a device sqrt / fma


def _fma(a, b, c):
    """One rounding of a * b + c, as a contracted device expression evaluates it."""
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def _f32(v):
    return float(np.float32(v))


def round_f32_with_margin(exact, evals):
    """(float32 rounding of the Fraction `exact`, margin condition holds): the distance of `exact`
    to the nearer float32 rounding boundary must exceed MARGIN x the largest difference between
    `exact` and the fp64 evaluations `evals` of the kernel's formula (at least 2 ulp of fp64)."""
    r = _f32(float(exact))
    lo = float(np.nextafter(np.float32(r), np.float32(-np.inf)))
    hi = float(np.nextafter(np.float32(r), np.float32(np.inf)))
    dist = min(abs(exact - (Fraction(lo) + Fraction(r)) / 2), abs(exact - (Fraction(hi) + Fraction(r)) / 2))
    diff = max([abs(Fraction(e) - exact) for e in evals] + [abs(exact) * Fraction(ULP64)])
    ok = dist > MARGIN * diff and all(_f32(e) == r for e in evals)
    return r, ok


def _exact_rsqrt(v):
    """1 / sqrt(v) of a Fraction to 60 digits, as a Fraction."""
    with decimal.localcontext() as ctx:
        ctx.prec = 60
        d = decimal.Decimal(v.numerator) / decimal.Decimal(v.denominator)
        return Fraction(1 / d.sqrt())


def stats_reference(s1, s2, n, shift, rm, rv, tile_form=False):
    """Float32 statistics of one channel over its segments, from exact integer sums.

    s1[g], s2[g]: sum (x - shift[g]) and sum (x - shift[g])^2 of segment g (Python ints), n rows a
    segment, rm / rv the running statistics before (float32 values).  tile_form False mirrors
    bn_stats_finalize (q = s2 - s1 * md, var = q / n, unbiased q / (n - 1)), True
    bn_tile_stats_finalize (shift 0; var = s2 / n - md * md, unbiased var * n / (n - 1)); both in
    double with and without fma contraction, the running update rounded to float per segment.
    Returns (mean[g], invstd[g], running_mean, running_var, margin condition holds for all)."""
    m, eps, ok = BN_MOMENTUM32, BN_EPS32, True
    means, invstds = [], []
    for g in range(len(s1)):
        a, b, k = float(s1[g]), float(s2[g]), float(shift[g])
        md = a / n
        if tile_form:
            vars64 = [max(b / n - md * md, 0.0), max(_fma(-md, md, b / n), 0.0)]
            unb64 = [v * n / (n - 1) for v in vars64]
        else:
            qs = [max(b - a * md, 0.0), max(_fma(-a, md, b), 0.0)]
            vars64, unb64 = [q / n for q in qs], [q / (n - 1) for q in qs]
        mean64 = k + md
        e_mean = Fraction(shift[g]) + Fraction(s1[g], n)
        e_q = Fraction(s2[g]) - Fraction(s1[g]) ** 2 / n
        e_var, e_unb = e_q / n, e_q / (n - 1)
        r, o = round_f32_with_margin(e_mean, [mean64])
        means.append(r)
        ok &= o
        r, o = round_f32_with_margin(_exact_rsqrt(e_var + Fraction(eps)), [1.0 / math.sqrt(v + eps) for v in vars64])
        invstds.append(r)
        ok &= o
        e_rm = (1 - Fraction(m)) * Fraction(rm) + Fraction(m) * e_mean
        rm, o = round_f32_with_margin(e_rm, [(1.0 - m) * rm + m * mean64, _fma(1.0 - m, rm, m * mean64),
                                             _fma(m, mean64, (1.0 - m) * rm)])
        ok &= o
        e_rv = (1 - Fraction(m)) * Fraction(rv) + Fraction(m) * e_unb
        ev = []
        for u in unb64:
            ev += [(1.0 - m) * rv + m * u, _fma(1.0 - m, rv, m * u), _fma(m, u, (1.0 - m) * rv)]
        rv, o = round_f32_with_margin(e_rv, ev)
        ok &= o
    return means, invstds, rm, rv, ok


TILE_ROWS = (32, 64, 128, 256)    # the M-tile heights of the conv GEMMs' configurations


def tile_stats_reference(y_ref, n, nseg, cout):
    """(mean, invstd, running_mean, running_var) float32, bitwise what the conv epilogue's
    statistics must be for the exact integer y_ref [nseg * n, cout, oh, ow] from fresh running
    statistics (0, 1) -- or None where a per-tile shifted sum could reach 2^24."""
    rows = rows_of(y_ref)
    ys = rows.reshape(nseg, -1, cout)
    cnt = ys.shape[1]
    if not torch.equal(ys, ys.round()):
        return None
    # the per-tile sums are shifted by the tile's first row; whatever the tile height
    for bm in TILE_ROWS:
        for r0 in range(0, rows.shape[0], bm):
            d = rows[r0:r0 + bm] - rows[r0]
            if (d * d).sum(0).max().item() >= 2 ** 24:
                return None
    s1, s2 = ys.sum(1).long().tolist(), (ys * ys).sum(1).long().tolist()
    cols = [stats_reference([s1[g][c] for g in range(nseg)], [s2[g][c] for g in range(nseg)], cnt,
                            [0] * nseg, 0.0, 1.0, tile_form=True) for c in range(cout)]
    assert all(col[4] for col in cols), "margin condition"
    t32 = lambda v: torch.tensor(v, dtype=torch.float64).to(f32)
    return (t32([[col[0][g] for col in cols] for g in range(nseg)]).reshape(-1),
            t32([[col[1][g] for col in cols] for g in range(nseg)]).reshape(-1),
            t32([col[2] for col in cols]), t32([col[3] for col in cols]))


def check_bn_stats(y_ref, n, nseg, cout, mean, invstd, bn, exact=None):
    """test_conv_fwd_bn_epilogue_stats's tolerances, against fp64 statistics of the exact y; and
    bitwise against tile_stats_reference where it applies (exact=True: it must apply)."""
    ref = tile_stats_reference(y_ref, n, nseg, cout)
    assert ref is not None or not exact
    if ref is not None:
        same(mean, ref[0], "epilogue mean")
        same(invstd, ref[1], "epilogue invstd")
        same(bn.running_mean, ref[2], "epilogue running_mean")
        same(bn.running_var, ref[3], "epilogue running_var")
    rm, rv = torch.zeros(cout, dtype=torch.float64), torch.ones(cout, dtype=torch.float64)
    for sg in range(nseg):
        ys = y_ref[sg * n:(sg + 1) * n]
        mu = ys.mean(dim=(0, 2, 3))
        var = ys.var(dim=(0, 2, 3), unbiased=False)
        cnt = ys.numel() // cout
        assert torch.allclose(mean[sg * cout:(sg + 1) * cout].double().cpu(), mu,
                              atol=1e-4 * (1 + mu.abs().max().item()), rtol=1e-5)
        assert torch.allclose(invstd[sg * cout:(sg + 1) * cout].double().cpu(), 1 / torch.sqrt(var + 1e-5), rtol=1e-4)
        rm = 0.9 * rm + 0.1 * mu
        rv = 0.9 * rv + 0.1 * var * cnt / (cnt - 1)
    assert torch.allclose(bn.running_mean.double().cpu(), rm, rtol=1e-4, atol=1e-5)
    assert torch.allclose(bn.running_var.double().cpu(), rv, rtol=1e-4, atol=1e-5)


@pytest.mark.parametrize("dt", [f32, bf])
@pytest.mark.parametrize("case", BN_CASES)
def test_conv_fwd_bn_exact(cuda, dt, case):
    n, cin, h, w, cout, k, s, p, d, nseg = case
    pr = conv_problem((nseg * n,) + case[1:9], REPR, 3, False)
    out = pr.outs["fwd"]
    verify(out)
    bn = K._BN(cout, cuda, 14)
    y, oh, ow, (mean, invstd) = ops.conv_fwd_bn(operand(rows_of(pr.x), dt, cuda), nseg * n, h, w,
                                                wf_of(pr.w, dt, cuda), cout, k, s, p, d, bn, nseg,
                                                bias=pr.bias.to(f32).to(cuda))
    torch.cuda.synchronize()
    same(y, rows_of(out.expect(dt)), "fwd_bn %s" % (case,))
    check_bn_stats(out.ref, n, nseg, cout, mean, invstd, bn, exact=True)


# ---- 7. dgrad fused with the BN + ReLU backward sums ------------------------------------------
@pytest.mark.parametrize("dt", [f32, bf])
@pytest.mark.parametrize("case", DGRAD_BN_CASES)
def test_conv_dgrad_bn_exact(cuda, dt, case):
    """cn_conv_dgrad_bn with the statistics passed in (mean 2, invstd 0.5, gamma +2 / -1, beta
    0.25): the stored gradient, sum dz (dbeta) and sum dz * xhat (dgamma) are all exact."""
    n, cin, h, w, cout, k, p, d = case
    pr = dgrad_bn_problem(case)
    for o in pr.outs.values():
        verify(o)
    bn = K._BN(cin, cuda, 24)
    bn.weight = pr.gamma.to(f32).to(cuda)
    bn.bias = torch.full((cin,), BN_BETA, dtype=f32, device=cuda)
    stats = (torch.full((cin,), BN_MEAN, dtype=f32, device=cuda), torch.full((cin,), BN_INVSTD, dtype=f32, device=cuda))
    dx, dgam, dbet = ops.conv_dgrad_bn(operand(rows_of(pr.gy), dt, cuda), n, h, w, wt_of(pr.w, dt, cuda), cin, k, p, d,
                                       operand(rows_of(pr.x), dt, cuda), stats, bn)
    torch.cuda.synchronize()
    same(dx, rows_of(pr.outs["dx"].expect(dt)), "dgrad_bn dx %s" % (case,))
    same(dbet, pr.outs["dbeta"].expect(f32), "dgrad_bn dbeta")
    same(dgam, pr.outs["dgamma"].expect(f32), "dgrad_bn dgamma")


# ---- 8. fp8 -----------------------------------------------------------------------------------
def fp8_state(scale, dev, fmt=ops.FP8_E4M3):
    return torch.tensor([scale, 1.0 / scale, 0.0, ops.FMT_MAX[fmt]], dtype=f32, device=dev)


E4M3, E5M2 = torch.float8_e4m3fn, torch.float8_e5m2


@pytest.mark.parametrize("case", FP8_FWD_CASES)
def test_conv_fwd_fp8_exact(cuda, case):
    """cn_conv_fwd_fp8 (bias): y = one rounding of acc * sx * sw + bias (a scale applied after the
    rounding would miss the ties)."""
    n, cin, h, w, cout, k, s, p, d = case
    pr = fp8_fwd_problem(case)
    out = pr.outs["fwd"]
    verify(out)
    x8 = operand(fp8_bytes(rows_of(pr.xb), E4M3), torch.uint8, cuda)
    w8 = fp8_bytes(pr.wb.permute(0, 2, 3, 1).reshape(cout, k * k * cin), E4M3).to(cuda).contiguous()
    xs, ws = fp8_state(FP8_SX, cuda), fp8_state(FP8_SW, cuda)
    bias = pr.bias.to(f32).to(cuda)
    m = n * pr.oh * pr.ow
    ybuf, yv = output(m, cout, bf, cuda)
    ops.conv_fwd_fp8(x8, n, h, w, w8, cout, k, s, p, d, xs, ws, bias=bias, out=yv)
    torch.cuda.synchronize()
    want = rows_of(out.expect(bf))
    same(yv, want, "fwd_fp8 %s" % (case,))
    untouched(ybuf, m, cout, "fwd_fp8")
    # bias-free, every e4m3 mantissa bit in use: most outputs are inexact in bf16 (multiples of 1/8)
    full = pr.outs["fwd_full"]
    verify(full)
    ybuf, yv = output(m, cout, bf, cuda)
    ops.conv_fwd_fp8(operand(fp8_bytes(rows_of(pr.xf), E4M3), torch.uint8, cuda), n, h, w,
                     fp8_bytes(pr.wf.permute(0, 2, 3, 1).reshape(cout, k * k * cin), E4M3).to(cuda).contiguous(),
                     cout, k, s, p, d, xs, ws, out=yv)
    torch.cuda.synchronize()
    same(yv, rows_of(full.expect(bf)), "fwd_fp8 full mantissa %s" % (case,))
    untouched(ybuf, m, cout, "fwd_fp8 full mantissa")


@pytest.mark.parametrize("case", FP8_DGRAD_CASES)
@pytest.mark.parametrize("accumulate", [False, True])
def test_conv_dgrad_fp8_exact(cuda, case, accumulate):
    n, cout, h, w, cin, k, p, d = case
    pr = fp8_dgrad_problem(case)
    out = pr.outs["dgrad_acc" if accumulate else "dgrad"]
    verify(out)
    dy8 = operand(fp8_bytes(rows_of(pr.gb), E5M2), torch.uint8, cuda)
    wt8 = fp8_bytes(pr.wb.permute(1, 2, 3, 0).reshape(cin, k * k * cout), E4M3).to(cuda).contiguous()
    dbuf, dv = output(n * h * w, cin, bf, cuda, old=rows_of(pr.old) if accumulate else None)
    ops.conv_dgrad_fp8(dy8, n, h, w, wt8, cin, k, p, d, h, w, fp8_state(FP8_SDY, cuda, ops.FP8_E5M2),
                       fp8_state(FP8_SW, cuda), out=dv, accumulate=accumulate)
    torch.cuda.synchronize()
    same(dv, rows_of(out.expect(bf)), "dgrad_fp8 accumulate=%s %s" % (accumulate, case))
    untouched(dbuf, n * h * w, cin, "dgrad_fp8")


@pytest.mark.parametrize("case", FP8_WGRAD_CASES)
@pytest.mark.parametrize("G", [1, 3])
def test_conv_wgrad_fp8_exact(cuda, case, G):
    """cn_conv_wgrad_fp8, G problems with their own scales (0.5 / 0.25 / 0.125 for both states of
    problem g): fp32, exact."""
    n, cin, h, w, cout, k, s, p, d = case
    prs = [fp8_wgrad_problem(case, g) for g in range(G)]
    jobs, bufs = [], []
    for pr in prs:
        verify(pr.outs["wgrad"])
        wbuf, dw = flat_output(cout * k * k * cin, cuda)
        bufs.append(wbuf)
        jobs.append((operand(fp8_bytes(rows_of(pr.xb), E4M3), torch.uint8, cuda), fp8_state(pr.scale, cuda),
                     operand(fp8_bytes(rows_of(pr.gb), E5M2), torch.uint8, cuda),
                     fp8_state(pr.scale, cuda, ops.FP8_E5M2), dw))
    ops.conv_wgrad_fp8(jobs, n, h, w, cin, prs[0].oh, prs[0].ow, cout, k, s, p, d)
    torch.cuda.synchronize()
    for g, (pr, job, wbuf) in enumerate(zip(prs, jobs, bufs)):
        same(job[4], dw_rows(pr.outs["wgrad"].ref), "wgrad_fp8 g%d %s" % (g, case))
        same(wbuf[job[4].numel():], torch.full((wbuf.numel() - job[4].numel(),), SENTINEL), "wgrad_fp8 tail")
