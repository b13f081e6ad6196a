"""cn_conv_fwd_affine (include/cosnet_hip_infer.h): a forward conv with an eval-mode BatchNorm, the
residual add and the activation in its GEMM epilogue -- bitwise, no tolerance.

The generators and the buffers are tests/test_gpu_exact_gemm.py's: integer operands (x in
[-4, 4], w in [-3, 3]) make the accumulator exact, `scale` in {1/2, 1, 2} per channel keeps the
product exact, `shift` = offset_bias and `res` = old_c put the pre-activation values where bf16's
spacing is >= 1, so a share of them are exact ties.  The contract then reads bitwise: the stored
value is ONE round-to-nearest-even rounding of act(fma(acc + bias, scale, shift) + res) (bf16), or
that value itself (fp32).  A kernel that rounded the raw conv output, the affine or the residual
sum first would miss the ties; tests/test_cpu_bn_fold.py checks the generators' guard conditions
without a GPU.

Operands and outputs are strided views in NaN / sentinel-filled buffers, as in that file.

Not reachable through the C ABI, hence not tested: st_mode 4 together with a group or a K split
of the GEMM itself (cn_conv_fwd_affine builds neither: its split-K route applies the affine in the
reduce, test_split_k_route).
"""
import functools
from types import SimpleNamespace

import pytest
import torch
import torch.nn as nn

from cosnet_amd import _native as nv
from cosnet_amd import ops

import test_gpu_exact_gemm as E
from test_gpu_exact_gemm import (CFG_CASES, SPLIT_K_CASE, WS_CASE, Out, bf, bound_of, conv_problem, f32, ints,
                                 offset_bias, old_c, operand, output, rows_of, same, untouched, wf_of)

pytestmark = pytest.mark.gpu

# n, cin, h, w, cout, k, stride, pad, dil
AFFINE_CASES = [
    (2, 64, 13, 11, 128, 1, 1, 0, 1),
    (2, 64, 13, 11, 64, 3, 1, 1, 1),
    (2, 32, 15, 9, 64, 3, 1, 2, 2),
    (2, 256, 7, 9, 128, 1, 2, 0, 1),     # stride-2 1x1: an ordinary forward gather
    (2, 8, 29, 31, 64, 7, 2, 3, 1),      # the stem (8 padded channels: K tiles straddle taps)
    (1, 64, 9, 9, 512, 3, 1, 6, 6),
    (4, 2048, 1, 1, 512, 1, 1, 0, 1),    # the ASPP pooling branch, M = 4
]
TILE_CASE = CFG_CASES[0]                 # (2, 96, 21, 23, 320, 1, 1, 0, 1)
EPI_TILES = (10, 11, 12, 13, 18, 19, 20)  # gemm.hip launch_epi
PRELU_SLOPE = 0.25
ACTS = (0, 1, 2)
MIN_TIES_PRE, MIN_TIES_RELU, ZEROS = 0.10, 0.05, (0.40, 0.60)


def act_of(t, act):
    if act == 1:
        return t.clamp_min(0.0)
    if act == 2:
        return torch.where(t > 0, t, PRELU_SLOPE * t)
    return t


def affine_scale(c, seed):
    """1/2, 1 or 2 per channel."""
    return torch.tensor([0.5, 1.0, 2.0], dtype=torch.float64)[ints((c,), 0, 2, seed).long()]


def affine_problem(case, act, with_res, with_bias, seed=0):
    return _affine_problem(case, act, with_res, with_bias, seed)


@functools.lru_cache(maxsize=None)
def _affine_problem(case, act, with_res, with_bias, seed):
    """The exact pre-activation and stored values of one folded conv on conv_problem(case)'s x, w
    and bias (never written)."""
    n, cin, h, w, cout, k, s, p, d = case
    pr = conv_problem(case, E.ROUND, seed, False)
    sd = 100 * seed + 7000
    acc = pr.outs["fwd"].ref if with_bias else pr.outs["fwd"].ref - pr.bias.view(1, -1, 1, 1)
    scale, shift = affine_scale(cout, sd + 1), offset_bias(cout, sd + 2)
    res = old_c(acc.shape, sd + 3) if with_res else None
    pre = acc * scale.view(1, -1, 1, 1) + shift.view(1, -1, 1, 1)
    if res is not None:
        pre = pre + res
    bound = 2 * bound_of(k * k * cin, pr.x, pr.w, pr.bias if with_bias else None) + E.amax(shift) + E.amax(res)
    return SimpleNamespace(conv=pr, scale=scale, shift=shift, res=res, act=act,
                           pre=Out(pre, bound, step=0.5),
                           out=Out(act_of(pre, act), bound, step=0.5 * (PRELU_SLOPE if act == 2 else 1.0)))


def verify_affine(ap):
    """The guard conditions of one folded comparison (CPU): the pre-activation value is exact in
    fp32 and below 2^24 with >= 10 % exact bf16 ties; after a ReLU >= 5 % of the stored values are
    ties and 40-60 % are zero.  Returns (tie share before, after the activation, zero share)."""
    E.verify(ap.pre)
    E.verify(ap.out)
    pre, post = E.tie_share(ap.pre.ref), E.tie_share(ap.out.ref)
    zeros = (ap.out.ref == 0).double().mean().item()
    assert pre >= MIN_TIES_PRE, pre
    if ap.act == 1:
        assert post >= MIN_TIES_RELU, post
        assert ZEROS[0] <= zeros <= ZEROS[1], zeros
    return pre, post, zeros


def all_affine_problems():
    """(label, problem) of every comparison of this file on the integer generators."""
    res = []
    for case in AFFINE_CASES + [TILE_CASE, SPLIT_K_CASE, WS_CASE]:
        for act in ACTS:
            for with_res in (False, True):
                for with_bias in (False, True):
                    res.append(("%s act %d res %d bias %d" % (case, act, with_res, with_bias),
                                affine_problem(case, act, with_res, with_bias)))
    return res


def run_affine(dev, dt, case, act, with_res, with_bias, what="affine"):
    ap = affine_problem(case, act, with_res, with_bias)
    verify_affine(ap)
    pr = ap.conv
    n, cin, h, w, cout, k, s, p, d = case
    m = n * pr.oh * pr.ow
    ybuf, yv = output(m, cout, dt, dev)
    res = operand(rows_of(ap.res), dt, dev) if with_res else None
    prelu = torch.tensor([PRELU_SLOPE], dtype=f32, device=dev) if act == 2 else None
    ops.conv_fwd_affine(operand(rows_of(pr.x), dt, dev), n, h, w, wf_of(pr.w, dt, dev), cout, k, s, p, d,
                        ap.scale.to(f32).to(dev), ap.shift.to(f32).to(dev), act=act, prelu=prelu, res=res,
                        bias=pr.bias.to(f32).to(dev) if with_bias else None, out=yv)
    torch.cuda.synchronize()
    label = "%s %s act %d res %d bias %d" % (what, case, act, with_res, with_bias)
    same(yv, rows_of(ap.out.expect(dt)), label)
    untouched(ybuf, m, cout, label)
    return yv


# ---- T3: the contract, every loader, both dtypes --------------------------------------------------
@pytest.mark.parametrize("dt", [f32, bf])
@pytest.mark.parametrize("case", AFFINE_CASES)
def test_conv_fwd_affine_exact(cuda, dt, case):
    """act 0 / 1 / 2, with and without a residual, with and without a bias."""
    for act in ACTS:
        for with_res in (False, True):
            for with_bias in (False, True):
                run_affine(cuda, dt, case, act, with_res, with_bias)


@pytest.fixture
def force_cfg():
    lib = nv.load()
    yield lib.cn_gemm_force_config
    lib.cn_gemm_force_config(-1)


@pytest.mark.parametrize("cfg", EPI_TILES)
def test_conv_fwd_affine_every_epilogue_tile(cuda, force_cfg, cfg):
    """Every tile launch_epi instantiates (M = 966, N = 320: ragged in both directions)."""
    force_cfg(cfg)
    for act, with_res in ((1, True), (2, False)):
        run_affine(cuda, bf, TILE_CASE, act, with_res, True, what="tile %d" % cfg)


def test_conv_fwd_affine_refuses_a_tile_without_the_epilogue(cuda, force_cfg):
    force_cfg(0)
    with pytest.raises(nv.NativeError, match="unsupported"):
        run_affine(cuda, bf, TILE_CASE, 1, True, True)


def test_split_k_route(cuda):
    """K = 18432 splits over K (cn_conv_fwd_workspace_floats > 0): bias, affine, residual and
    activation in the reduce, one rounding after them."""
    n, cin, h, w, cout, k, s, p, d = SPLIT_K_CASE
    pr = conv_problem(SPLIT_K_CASE, E.ROUND, 0, False)
    xv = operand(rows_of(pr.x), bf, cuda)
    assert ops.fwd_split_floats(xv, n * pr.oh * pr.ow, cout, k * k * cin) > 0
    for act, with_res, with_bias in ((1, True, True), (2, False, True), (0, True, False)):
        run_affine(cuda, bf, SPLIT_K_CASE, act, with_res, with_bias, what="split-K")


def test_conv_fwd_affine_weight_stationary_kernel(cuda):
    """The weight-stationary kernel's folded epilogue (gemm_ws.hip FOLD 1 / 2) under
    cn_gemm_ws_mode 2 (every eligible problem) and 3 (one M walker per XCD: long tile walks), with
    and without a residual: a ws launch is counted, and the output is the exact value and bitwise
    the generic epilogue's (mode 0)."""
    lib = nv.load()
    prev = lib.cn_gemm_ws_mode(0)
    try:
        generic = {}
        before = lib.cn_gemm_ws_launches()
        for act, with_res in ((1, True), (0, False), (1, False)):
            generic[act, with_res] = run_affine(cuda, bf, WS_CASE, act, with_res, False, what="ws off").clone()
        assert lib.cn_gemm_ws_launches() == before
        for mode in (2, 3):
            lib.cn_gemm_ws_mode(mode)
            for (act, with_res), ref in generic.items():
                before = lib.cn_gemm_ws_launches()
                got = run_affine(cuda, bf, WS_CASE, act, with_res, False, what="ws mode %d" % mode)
                assert lib.cn_gemm_ws_launches() == before + 1
                assert torch.equal(got.view(torch.int16), ref.view(torch.int16))
            # PReLU and a bias stay on the generic epilogue
            before = lib.cn_gemm_ws_launches()
            run_affine(cuda, bf, WS_CASE, 2, True, False, what="ws mode %d" % mode)
            run_affine(cuda, bf, WS_CASE, 1, True, True, what="ws mode %d" % mode)
            assert lib.cn_gemm_ws_launches() == before
    finally:
        lib.cn_gemm_ws_mode(prev)


# ---- T3b: one rounding on real values -------------------------------------------------------------
@pytest.mark.parametrize("m,cin,cout,act,with_res", [(286, 64, 128, 1, True), (286, 256, 64, 0, False),
                                                     (1000, 128, 512, 2, True)])
def test_conv_fwd_affine_is_one_rounding_of_the_fp32_apply(cuda, m, cin, cout, act, with_res):
    """Random bf16 data, 1x1: conv_fwd_affine (bf16) is bitwise bn_apply in fp32 on the fp32
    product of the same bf16 operands (ops.gemm, out_dtype fp32: the same tile, the same
    accumulation order), with the fold table's scale and shift, cast to bf16 -- no bf16 raw conv
    output in between."""
    g = torch.Generator().manual_seed(m + cin)
    x = torch.randn((m, cin), generator=g).to(bf).to(cuda)
    wf = (torch.randn((cout, cin), generator=g) * 0.1).to(bf).to(cuda)
    res = torch.randn((m, cout), generator=g).to(bf).to(cuda) if with_res else None
    bn = nn.BatchNorm2d(cout)
    bn.running_mean.copy_(torch.randn((cout,), generator=g) * 0.3)
    bn.running_var.copy_(torch.rand((cout,), generator=g) + 0.5)
    bn.weight.data.copy_(torch.rand((cout,), generator=g) + 0.5)
    bn.bias.data.copy_(torch.randn((cout,), generator=g) * 0.2)
    bn = bn.to(cuda).eval()
    prelu = torch.tensor([PRELU_SLOPE], dtype=f32, device=cuda) if act == 2 else None
    with torch.no_grad():
        sc, sf = ops.bn_fold_table(bn)
        got, _, _ = ops.conv_fwd_affine(x, 1, m, 1, wf, cout, 1, 1, 0, 1, sc, sf, act=act, prelu=prelu, res=res)
        c32 = ops.gemm(x, wf, m, cout, cin, lda=cin, ldb=cin, out_dtype=f32)
        y32 = ops.bn_apply(c32, ops.bn_stats(c32, bn, False), bn, act=act, prelu=prelu,
                           res=res.float() if with_res else None)
    torch.cuda.synchronize()
    assert torch.isfinite(y32).all()
    same(got, y32.to(bf).cpu(), "folded vs fp32 apply m %d cin %d cout %d" % (m, cin, cout))


# ---- T3d: error codes -------------------------------------------------------------------------------
def test_conv_fwd_affine_error_codes(cuda):
    case = AFFINE_CASES[0]
    n, cin, h, w, cout, k, s, p, d = case
    pr = conv_problem(case, E.ROUND, 0, False)
    x, wf = operand(rows_of(pr.x), bf, cuda), wf_of(pr.w, bf, cuda)
    _, yv = output(n * pr.oh * pr.ow, cout, bf, cuda)
    tab = torch.ones((cout + 4,), dtype=f32, device=cuda)
    ok, off = tab[:cout], tab[1:cout + 1]            # off: 4 bytes past a 16-byte boundary
    call = lambda sc, sf, **kw: ops.conv_fwd_affine(x, n, h, w, wf, cout, k, s, p, d, sc, sf, out=yv, **kw)
    with pytest.raises(nv.NativeError, match="alignment"):
        call(off, ok)
    with pytest.raises(nv.NativeError, match="alignment"):
        call(ok, off)
    with pytest.raises(nv.NativeError, match="unsupported"):
        call(ok, ok, act=2)                           # PReLU without its slope
    with pytest.raises(nv.NativeError, match="unsupported"):
        call(ok, ok, act=3)
    with pytest.raises(ValueError):
        call(ok[:cout - 8], ok)
    call(ok, ok, act=1)                               # the same call with valid arguments runs
    torch.cuda.synchronize()
