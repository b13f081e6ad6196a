"""Exact-arithmetic parity of the BatchNorm kernels (bn.hip) -- bitwise, no tolerance.

The inputs are chosen so that every intermediate of every kernel is exact in fp32 and independent
of the order of evaluation: activations are small integers around an integer mean, invstd a power
of two in {1, 1/2, 1/4}, gamma from {2, -1, 1/2, 1, 0}, beta a multiple of 1/4, gradients integers
in [-4, 4], PReLU's a = 1/4.  Then the contract of include/cosnet_hip.h reads bitwise: fp32
outputs equal the exact value, bf16 outputs ONE round-to-nearest-even rounding of it, the fp8 copy
and its amax come from the fp32 activation, the mask bits are `stored y > 0`, and the statistics
are the float rounding of the exact mean / invstd / running update (test_gpu_exact_gemm's
stats_reference proves, per channel, that no fp64 last-bit difference can flip that rounding).

About 5 % of the pre-activations are exactly 0 (some as +x - x through the residual), the
residual / second-BN outputs sit where bf16's spacing is 2 (>= 10 % exact ties), and the backward's
dx holds exact bf16 ties as well.  Every activation operand is a strided view in a NaN-filled
buffer, every output a view in a sentinel-filled one that must come back unchanged outside [P, C]
-- the fp8 bytes and the mask bits included.  tests/test_cpu_bn_exact_inputs.py checks the
generators, and that mutated references differ after the rounding, without a GPU.
"""
import functools
from types import SimpleNamespace

import pytest
import torch

from cosnet_amd import _native as nv
from cosnet_amd import ops

import test_gpu_kernels as K
from test_gpu_exact_gemm import (MIN_TIES, ROWPAD, ROWS_PAST, fp8_bytes, ints, is_tie, old_c, operand, output,
                                 rne_bf16, same, stats_reference, untouched)

pytestmark = pytest.mark.gpu

bf, f32, f64 = torch.bfloat16, torch.float32, torch.float64
DTS = [f32, bf]
E4M3 = torch.float8_e4m3fn
PRELU_A = 0.25
MIN_ZEROS = 0.02
BYTE_SENTINEL, BYTE_BLANK = 0x5A, 0xA5

TUNING = (1024, 8, 2048, 4, 512, 4, 2048, 4)    # bn.hip's defaults (blocks, rows per thread) x 4 passes


def vec(dt):
    return 8 if dt == bf else 4


def shapes(dt):
    """(P, C): P in {2, 64, 2048, 2294} x C in {one 16-byte chunk, 40}, C = 320 at P in {64, 2294},
    C = 2560 at P = 64."""
    ps = (2, 64, 2048, 2294)
    return [(p, c) for c in (vec(dt), 40) for p in ps] + [(64, 320), (2294, 320), (64, 2560)]


CASES = [(dt, p, c) for dt in DTS for p, c in shapes(dt)]
CASE_IDS = ["%s-%dx%d" % ("bf16" if dt == bf else "fp32", p, c) for dt, p, c in CASES]
STATS_NSEG = {2: 4, 64: 2, 2048: 1, 2294: 3}    # segments of the statistics case, by P


# ---- the launch layouts of bn.hip, restated (the coverage table) ------------------------------
def layout(c, dt, red):
    """(CPR, CB, RPB): chunks per row, chunk columns and rows of a 256-thread block; the reduction
    passes (statistics, backward sums) use at most 32 chunk columns."""
    cpr = c // vec(dt)
    cb = min(cpr, 32 if red else 256)
    return cpr, cb, 256 // cb


def grid(p, c, dt, blocks, min_rows, nseg=1, red=False):
    """(gridDim.x, gridDim.y) of a pass (grid_rows)."""
    cpr, cb, rpb = layout(c, dt, red)
    gx = -(-cpr // cb)
    want = (blocks // nseg + gx - 1) // gx
    maxy = -(-p // (min_rows * rpb))
    return gx, max(1, min(want, maxy))


def launch_table(dt, p, c, nseg=1):
    """The properties of the four passes' launches at one shape."""
    v = vec(dt)
    st = grid(p, c, dt, TUNING[0], TUNING[1], nseg, True)
    ap = grid(p, c, dt, TUNING[2], TUNING[3], nseg)
    br = grid(p, c, dt, TUNING[4], TUNING[5], 1, True)
    ba = grid(p, c, dt, TUNING[6], TUNING[7])
    red, app = layout(c, dt, True), layout(c, dt, False)
    return SimpleNamespace(
        stat_splits=st[1], bwd_splits=br[1],
        workspace=c * max(nseg * 2 * st[1], 3 * br[1]),
        multi_row_blocks=min(st[1], ap[1], br[1], ba[1]) > 1,
        over_32_splits=st[1] > 32 or br[1] > 32,
        partial_col_block_red=red[0] % red[1] != 0, partial_col_block_apply=app[0] % app[1] != 0,
        idle_threads_red=256 % red[1] != 0, idle_threads_apply=256 % app[1] != 0,
        ncol_not_dividing=red[1] * v < 256 and 256 % (red[1] * v) != 0,
        one_chunk=red[0] == 1,
        rows_past_p_everywhere=p < app[2] and p < red[2])


def coverage():
    """Which shape reaches which property; every property must be reached (asserted on the CPU)."""
    cov = {}
    for dt, p, c in CASES:
        for name, val in vars(launch_table(dt, p, c)).items():
            if isinstance(val, bool) and val:
                cov.setdefault(name, []).append((dt, p, c))
    return cov


COVERED = ("multi_row_blocks", "over_32_splits", "partial_col_block_red", "partial_col_block_apply",
           "idle_threads_red", "idle_threads_apply", "ncol_not_dividing", "one_chunk", "rows_past_p_everywhere")


# ---- per-channel parameters -------------------------------------------------------------------
# (gamma, invstd) by channel % 8: sc = gamma * invstd in {1, -1, 1/8, 1, 0, 2, 1/2, -1/4}
GAMMAS = (2.0, -1.0, 0.5, 1.0, 0.0, 2.0, 1.0, -1.0)
INVSTDS = (0.5, 1.0, 0.25, 1.0, 0.5, 1.0, 0.5, 0.25)
FINE = 2    # the channel class with sc = 1/8: its activations are odd multiples of 1/8


def params(c, nseg, seed, zero_gamma=True, big_beta=False):
    """mean [nseg, C] (integers), invstd [nseg, C], gamma, beta [C].  Segment g rolls the invstd
    table by 3 g and draws its own means.  beta = -sc * k for an integer k in [-3, 3] in the
    channels with |sc| in {1, 1/2} (so x - mean = k gives a pre-activation of exactly 0), another
    multiple of 1/4 in [-2, 2] in the rest.  big_beta: +-100 + an odd multiple of 1/4 in the
    channels % 8 == 5, whose activations then need more than bf16's 8 bits."""
    idx = torch.arange(c) % 8
    gamma = torch.tensor(GAMMAS, dtype=f64)[idx]
    if not zero_gamma:
        gamma = torch.where(gamma == 0, torch.tensor(0.5, dtype=f64), gamma)
    inv = torch.stack([torch.tensor(INVSTDS, dtype=f64)[(idx + 3 * g) % 8] for g in range(nseg)])
    mean = ints((nseg, c), -3, 3, seed + 1)
    sc0 = gamma * inv[0]
    zeroable = (sc0.abs() == 1) | (sc0.abs() == 0.5)
    k = ints((c,), -3, 3, seed + 2)
    beta = torch.where(zeroable, -sc0 * k, ints((c,), -8, 8, seed + 3) / 4)
    if big_beta:
        big = (2 * ints((c,), 0, 1, seed + 4) - 1) * (100 + (2 * ints((c,), 0, 3, seed + 5) + 1) / 4)
        beta = torch.where(idx == 5, big, beta)
    return SimpleNamespace(mean=mean, invstd=inv, gamma=gamma, beta=beta, zero_at=torch.where(zeroable, k, k + 9))


def activations(p, c, par, seed, last=None):
    """x [nseg * P, C] = mean + an integer in [-6, 6], and its exact pre-activation t.  The first
    row holds the zero of every channel that has one (so the smallest shapes have some too)."""
    nseg = par.mean.shape[0]
    d = ints((nseg, p, c), -6, 6, seed)
    d[0, 0] = torch.where(par.zero_at.abs() <= 6, par.zero_at, d[0, 0])
    if last:    # row `last`: a positive pre-activation in every channel that has a zero
        d[0, last] = 6 * torch.sign(par.gamma)
    x = d + par.mean[:, None, :]
    xhat = (x - par.mean[:, None, :]) * par.invstd[:, None, :]
    t = par.gamma * xhat + par.beta
    return x.reshape(nseg * p, c), xhat.reshape(nseg * p, c), t.reshape(nseg * p, c)


def act_of(t, act):
    if act == 1:
        return t.clamp(min=0.0)
    if act == 2:
        return torch.where(t > 0, t, PRELU_A * t)
    return t


def exact32(*vals):
    """Every value is representable in fp32 (so fp32 arithmetic that produced it was exact)."""
    return all(torch.equal(v.to(f32).double(), v) for v in vals)


def expect(ref, dt):
    return ref.to(f32) if dt == f32 else rne_bf16(ref)


def mask_bytes(y, dt):
    """The bit mask of `y > 0`: byte [row, chunk], bit v = channel chunk * vec + v."""
    p, c = y.shape
    v = vec(dt)
    bits = (y > 0).view(p, c // v, v).long()
    return (bits << torch.arange(v)).sum(-1).to(torch.uint8)


# ---- byte outputs (the fp8 copy, the mask) ------------------------------------------------------
def byte_output(p, c, dev, ld_mult=1):
    """(buffer, view [p, c]) of bytes: BYTE_SENTINEL outside the view, BYTE_BLANK inside; the view
    starts at column ROWPAD and the row stride is a multiple of ld_mult."""
    ld = -(-(c + ROWPAD + 3) // ld_mult) * ld_mult
    buf = torch.full((p + ROWS_PAST, ld), BYTE_SENTINEL, dtype=torch.uint8)
    buf[:p, ROWPAD:ROWPAD + c] = BYTE_BLANK
    buf = buf.to(dev)
    return buf, buf[:p, ROWPAD:ROWPAD + c]


def bytes_untouched(buf, p, c, what):
    b = buf.cpu()
    inside = torch.zeros(b.shape, dtype=torch.bool)
    inside[:p, ROWPAD:ROWPAD + c] = True
    assert bool((b[~inside] == BYTE_SENTINEL).all()), "%s: written outside the view" % what


def same_bytes(got, want, what):
    got = got.cpu()
    ne = got != want
    if ne.any():
        idx = ne.nonzero()[:4].tolist()
        raise AssertionError("%s: %d of %d bytes differ, first at %s: got %s, want %s" % (
            what, int(ne.sum()), ne.numel(), idx, got[ne][:4].tolist(), want[ne][:4].tolist()))


# ---- a. statistics ----------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def stats_problem(dt, p, c, nseg):
    """x [nseg * P, C]: a channel offset in [-64, 64] + 16 * segment + an integer in [-6, 6];
    channel 0 constant (var = 0, invstd = 1 / sqrt(eps)), channel 1 constant but for its last row
    (the tail of every loop).  A seed whose margin condition fails in any channel is rejected."""
    for seed in range(700, 708):
        off = ints((c,), -64, 64, seed)
        x = off + 16.0 * torch.arange(nseg, dtype=f64).view(nseg, 1, 1) + ints((nseg, p, c), -6, 6, seed + 50)
        x[:, :, 0] = x[:, :1, 0]
        x[:, :, 1] = x[:, :1, 1]
        x[:, p - 1, 1] += 5.0
        rm0 = ints((c,), -8, 8, seed + 60) / 4
        rv0 = 1 + ints((c,), 0, 8, seed + 61) / 8
        pr = stats_of(x, rm0, rv0)
        if pr.ok:
            assert exact32(x) and (dt == f32 or torch.equal(rne_bf16(x).double(), x))
            return pr
    raise AssertionError("no seed meets the margin condition")


def stats_of(x, rm0, rv0):
    """The float32 statistics of x [nseg, P, C] (stats_reference per channel, the sums shifted by
    the segment's first row as in the kernel) and the bound on those sums."""
    nseg, p, c = x.shape
    shift = x[:, 0, :]
    d = x - shift[:, None, :]
    s1, s2 = d.sum(1), (d * d).sum(1)
    bound = max(d.abs().sum(1).max().item(), s2.max().item())
    s1l, s2l, shl = s1.long().tolist(), s2.long().tolist(), shift.long().tolist()
    cols = [stats_reference([s1l[g][ch] for g in range(nseg)], [s2l[g][ch] for g in range(nseg)], p,
                            [shl[g][ch] for g in range(nseg)], float(rm0[ch]), float(rv0[ch])) for ch in range(c)]
    t32 = lambda v: torch.tensor(v, dtype=f64).to(f32)
    return SimpleNamespace(
        x=x, rm0=rm0, rv0=rv0, bound=bound, ok=all(col[4] for col in cols),
        mean=t32([[col[0][g] for col in cols] for g in range(nseg)]).reshape(-1),
        invstd=t32([[col[1][g] for col in cols] for g in range(nseg)]).reshape(-1),
        running_mean=t32([col[2] for col in cols]), running_var=t32([col[3] for col in cols]))


@pytest.mark.parametrize("dt,p,c", CASES, ids=CASE_IDS)
def test_bn_stats_exact(cuda, dt, p, c):
    """cn_bn_stats, nseg = 4 / 2 / 1 / 3 at P = 2 / 64 / 2048 / 2294: mean, invstd and the running
    statistics (segments in the order a, b, c, d) bitwise the float rounding of the exact value."""
    nseg = STATS_NSEG[p]
    pr = stats_problem(dt, p, c, nseg)
    assert pr.ok and pr.bound < 2 ** 24
    bn = K._BN(c, cuda, 1)
    bn.running_mean, bn.running_var = pr.rm0.to(f32).to(cuda), pr.rv0.to(f32).to(cuda)
    mean, invstd = ops.bn_stats(operand(pr.x.reshape(nseg * p, c), dt, cuda), bn, True, nseg=nseg)
    torch.cuda.synchronize()
    same(mean, pr.mean, "mean")
    same(invstd, pr.invstd, "invstd")
    same(bn.running_mean, pr.running_mean, "running_mean")
    same(bn.running_var, pr.running_var, "running_var")


def test_workspace_matches_the_layout_table(cuda):
    """cn_bn_workspace_floats = C * max(2 * nseg * statistics splits, 3 * backward splits) with the
    splits of this file's restatement of bn.hip's launch arithmetic, at every shape."""
    for dt, p, c in CASES:
        for nseg in (1, STATS_NSEG[p]):
            got = int(nv.query("cn_bn_workspace_floats", nv.dtype_code(dt), p, c, nseg))
            assert got == launch_table(dt, p, c, nseg).workspace, (dt, p, c, nseg)


# ---- b. apply ---------------------------------------------------------------------------------
FORMS = ("plain", "res", "xr")
FORMS_ALL = FORMS + ("fp8",)
CANCEL = 3    # xr form: in the channels % 8 == CANCEL the second BN is minus the first, of xr = x


@functools.lru_cache(maxsize=None)
def apply_problem(dt, p, c, nseg, form):
    """Operands and the exact fp32 activation t[act] of one apply.
    plain  t = bn(x)
    res    + an even residual in +-[256, 510] (odd sums are exact bf16 ties); 6 % of the residuals
           are -bn(x) instead, so the sum is exactly 0 as +x - x
    xr     + a second BN of xr with an integer output of magnitude ~384 (rbeta = +-384 + [-8, 8])
    fp8    + an even residual in +-[16, 72] under qinv = 8, so values past 56 saturate; the first
           two rows of the first sc = 1/8 channel are planted: 96 + an odd multiple of 1/8 (the
           amax, not representable in bf16) and 34 + 1/8 (bf16 rounds it onto the e4m3 midpoint
           34, so bytes taken from the rounded y differ)
    A seed whose draw misses a share the comparisons rest on (zeros, ties, a zero reached as
    +x - x) is rejected; only the smallest shapes ever reject one."""
    for attempt in range(256):
        pr = _apply_problem(dt, p, c, nseg, form, 1000 + 10 * FORMS_ALL.index(form) + nseg + 100 * attempt)
        ok = zero_share(pr) >= MIN_ZEROS or form == "fp8"
        if form == "res":
            ok &= bool(((pr.res == -pr.pre) & (pr.pre != 0)).any())
        if form in ("res", "xr") and dt == bf:
            ok &= is_tie(pr.sum).double().mean().item() >= MIN_TIES
            ok &= all(not torch.equal(rne_bf16(late_add(pr, act)), rne_bf16(pr.t[act])) for act in (0, 1, 2))
        if ok:
            return pr
    raise AssertionError("no seed gives the shares")


def late_add(pr, act):
    """The mutation `rounded to bf16 first, added afterwards`: the first BN's output under a
    residual, the second BN's output in the xr form."""
    if pr.form == "xr":
        return act_of(pr.pre + rne_bf16(pr.sum - pr.pre).double(), act)
    return act_of(rne_bf16(pr.pre).double() + pr.res, act)


def _apply_problem(dt, p, c, nseg, form, sd):
    par = params(c, nseg, sd, big_beta=form != "fp8")
    x, xhat, t = activations(p, c, par, sd + 5)
    pr = SimpleNamespace(par=par, x=x, pre=t, res=None, xr=None, rpar=None, form=form, nseg=nseg)
    if form == "res":
        pr.res = torch.where((ints(t.shape, 0, 15, sd + 6) == 0) & (rne_bf16(t).double() == t), -t,
                             old_c(t.shape, sd + 7))
        t = t + pr.res
    elif form == "xr":
        rpar = params(c, nseg, sd + 20)
        rpar.gamma = torch.tensor((2.0, 1.0, -1.0), dtype=f64)[torch.arange(c) % 3]
        rpar.invstd = torch.ones((nseg, c), dtype=f64)
        sign = (1 - 2 * (torch.arange(c) % 2)).double()
        rpar.beta = sign * 384 + ints((c,), -8, 8, sd + 8)
        cancel = torch.arange(c) % 8 == CANCEL
        rpar.gamma = torch.where(cancel, -par.gamma, rpar.gamma)
        rpar.beta = torch.where(cancel, -par.beta, rpar.beta)
        rpar.invstd = torch.where(cancel, par.invstd, rpar.invstd)
        rpar.mean = torch.where(cancel, par.mean, rpar.mean)
        pr.xr, _, r = activations(p, c, rpar, sd + 9)
        pr.xr = torch.where(cancel, x, pr.xr)
        r = torch.where(cancel, -t, r)
        pr.rpar = rpar
        t = t + r
    elif form == "fp8":
        pr.res = 2 * ints(t.shape, 8, 36, sd + 6) * (2 * ints(t.shape, 0, 1, sd + 7) - 1)
        ch = FINE
        assert par.gamma[ch] * par.invstd[0, ch] == 0.125
        pr.x = x.clone()
        pr.x[0, ch], pr.x[1, ch] = par.mean[0, ch] + 1, par.mean[0, ch] + 3
        pr.pre = t = t.clone()
        t[0, ch], t[1, ch] = 0.125 + par.beta[ch], 0.375 + par.beta[ch]
        pr.res[0, ch] = 96.0
        pr.res[1, ch] = 34.125 - t[1, ch]
        t = t + pr.res
        pr.qinv = 8.0
    pr.sum = t
    pr.t = {act: act_of(t, act) for act in (0, 1, 2)}
    # exactness: every operand in its format, every fp32 intermediate representable
    ops_ = [v for v in (pr.x, pr.res, pr.xr) if v is not None]
    assert exact32(pr.pre, t, *pr.t.values(), *ops_)
    assert dt == f32 or all(torch.equal(rne_bf16(v).double(), v) for v in ops_)
    return pr


def zero_share(pr):
    return (pr.sum == 0).double().mean().item()


def e4m3_of(t, qinv):
    """e4m3(clamp(t * qinv, +-448)) of the fp32 t: (bytes, the clamped scaled values)."""
    v = (t.to(f32) * qinv).clamp(-448.0, 448.0)
    return v.to(E4M3).view(torch.uint8), v.double()


def e4m3_midpoint(v):
    """v (scaled, clamped) lies exactly halfway between two e4m3 codes."""
    m, e = torch.frexp(v.abs())                     # |v| = m * 2^e, m in [0.5, 1)
    half = torch.exp2((e - 1).clamp(min=-6).double() - 4)    # half the spacing: 3 mantissa bits
    q = v.abs() / half
    return (q == q.round()) & (q.round() % 2 == 1)


def launch_apply(dev, dt, pr, act, y, mask=None, out8=None, qstate=None, q8=False):
    par = pr.par
    bn = K._BN(par.gamma.numel(), dev, 1)
    bn.weight, bn.bias = par.gamma.to(f32).to(dev), par.beta.to(f32).to(dev)
    stats = (par.mean.reshape(-1).to(f32).to(dev), par.invstd.reshape(-1).to(f32).to(dev))
    kw = dict(act=act, prelu=torch.tensor([PRELU_A], dtype=f32, device=dev), nseg=pr.nseg)
    if pr.res is not None:
        kw["res"] = operand(pr.res, dt, dev)
    if pr.xr is not None:
        rbn = K._BN(par.gamma.numel(), dev, 2)
        rbn.weight, rbn.bias = pr.rpar.gamma.to(f32).to(dev), pr.rpar.beta.to(f32).to(dev)
        kw.update(xr=operand(pr.xr, dt, dev), rbn=rbn,
                  rstats=(pr.rpar.mean.reshape(-1).to(f32).to(dev), pr.rpar.invstd.reshape(-1).to(f32).to(dev)))
    xv = operand(pr.x, dt, dev)
    if q8:
        ops.bn_apply_q8(xv, stats, bn, qstate, out=y, out8=out8, **kw)
    else:
        ops.bn_apply(xv, stats, bn, out=y, out8=out8, qstate=qstate, mask=mask, **kw)
    torch.cuda.synchronize()


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("dt,p,c", CASES, ids=CASE_IDS)
def test_bn_apply_exact(cuda, dt, p, c, form):
    """cn_bn_apply_ex: plain, + res, + a second BN of xr; act 0, 1, 2; nseg 1 and 2 with their own
    statistics; the mask output with act 0 and 1.  y is one RNE rounding of the exact activation,
    the mask `stored y > 0`, nothing outside the views is written."""
    for nseg in (1, 2):
        pr = apply_problem(dt, p, c, nseg, form)
        assert zero_share(pr) >= MIN_ZEROS
        if form != "plain" and dt == bf:
            assert is_tie(pr.sum).double().mean().item() >= MIN_TIES
        rows = nseg * p
        for act in (0, 1, 2):
            want = expect(pr.t[act], dt)
            ybuf, yv = output(rows, c, dt, cuda)
            mbuf, mv = byte_output(rows, c // vec(dt), cuda) if act != 2 else (None, None)
            launch_apply(cuda, dt, pr, act, yv, mask=mv)
            what = "apply %s act %d nseg %d" % (form, act, nseg)
            same(yv, want, what)
            untouched(ybuf, rows, c, what)
            if mv is not None:
                same_bytes(mv, mask_bytes(want.double(), dt), what + " mask")
                bytes_untouched(mbuf, rows, c // vec(dt), what + " mask")


def fp8_qstate(qinv, dev):
    return torch.tensor([1.0 / qinv, qinv, 0.5, 448.0], dtype=f32, device=dev)


@pytest.mark.parametrize("p,c", shapes(bf), ids=["%dx%d" % s for s in shapes(bf)])
def test_bn_apply_fp8_copy_exact(cuda, p, c):
    """The fp8 copy of cn_bn_apply_ex and cn_bn_apply_q8 (bf16): the bytes are e4m3(clamp(t * qinv))
    of the fp32 activation t, amax = max |t| of the fp32 t (the rounded y's differs), qstate[0:2]
    untouched; q8 writes the same bytes with the state untouched, with y NULL and with y given."""
    for nseg in (1, 2):
        pr = apply_problem(bf, p, c, nseg, "fp8")
        rows = nseg * p
        for act in (0, 1, 2):
            t = pr.t[act]
            want, want8 = expect(t, bf), e4m3_of(t, pr.qinv)[0]
            assert torch.equal(fp8_bytes(want8.view(E4M3).double(), E4M3), want8)    # canonical codes, no NaN
            amax = t.abs().max().to(f32)
            assert amax.item() != want.double().abs().max().item() and amax.item() > 0.5
            what = "fp8 copy act %d nseg %d" % (act, nseg)
            q = fp8_qstate(pr.qinv, cuda)
            ybuf, yv = output(rows, c, bf, cuda)
            buf8, v8 = byte_output(rows, c, cuda, ld_mult=16)
            launch_apply(cuda, bf, pr, act, yv, out8=v8, qstate=q)
            same(yv, want, what)
            untouched(ybuf, rows, c, what)
            same_bytes(v8, want8, what + " bytes")
            bytes_untouched(buf8, rows, c, what + " bytes")
            same(q, torch.stack([torch.tensor(1.0 / pr.qinv), torch.tensor(pr.qinv), amax, torch.tensor(448.0)]),
                 what + " state")
            for with_y in (False, True):
                q = fp8_qstate(pr.qinv, cuda)
                ybuf, yv = output(rows, c, bf, cuda)
                buf8, v8 = byte_output(rows, c, cuda, ld_mult=16)
                launch_apply(cuda, bf, pr, act, yv if with_y else None, out8=v8, qstate=q, q8=True)
                same_bytes(v8, want8, what + " q8 bytes")
                bytes_untouched(buf8, rows, c, what + " q8 bytes")
                same(q, fp8_qstate(pr.qinv, "cpu"), what + " q8 state")
                if with_y:
                    same(yv, want, what + " q8 y")
                    untouched(ybuf, rows, c, what + " q8 y")


# ---- c. backward ------------------------------------------------------------------------------
# mode: (act given to cn_bn_bwd, residual in the forward, what the mask is taken from)
BWD_MODES = {"none": (0, False), "relu_y": (1, False), "relu_x": (3, False), "relu_bits": (4, False),
             "prelu": (2, False), "relu_y_res": (1, True), "relu_bits_res": (4, True)}


@functools.lru_cache(maxsize=None)
def bwd_problem(dt, p, c, paired=False):
    """x, dy and, per mode, the stored forward y and the exact dz, sums and dx.
    paired: rows r and r + P / 2 have equal x (and residual) and opposite dy, so both column sums
    are exactly 0 and dx = k1 * dz whatever 1 / P is (P = 2294)."""
    sd = 2000 + int(paired)
    par = params(c, 1, sd, zero_gamma=False)
    last = p // 2 - 1 if paired else p - 1
    x, xhat, pre = activations(p, c, par, sd + 5, last=last)
    dy = ints((p, c), -4, 4, sd + 6)
    res = torch.where(ints((p, c), 0, 15, sd + 7) == 0, -pre, 2 * ints((p, c), -3, 3, sd + 8))
    dy[last], res[last] = 3.0, 6.0     # the tail row counts in the sums of every channel it is unmasked in
    if paired:
        h = p // 2
        assert p == 2 * h
        x, xhat, pre, res = (torch.cat([v[:h], v[:h]]) for v in (x, xhat, pre, res))
        dy = torch.cat([dy[:h], -dy[:h]])
    k1 = par.gamma * par.invstd[0]
    pr = SimpleNamespace(par=par, x=x, xhat=xhat, pre=pre, dy=dy, res=res, p=p, k1=k1, modes={}, paired=paired)
    assert exact32(x, dy, res, xhat, pre, pre + res)
    assert dt == f32 or all(torch.equal(rne_bf16(v).double(), v) for v in (x, dy, res))
    pow2 = p & (p - 1) == 0
    for name, (act, with_res) in BWD_MODES.items():
        m = SimpleNamespace(act=act, y=None, with_res=with_res)
        if act in (1, 4):
            # the mask of the STORED y = one rounding of relu(bn(x) [+ res])
            m.y = expect((pre + res if with_res else pre).clamp(min=0.0), dt)
            m.dz = torch.where(m.y.double() > 0, dy, 0.0)     # a masked gradient is +0, whatever dy's sign
        elif act == 3:
            m.dz = torch.where(pre > 0, dy, 0.0)
        elif act == 2:
            m.dz = torch.where(pre > 0, dy, PRELU_A * dy)
        else:
            m.dz = dy
        m.dbeta, m.dgamma = m.dz.sum(0), (m.dz * xhat).sum(0)
        m.dprelu_c = (dy * pre * (pre <= 0)).sum(0) if act == 2 else None
        m.sum_bound = max(m.dz.abs().sum(0).max().item() * 4, (m.dz * xhat).abs().sum(0).max().item() * 16)
        if act == 2:
            m.sum_bound = max(m.sum_bound, (dy * pre).abs().sum(0).max().item() * 8, m.dprelu_c.abs().sum().item() * 8)
        m.has_dx = pow2 or paired
        if m.has_dx:
            m1, m2 = m.dbeta / p, m.dgamma / p
            m.m1, m.m2 = m1, m2
            m.dx = k1 * (m.dz - m1 - xhat * m2)
        pr.modes[name] = m
    return pr


def verify_bwd(pr, m):
    """The exactness conditions of one mode (the GPU test and the CPU self-check call this): sums
    below 2^24 in units of their granularity, every fp32 intermediate of dx representable in both
    association orders."""
    assert m.sum_bound < 2 ** 24
    assert exact32(m.dz, m.dz * pr.xhat, m.dbeta, m.dgamma)
    if m.act == 2:
        assert exact32(pr.dy * pr.pre, m.dprelu_c, m.dprelu_c.sum())
    if pr.paired:
        assert not m.dbeta.any() and not m.dgamma.any()
    if m.has_dx:
        prod = pr.xhat * m.m2
        assert exact32(m.m1, m.m2, prod, m.dz - m.m1, m.dz - m.m1 - prod, m.m1 + prod, m.dx)


def bwd_zero_share(pr):
    return (pr.pre == 0).double().mean().item()


def launch_bwd(dev, dt, pr, m, want_dx, want_dres, what):
    par, p, c = pr.par, pr.p, pr.x.shape[1]
    bn = K._BN(c, dev, 1)
    bn.weight, bn.bias = par.gamma.to(f32).to(dev), par.beta.to(f32).to(dev)
    stats = (par.mean[0].to(f32).to(dev), par.invstd[0].to(f32).to(dev))
    y, act = None, m.act
    if act == 1:
        y = operand(m.y.double(), dt, dev)
    elif act == 4:
        mb = mask_bytes(m.y.double(), dt)
        ybuf = torch.full((p + ROWS_PAST, mb.shape[1] + 5), 0xFF, dtype=torch.uint8)
        ybuf[:p, 3:3 + mb.shape[1]] = mb
        y = ybuf.to(dev)[:p, 3:3 + mb.shape[1]]
    dxbuf, dxv = output(p, c, dt, dev) if want_dx else (None, None)
    drbuf, drv = output(p, c, dt, dev) if want_dres else (None, None)
    dx, dgam, dbet, dpr = ops.bn_bwd(operand(pr.x, dt, dev), operand(pr.dy, dt, dev), y, stats, bn,
                                     act=1 if act == 3 else act, prelu=torch.tensor([PRELU_A], dtype=f32, device=dev),
                                     want_dx=want_dx, dx=dxv, dres=drv)
    torch.cuda.synchronize()
    same(dbet, m.dbeta.to(f32), what + " dbeta")
    same(dgam, m.dgamma.to(f32), what + " dgamma")
    if act == 2:
        same(dpr, m.dprelu_c.sum().to(f32).view(1), what + " dprelu")
    if want_dx:
        if m.has_dx:
            same(dxv, expect(m.dx, dt), what + " dx")
        untouched(dxbuf, p, c, what + " dx")
    else:
        assert dx is None
    if want_dres:
        same(drv, expect(m.dz, dt), what + " dres")
        untouched(drbuf, p, c, what + " dres")


@pytest.mark.parametrize("dt,p,c", CASES, ids=CASE_IDS)
def test_bn_bwd_exact(cuda, dt, p, c):
    """cn_bn_bwd, act 0, 1, 3, 4 and 2 (and 1 / 4 on a forward with a residual, where the mask is
    the stored y's, not x's); sums only, dx, dx + dres.  dgamma / dbeta / dprelu bitwise everywhere;
    dx bitwise at power-of-two P, and at P = 2294 on the paired inputs (zero sums) where dx = k1 dz;
    dres = dz bitwise everywhere.  act 1, 3 and 4 share one reference, zero pre-activations
    (>= 2 %) included."""
    prs = [bwd_problem(dt, p, c)] + ([bwd_problem(dt, p, c, True)] if p & (p - 1) else [])
    for pr in prs:
        assert bwd_zero_share(pr) >= MIN_ZEROS
        for name, m in pr.modes.items():
            verify_bwd(pr, m)
            what = "bwd %s%s" % (name, " paired" if pr.paired else "")
            launch_bwd(cuda, dt, pr, m, True, True, what)
            launch_bwd(cuda, dt, pr, m, True, False, what + " no dres")
            if not pr.paired:
                launch_bwd(cuda, dt, pr, m, False, False, what + " sums only")


# ---- d. backward apply from given sums --------------------------------------------------------
@functools.lru_cache(maxsize=None)
def bwd_apply_problem(dt, p, c):
    """cn_bn_bwd_apply (ReLU mask from x): sums that are integer multiples of P at power-of-two P,
    zeros otherwise."""
    pr = bwd_problem(dt, p, c)
    pow2 = p & (p - 1) == 0
    s1 = p * ints((c,), -2, 2, 3001) if pow2 else torch.zeros(c, dtype=f64)
    s2 = p * ints((c,), -2, 2, 3002) if pow2 else torch.zeros(c, dtype=f64)
    dz = torch.where(pr.pre > 0, pr.dy, 0.0)
    m1, m2 = s1 / p, s2 / p
    prod = pr.xhat * m2
    dx = pr.k1 * (dz - m1 - prod)
    assert exact32(s1, s2, m1, m2, prod, dz - m1, dz - m1 - prod, m1 + prod, dx)
    return SimpleNamespace(pr=pr, s1=s1, s2=s2, dx=dx)


@pytest.mark.parametrize("dt,p,c", CASES, ids=CASE_IDS)
def test_bn_bwd_apply_exact(cuda, dt, p, c):
    ap = bwd_apply_problem(dt, p, c)
    pr, par = ap.pr, ap.pr.par
    bn = K._BN(c, cuda, 1)
    bn.weight, bn.bias = par.gamma.to(f32).to(cuda), par.beta.to(f32).to(cuda)
    stats = (par.mean[0].to(f32).to(cuda), par.invstd[0].to(f32).to(cuda))
    dxbuf, dxv = output(p, c, dt, cuda)
    ops.bn_bwd_apply(operand(pr.x, dt, cuda), operand(pr.dy, dt, cuda), stats, bn, ap.s2.to(f32).to(cuda),
                     ap.s1.to(f32).to(cuda), out=dxv)
    torch.cuda.synchronize()
    same(dxv, expect(ap.dx, dt), "bwd_apply dx")
    untouched(dxbuf, p, c, "bwd_apply dx")
