"""Exact closed-form parity of the co-attention kernels (coatt_fused.hip, coatt_q48.hip,
coatt_flash.hip, coatt_f8.hip): inputs whose softmax weights, outputs and gradients are known in
closed form and exactly representable, so Z_a, Z_b, dVa_t and the PV product are compared
BITWISE (torch.equal on the values, after a finiteness check) and the normalisers against their
closed form within the project's own bounds.

The input family (C = 256, bf16 operands).  H is the 256 x 256 Sylvester Hadamard matrix (rows
exactly orthogonal, H[0] all ones).  One frame of hw pixels has power-of-two group sizes summing
to hw (at most 127 groups, ids 1..G), a query-side assignment gq and a key-side assignment gk (two
seeded permutations of the same ids, so a group has the same size on both sides), and

    vat[i] = H[gq[i]] - 2 H[0]                      entries -1, -3
    vb[j]  = H[gk[j]] + H[0] + r_j                  entries -2..4; r_j = +-H[m1] +- H[m2],
                                                    m1 in 128..191, m2 in 192..255: orthogonal to
                                                    every query row, makes a group's values differ
    va     = integers in -4..4                      the values of the Z_b direction
    dza, dzb: two channels per row set to +-1, the rest 0

so that S = vat vb^T is exactly -256 inside a group and -512 outside: the gap is 369 in log2
units, every out-of-group weight underflows to 0, P0 and P1 are exactly 1/|group| inside, Z_a /
Z_b are group means (bf16-exact up to |group| = 32), lse = -256 log2(e) + log2|group|, and every
real logit is negative, so a zero padding row that escaped its mask (logit 0) would take the
whole row.  For |group| <= 8, dS = P0 (dza.vb - D0) + P1 (va.dzb - D1) is bf16-exact too and
dVa_t = dS vb and P1 dzb are sums of small dyadic numbers, exact in fp32.

Why equality is asserted: the kernels' fp32 error enters as a relative perturbation of ~1e-5 on
a weight (or on Z before its final rounding), far below half a bf16 ulp (2^-9) of a value that is
itself bf16-representable; the rounding to bf16 (of P, dS, a partial row, the output) snaps back,
every accumulation of snapped values is exact in fp32, and the final cast is one
round-to-nearest-even of the exact sum.

Rows whose group has a key among the first 32 keys and rows whose group lies wholly later both
occur: the latter take the 48-row kernel (variant 5) through its redo pass, as the logit outgrows
the first-tile reference by 369.  Pairs of one launch have different seeds (a kernel that reads
the next pair's rows as keys is caught).  The expectations are group means by index_add, never an
hw x hw matrix; tests/test_cpu_coatt_exact_inputs.py proves every property above without a GPU,
and that the comparison bites (mutated references differ after bf16 rounding).
"""
import contextlib
import functools
import math
from types import SimpleNamespace

import pytest
import torch

from cosnet_amd import _native as nv
from cosnet_amd import ops

from test_gpu_exact_gemm import ints, rne_bf16

pytestmark = pytest.mark.gpu

bf = torch.bfloat16
f32 = torch.float32
f64 = torch.float64
C = 256
MAX_GROUPS = 127
L2E = math.log2(math.e)
S_IN, S_OUT = -256.0, -512.0     # the two logits: inside / outside the row's group

# (n, hw, maxg, fixed): fixed = every group of size maxg, plus the remainder
FWD_CASES = [(1, 1, 1, False), (2, 33, 4, False), (3, 97, 8, False), (2, 129, 8, False),
             (2, 193, 8, False), (1, 300, 8, False), (2, 1271, 32, False),
             (5, 3600, 32, True), (8, 3600, 32, True)]
BWD_CASES = [(1, 1, 1, False), (2, 33, 4, False), (3, 97, 8, False), (2, 129, 8, False),
             (1, 300, 8, False), (2, 500, 4, True)]
# banks of 3 frames (hw, maxg) and the frame maps of 4 pairs: not the identity, an a-frame and a
# b-frame repeat, pair 1 has ia == ib
BANK_CASES = [(97, 8), (193, 8)]
BANK_T, BANK_IA, BANK_IB = 3, [2, 0, 2, 1], [1, 0, 0, 2]
# the Gaussian cases of test_gpu_coatt_fused.py::test_flash_training_fwd_bwd_vs_fp64 whose flash
# normalisers are compared with fp64 here
GAUSS_CASES = [(1, 97), (2, 169)]
WHICH = ["both", "a_only", "b_only"]
LSE_TOL = 1e-4       # x max(1, max |lse|): the bound of the variant-vs-variant tests
LSE_TOL_F8 = 1e-3    # x max(1, max |lse|): test_gpu_coatt_f8.py's training bound


def case_id(c):
    return "n%d-hw%d-g%d%s" % (c[0], c[1], c[2], "-fixed" if c[3] else "")


# ---- generators and closed forms (CPU, fp64) ------------------------------------------------
@functools.lru_cache(None)
def hadamard():
    h = torch.ones((1, 1), dtype=f64)
    while h.shape[0] < C:
        h = torch.cat([torch.cat([h, h], 1), torch.cat([h, -h], 1)], 0)
    return h


def group_sizes(hw, maxg, seed, fixed=False):
    """Powers of two up to maxg that sum to hw, at most MAX_GROUPS of them: drawn uniformly among
    the sizes that still leave the rest coverable within the limit (fixed: always the largest)."""
    g = torch.Generator().manual_seed(seed)
    pows = [1 << k for k in range(maxg.bit_length()) if 1 << k <= maxg]
    need = lambda rem: rem // maxg + bin(rem % maxg).count("1")   # fewest groups that cover rem
    sizes, rem = [], hw
    while rem:
        ok = [s for s in pows if s <= rem and len(sizes) + 1 + need(rem - s) <= MAX_GROUPS]
        assert ok, "hw = %d needs more than %d groups of <= %d" % (hw, MAX_GROUPS, maxg)
        s = max(ok) if fixed else ok[int(torch.randint(len(ok), (1,), generator=g))]
        sizes.append(s)
        rem -= s
    assert sum(sizes) == hw and len(sizes) <= MAX_GROUPS
    return sizes


def make_frame(hw, sizes, seed):
    """One frame: both roles' group ids and operands (fp64), gradients included."""
    g = torch.Generator().manual_seed(seed)
    H = hadamard()
    G = len(sizes)
    gid = torch.repeat_interleave(torch.arange(1, G + 1), torch.tensor(sizes))
    gq = gid[torch.randperm(hw, generator=g)]
    gk = gid[torch.randperm(hw, generator=g)]
    rnd = lambda lo, hi, shape: torch.randint(lo, hi, shape, generator=g)
    sign = lambda shape: (2 * rnd(0, 2, shape) - 1).double()
    r = sign((hw, 1)) * H[rnd(128, 192, (hw,))] + sign((hw, 1)) * H[rnd(192, 256, (hw,))]
    f = SimpleNamespace(hw=hw, G=G, sizes=list(sizes), gq=gq, gk=gk)
    f.vat = H[gq] - 2 * H[0]
    f.vb = H[gk] + H[0] + r
    f.va = rnd(-4, 5, (hw, C)).double()
    for name in ("dza", "dzb"):
        d = torch.zeros((hw, C), dtype=f64)
        c1 = rnd(0, C, (hw,))
        c2 = (c1 + 1 + rnd(0, C - 1, (hw,))) % C          # a second, different channel
        rows = torch.arange(hw)
        d[rows, c1] = sign((hw,))
        d[rows, c2] = sign((hw,))
        setattr(f, name, d)
    return f


def group_stats(rows, gid, G):
    """Mean of `rows` over each group and the group sizes, indexed by group id (0 unused)."""
    tot = torch.zeros((G + 1, rows.shape[1]), dtype=f64).index_add_(0, gid, rows)
    cnt = torch.zeros((G + 1,), dtype=f64).index_add_(0, gid, torch.ones_like(gid, dtype=f64))
    return tot / cnt.clamp_min(1)[:, None], cnt


def pair_expect(fa, fb):
    """Closed form of one pair with a-role frame fa and b-role frame fb (which share their group
    sizes): Z_a, Z_b [hw, C] and the log2 normalisers [hw] of both directions, fp64."""
    assert fa.sizes == fb.sizes
    mb, cb = group_stats(fb.vb, fb.gk, fb.G)     # keys of each group
    ma, ca = group_stats(fa.va, fa.gq, fa.G)     # queries of each group
    assert torch.equal(ca, cb)
    return SimpleNamespace(za=mb[fa.gq], zb=ma[fb.gk],
                           lse_a=S_IN * L2E + torch.log2(cb[fa.gq]),
                           lse_b=S_IN * L2E + torch.log2(ca[fb.gk]))


def _stack(frames_a, frames_b):
    """The stacked operands and expectations of pairs (frames_a[p], frames_b[p])."""
    hw = frames_a[0].hw
    ex = [pair_expect(a, b) for a, b in zip(frames_a, frames_b)]
    cat = lambda xs: torch.cat(list(xs), 0)
    out = SimpleNamespace(n=len(ex), hw=hw, frames_a=frames_a, frames_b=frames_b)
    out.vat, out.va = cat(a.vat for a in frames_a), cat(a.va for a in frames_a)
    out.vb = cat(b.vb for b in frames_b)
    out.za, out.zb = cat(e.za for e in ex), cat(e.zb for e in ex)
    out.lse_a = torch.stack([e.lse_a for e in ex])          # [n, hw]
    out.lse_b = torch.stack([e.lse_b for e in ex])
    return out


@functools.lru_cache(None)
def make_case(n, hw, maxg, fixed=False):
    """n pairs, each a frame of its own (own seed, own group sizes) in both roles."""
    seed = 7919 * hw + 31 * maxg + n
    frames = [make_frame(hw, group_sizes(hw, maxg, seed + 101 * p, fixed), seed + 101 * p + 50)
              for p in range(n)]
    return _stack(frames, frames)


@functools.lru_cache(None)
def make_bank(hw, maxg):
    """BANK_T frames with common group sizes; the pairs (BANK_IA[p], BANK_IB[p]) stacked."""
    seed = 104729 + 7919 * hw + maxg
    sizes = group_sizes(hw, maxg, seed)
    frames = [make_frame(hw, sizes, seed + 101 * t + 50) for t in range(BANK_T)]
    out = _stack([frames[i] for i in BANK_IA], [frames[i] for i in BANK_IB])
    out.frames = frames
    out.bank_vat, out.bank_va, out.bank_vb = (torch.cat([getattr(f, k) for f in frames], 0)
                                              for k in ("vat", "va", "vb"))
    return out


def group_blocks(gid, G, mg):
    """Row indices of every group as a [G, mg] matrix with a validity mask (padding index 0)."""
    order = torch.argsort(gid, stable=True)
    sid = gid[order]
    cnt = torch.bincount(gid, minlength=G + 1)
    start = torch.cumsum(cnt, 0) - cnt
    pos = torch.arange(gid.shape[0]) - start[sid]
    idx = torch.zeros((G, mg), dtype=torch.long)
    mask = torch.zeros((G, mg), dtype=torch.bool)
    idx[sid - 1, pos] = order
    mask[sid - 1, pos] = True
    return idx, mask


def backward_expect(f, e, which):
    """Closed form of the backward of pair (f, f) with expectations e, group by group (blocks of
    at most max|group| x max|group|): D0, D1 [hw], dS's in-group blocks [G, mg, mg] with their row
    / column indices and mask, dVa_t = dS vb and the PV product P1 dzb [hw, C].  which: the
    gradient reaches both outputs, Z_a only or Z_b only."""
    mg = max(f.sizes)
    qi, qm = group_blocks(f.gq, f.G, mg)
    ki, km = group_blocks(f.gk, f.G, mg)
    inv = 1.0 / torch.tensor(f.sizes, dtype=f64)[:, None, None]          # P0 = P1 inside a group
    m2 = (qm[:, :, None] & km[:, None, :]).double()
    out = SimpleNamespace(qi=qi, ki=ki, m2=m2, p=inv * m2)
    out.d0 = (f.dza * e.za).sum(1)
    out.d1 = (f.dzb * e.zb).sum(1)
    x = torch.zeros((f.G, mg, mg), dtype=f64)
    vbk = f.vb[ki]                                                       # [G, mg, C]
    if which in ("both", "a_only"):
        x = x + f.dza[qi] @ vbk.transpose(1, 2) - out.d0[qi][:, :, None]
    if which in ("both", "b_only"):
        x = x + f.va[qi] @ f.dzb[ki].transpose(1, 2) - out.d1[ki][:, None, :]
    out.ds = out.p * x
    out.dvat = torch.zeros((f.hw, C), dtype=f64)
    out.dvat[qi[qm]] = (out.ds @ vbk)[qm]
    out.pv = torch.zeros((f.hw, C), dtype=f64)
    out.pv[qi[qm]] = (out.p @ f.dzb[ki])[qm]
    return out


@functools.lru_cache(None)
def make_backward(n, hw, maxg, fixed, which):
    """Stacked gradients and backward expectations of make_case(n, hw, maxg, fixed)."""
    case = make_case(n, hw, maxg, fixed)
    ex = [backward_expect(f, pair_expect(f, f), which) for f in case.frames_a]
    cat = lambda xs: torch.cat(list(xs), 0)
    out = SimpleNamespace(case=case, pairs=ex)
    out.dza, out.dzb = cat(f.dza for f in case.frames_a), cat(f.dzb for f in case.frames_a)
    out.dvat, out.pv = cat(b.dvat for b in ex), cat(b.pv for b in ex)
    out.d0 = cat(b.d0 for b in ex)                                       # [n * hw]
    out.d1 = torch.stack([b.d1 for b in ex])                             # [n, hw]
    return out


def old_dva(rows, seed):
    """The tensor the PV kernel accumulates onto: integers in +-[0, 255] (bf16-exact).  From 128
    on bf16's spacing is 1, so old + P1 dzb (multiples of 1/8) is rounded, exact ties included."""
    return ints((rows, C), -255, 255, seed)


@functools.lru_cache(None)
def gaussian_case(n, hw):
    """The operands of test_flash_training_fwd_bwd_vs_fp64 at (n, hw) -- same generator, same
    order of draws -- with Va_t = Va W^T rounded to bf16 once from fp64, and the fp64 log2
    normalisers of both directions [n, hw]."""
    g = torch.Generator().manual_seed(hw + n)
    va = (torch.randn((n * hw, C), generator=g) * 0.7).to(bf)
    vb = (torch.randn((n * hw, C), generator=g) * 0.7).to(bf)
    W = torch.randn((C, C), generator=g) * C ** -0.5
    vat = (va.double() @ W.double().t()).to(bf)
    S = vat.double().reshape(n, hw, C) @ vb.double().reshape(n, hw, C).transpose(1, 2)
    return SimpleNamespace(n=n, hw=hw, vat=vat, va=va, vb=vb, S=S,
                           lse_a=torch.logsumexp(S, 2) * L2E, lse_b=torch.logsumexp(S, 1) * L2E)


# ---- GPU side --------------------------------------------------------------------------------
@contextlib.contextmanager
def forced_variant(v):
    lib = nv.load()
    old = lib.cn_coatt_force_variant(v)
    assert old != -1
    try:
        yield
    finally:
        lib.cn_coatt_force_variant(old)


def up(x, cuda):
    """fp64 (bf16-exact) -> bf16 on the GPU."""
    return x.to(bf).to(cuda)


def operands(case, cuda):
    if not hasattr(case, "dev"):
        case.dev = tuple(up(x, cuda) for x in (case.vat, case.va, case.vb))
    return case.dev


def strided(x, cuda):
    """x as the right half of a [rows, 512] buffer whose left half is NaN (row stride 512)."""
    buf = torch.full((x.shape[0], 2 * C), float("nan"), dtype=bf)
    buf[:, C:] = x.to(bf)
    view = buf.to(cuda)[:, C:]
    assert ops.ld(view) == 2 * C and view.data_ptr() % 16 == 0
    return view


def z_buf(rows, cuda):
    return torch.full((rows, C), float("nan"), dtype=bf, device=cuda)


def lse_buf(n, hw, cuda):
    return torch.full((n, ops.hw_pad(hw)), float("nan"), dtype=f32, device=cuda)


def assert_exact(got, ref, what):
    """got (bf16, GPU) equals one RNE rounding of the fp64 closed form, element by element."""
    torch.cuda.synchronize()
    g = got.float().cpu()
    r = rne_bf16(ref).float()
    assert torch.isfinite(g).all(), (what, "not finite", int((~torch.isfinite(g)).sum()))
    bad = g != r
    assert not bad.any(), (what, "%d of %d elements differ, max |diff| %.3e, first row %d" % (
        int(bad.sum()), bad.numel(), (g - r).abs().max().item(), int(bad.any(1).nonzero()[0])))


def assert_lse(got, ref, hw, tol, what):
    """got [n, hw_pad] fp32 on the GPU: within tol x max(1, max |ref|) of ref [n, hw]; +inf behind."""
    torch.cuda.synchronize()
    g = got.cpu()
    err = (g[:, :hw].double() - ref).abs().max().item()
    bound = tol * max(1.0, ref.abs().max().item())
    print("%s: max |lse - closed form| %.3e (bound %.3e)" % (what, err, bound))
    assert err <= bound, (what, err, bound)
    assert (g[:, hw:] == float("inf")).all(), (what, "padding is not +inf")


# ---- forward ---------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", [1, 5])
@pytest.mark.parametrize("case", FWD_CASES, ids=case_id)
def test_fused_forward(cuda, case, variant):
    """ops.coatt_fused: both directions, Z_b alone (za = None), and both on channel-slice views
    with row stride 512."""
    k = make_case(*case)
    n, hw = k.n, k.hw
    vat, va, vb = operands(k, cuda)
    with forced_variant(variant):
        za, zb = ops.coatt_fused(vat, va, vb, n, hw, z_buf(n * hw, cuda), z_buf(n * hw, cuda))
        _, zb1 = ops.coatt_fused(vat, va, vb, n, hw, None, z_buf(n * hw, cuda))
        sa, sb = ops.coatt_fused(strided(k.vat, cuda), strided(k.va, cuda), strided(k.vb, cuda), n, hw,
                                 z_buf(n * hw, cuda), z_buf(n * hw, cuda))
        torch.cuda.synchronize()
    assert_exact(za, k.za, "za")
    assert_exact(zb, k.zb, "zb")
    assert_exact(zb1, k.zb, "zb with za = None")
    assert_exact(sa, k.za, "za from strided views")
    assert_exact(sb, k.zb, "zb from strided views")


@pytest.mark.parametrize("variant", [1, 5])
@pytest.mark.parametrize("hw,maxg", BANK_CASES)
def test_indexed_forward(cuda, hw, maxg, variant):
    """ops.coatt_fused_idx over a bank of 3 frames with non-identity, repeating maps."""
    k = make_bank(hw, maxg)
    p = k.n
    bank = [up(x, cuda) for x in (k.bank_vat, k.bank_va, k.bank_vb)]
    ia = torch.tensor(BANK_IA, dtype=torch.int32, device=cuda)
    ib = torch.tensor(BANK_IB, dtype=torch.int32, device=cuda)
    with forced_variant(variant):
        za, zb = ops.coatt_fused_idx(*bank, ia, ib, p, hw, z_buf(p * hw, cuda), z_buf(p * hw, cuda))
        torch.cuda.synchronize()
    assert_exact(za, k.za, "za")
    assert_exact(zb, k.zb, "zb")


@pytest.mark.parametrize("variant", [1, 5])
@pytest.mark.parametrize("case", FWD_CASES, ids=case_id)
def test_flash_forward(cuda, case, variant):
    """ops.coatt_flash_fwd: Z bitwise, the normalisers within LSE_TOL x max(1, max |lse|) of the
    closed form, +inf in their padding."""
    k = make_case(*case)
    n, hw = k.n, k.hw
    vat, va, vb = operands(k, cuda)
    za, zb = z_buf(n * hw, cuda), z_buf(n * hw, cuda)
    la, lb = lse_buf(n, hw, cuda), lse_buf(n, hw, cuda)
    with forced_variant(variant):
        ops.coatt_flash_fwd(vat, va, vb, n, hw, za, zb, la, lb)
        torch.cuda.synchronize()
    assert_exact(za, k.za, "za")
    assert_exact(zb, k.zb, "zb")
    assert_lse(la, k.lse_a, hw, LSE_TOL, "lse_a")
    assert_lse(lb, k.lse_b, hw, LSE_TOL, "lse_b")


@pytest.mark.parametrize("variant", [1, 5])
@pytest.mark.parametrize("n,hw", GAUSS_CASES)
def test_flash_forward_lse_on_gaussian_inputs(cuda, n, hw, variant):
    """The flash forward's normalisers on Gaussian operands against fp64 logsumexp, under the
    bound the variant-vs-variant tests use (an fp32 evaluation of the reference stays inside it:
    tests/test_cpu_coatt_exact_inputs.py)."""
    k = gaussian_case(n, hw)
    vat, va, vb = (x.to(cuda) for x in (k.vat, k.va, k.vb))
    la, lb = lse_buf(n, hw, cuda), lse_buf(n, hw, cuda)
    with forced_variant(variant):
        ops.coatt_flash_fwd(vat, va, vb, n, hw, z_buf(n * hw, cuda), z_buf(n * hw, cuda), la, lb)
        torch.cuda.synchronize()
    assert_lse(la, k.lse_a, hw, LSE_TOL, "lse_a")
    assert_lse(lb, k.lse_b, hw, LSE_TOL, "lse_b")


@pytest.mark.parametrize("case", FWD_CASES, ids=case_id)
def test_f8_forward(cuda, case):
    """ops.coatt_f8 (MX e4m3 operands, P in e4m3: all exact here): Z bitwise, the normalisers
    within LSE_TOL_F8 x max(1, max |lse|)."""
    k = make_case(*case)
    n, hw = k.n, k.hw
    vat, va, vb = operands(k, cuda)
    za, zb = z_buf(n * hw, cuda), z_buf(n * hw, cuda)
    la, lb = lse_buf(n, hw, cuda), lse_buf(n, hw, cuda)
    ops.coatt_f8(vat, va, vb, n, hw, za, zb, la, lb)
    assert_exact(za, k.za, "za")
    assert_exact(zb, k.zb, "zb")
    assert_lse(la, k.lse_a, hw, LSE_TOL_F8, "lse_a")
    assert_lse(lb, k.lse_b, hw, LSE_TOL_F8, "lse_b")


@pytest.mark.parametrize("case", FWD_CASES, ids=case_id)
def test_f8_training_forward(cuda, case):
    """ops.coatt_f8_train: the decoded operands equal the inputs, Z bitwise, the normalisers
    within test_gpu_coatt_f8.py's training bound."""
    k = make_case(*case)
    n, hw = k.n, k.hw
    vat, va, vb = operands(k, cuda)
    za, zb = z_buf(n * hw, cuda), z_buf(n * hw, cuda)
    la, lb = lse_buf(n, hw, cuda), lse_buf(n, hw, cuda)
    qvat, qva, qvb = ops.coatt_f8_train(vat, va, vb, n, hw, za, zb, la, lb)
    torch.cuda.synchronize()
    assert torch.equal(qvat, vat) and torch.equal(qva, va) and torch.equal(qvb, vb)
    assert_exact(za, k.za, "za")
    assert_exact(zb, k.zb, "zb")
    assert_lse(la, k.lse_a, hw, LSE_TOL_F8, "lse_a")
    assert_lse(lb, k.lse_b, hw, LSE_TOL_F8, "lse_b")


@pytest.mark.parametrize("hw,maxg", BANK_CASES)
def test_f8_indexed_forward(cuda, hw, maxg):
    """ops.coatt_f8_idx over ops.coatt_f8_bank: the bank's second matrix serves as keys and
    values, so it holds the frames' vb."""
    k = make_bank(hw, maxg)
    p = k.n
    img = ops.coatt_f8_bank(up(k.bank_vat, cuda), up(k.bank_vb, cuda), BANK_T, hw)
    ia = torch.tensor(BANK_IA, dtype=torch.int32, device=cuda)
    ib = torch.tensor(BANK_IB, dtype=torch.int32, device=cuda)
    za, _ = ops.coatt_f8_idx(img, None, BANK_T, ia, ib, p, hw, z_buf(p * hw, cuda))
    assert_exact(za, k.za, "za")


# ---- backward --------------------------------------------------------------------------------
def flash_forward(k, cuda):
    """The training forward under the variant in force: (za, zb, lse_a, lse_b) on the GPU."""
    vat, va, vb = operands(k, cuda)
    za, zb = z_buf(k.n * k.hw, cuda), z_buf(k.n * k.hw, cuda)
    la, lb = lse_buf(k.n, k.hw, cuda), lse_buf(k.n, k.hw, cuda)
    ops.coatt_flash_fwd(vat, va, vb, k.n, k.hw, za, zb, la, lb)
    return za, zb, la, lb


def gradients(b, which, cuda):
    dza = up(b.dza, cuda) if which in ("both", "a_only") else None
    dzb = up(b.dzb, cuda) if which in ("both", "b_only") else None
    return dza, dzb


@pytest.mark.parametrize("variant", [1, 5])
@pytest.mark.parametrize("which", WHICH)
@pytest.mark.parametrize("case", BWD_CASES, ids=case_id)
def test_dvat_through_the_product_chain(cuda, case, which, variant):
    """ops.coatt_flash_fwd then ops.coatt_flash_bwd, so that the normalisers, D0 and D1 are the
    ones training uses: dVa_t is one RNE rounding of the closed form."""
    b = make_backward(*case, which)
    k = b.case
    vat, va, vb = operands(k, cuda)
    dza, dzb = gradients(b, which, cuda)
    with forced_variant(variant):
        za, zb, la, lb = flash_forward(k, cuda)
        dvat = ops.coatt_flash_bwd(vat, va, vb, None, za, zb, la, lb, dza, dzb, k.n, k.hw)
        torch.cuda.synchronize()
    assert_exact(dvat, b.dvat, "dVa_t")


@pytest.mark.parametrize("variant", [1, 5])
@pytest.mark.parametrize("accumulate", [False, True])
@pytest.mark.parametrize("case", BWD_CASES, ids=case_id)
def test_pv_kernel(cuda, case, accumulate, variant):
    """cn_coatt_flash_pv_ws through ops.coatt_flash_bwd with `dva` given, plain (over NaN) and
    accumulating onto seeded integers: rne_bf16(old + P1 dzb)."""
    b = make_backward(*case, "b_only")
    k = b.case
    vat, va, vb = operands(k, cuda)
    old = old_dva(k.n * k.hw, 17 + k.hw) if accumulate else torch.zeros((k.n * k.hw, C), dtype=f64)
    dva = up(old, cuda) if accumulate else z_buf(k.n * k.hw, cuda)
    with forced_variant(variant):
        za, zb, la, lb = flash_forward(k, cuda)
        ops.coatt_flash_bwd(vat, va, vb, None, za, zb, la, lb, None, up(b.dzb, cuda), k.n, k.hw, dva=dva,
                            dva_accumulate=accumulate)
        torch.cuda.synchronize()
    assert_exact(dva, old + b.pv, "dva")


@pytest.mark.parametrize("which", ["both", "b_only"])
@pytest.mark.parametrize("case", BWD_CASES, ids=case_id)
def test_dvat_ignores_d1_padding(cuda, case, which):
    """cn_coatt_flash_dvat_ws called directly with D0 / D1 from the closed form (exact in fp32)
    and D1's padding ([n, hw_pad], entries past hw) set to NaN: the kernel zeroes the padding it
    reads, so the output is the closed form all the same."""
    b = make_backward(*case, which)
    k = b.case
    n, hw, hwp = k.n, k.hw, ops.hw_pad(k.hw)
    vat, va, vb = operands(k, cuda)
    dza, dzb = gradients(b, which, cuda)
    _, _, la, lb = flash_forward(k, cuda)
    d0 = b.d0.to(f32).to(cuda)
    d1 = torch.full((n, hwp), float("nan"), dtype=f32)
    d1[:, :hw] = b.d1.to(f32)
    d1 = d1.to(cuda)
    dvat = z_buf(n * hw, cuda)
    nws = int(nv.query("cn_coatt_flash_bwd_workspace_bytes", n, hw))
    ws = torch.empty((max(nws, 16) // 4,), dtype=f32, device=cuda)
    nv.call("cn_coatt_flash_dvat_ws", vat.data_ptr(), ops.ld(vat), va.data_ptr(), ops.ld(va),
            nv.ptr(dza), C, vb.data_ptr(), ops.ld(vb), dzb.data_ptr(), ops.ld(dzb), la.data_ptr(),
            d0.data_ptr() if dza is not None else None, lb.data_ptr(), d1.data_ptr(), n, hw, C,
            dvat.data_ptr(), ops.ld(dvat), 0, ws.data_ptr(), nws, nv.stream())
    assert_exact(dvat, b.dvat, "dVa_t")
