"""The input family of tests/test_gpu_coatt_exact.py, checked without a GPU: for every case of that
file the generators' outputs must have the properties its bitwise comparisons rest on -- operands
that survive bf16 and e4m3 (and the MX block scalings) unchanged, logits of exactly -256 inside a
group and -512 outside, weights 1/|group|, closed-form outputs, normalisers and gradients that
are exactly representable and agree with a dense fp64 softmax -- and the comparison must bite:
dense fp64 references mutated the way a kernel goes wrong (an unmasked padding key, a dropped
key, a key of the next pair, a wrong merge weight) differ from the closed form after the bf16
rounding."""
import pytest
import torch

import test_gpu_coatt_exact as X
import test_gpu_coatt_f8 as F8
from test_gpu_exact_gemm import is_tie

f64 = torch.float64
DENSE_HW = 300     # dense fp64 references for every pair up to here, beyond for the first pair only

ALL_FWD = sorted(set(X.FWD_CASES) | set(X.BWD_CASES))


def rt(x, dtype):
    return x.to(dtype).double()


def dense(fa, fb):
    """S, P0 (softmax over keys, rows) and P1 (softmax over queries, columns) in fp64."""
    S = fa.vat @ fb.vb.t()
    return S, torch.softmax(S, 1), torch.softmax(S, 0)


def check_frame(f, maxg):
    hw = f.hw
    assert f.G == len(f.sizes) <= X.MAX_GROUPS and sum(f.sizes) == hw
    assert all(s & (s - 1) == 0 and 1 <= s <= maxg for s in f.sizes)
    cq = torch.bincount(f.gq, minlength=f.G + 1)
    ck = torch.bincount(f.gk, minlength=f.G + 1)
    assert cq[0] == 0 and torch.equal(cq, ck) and cq[1:].tolist() == f.sizes
    assert 1 <= int(f.gq.min()) and int(f.gq.max()) == f.G
    # value ranges and formats
    assert set(f.vat.unique().tolist()) <= {-1.0, -3.0}
    assert f.vb.min() >= -2 and f.vb.max() <= 4 and torch.equal(f.vb, f.vb.round())
    assert f.va.min() >= -4 and f.va.max() <= 4 and torch.equal(f.va, f.va.round())
    for d in (f.dza, f.dzb):
        assert ((d != 0).sum(1) == 2).all() and set(d.unique().tolist()) <= {-1.0, 0.0, 1.0}
    for x in (f.vat, f.va, f.vb, f.dza, f.dzb):
        assert torch.equal(rt(x, torch.bfloat16), x) and torch.equal(rt(x, torch.float8_e4m3fn), x)
    # the MX block scalings of the fp8 kernels (the emulations of test_gpu_coatt_f8.py)
    for x in (f.vat, f.vb):
        assert torch.equal(F8.mx_rows(x), x)
    for x in (f.va, f.vb):
        assert torch.equal(F8.mx_vt(x, 1, hw), x)
    assert torch.equal(F8.mx_blk(f.vb, 1, hw), f.vb)
    # the value rows of one group are not all alike (r_j differs)
    if max(f.sizes) > 1:
        big = int(torch.tensor(f.sizes).argmax()) + 1
        assert f.vb[f.gk == big].unique(dim=0).shape[0] > 1


def check_pair_dense(fa, fb, e):
    S, P0, P1 = dense(fa, fb)
    same = fa.gq[:, None] == fb.gk[None, :]
    assert torch.equal(S, torch.where(same, X.S_IN, X.S_OUT).double())
    assert (S < 0).all()
    size = torch.tensor([0] + fa.sizes, dtype=f64)
    w = same.double() / size[fa.gq][:, None]
    # the closed-form weights are powers of two; fp64 softmax agrees with them to 1e-12
    assert torch.equal(torch.log2(w[same]), torch.log2(w[same]).round())
    assert (P0 - w).abs().max() <= 1e-12 and (P1 - w).abs().max() <= 1e-12
    assert (P0 @ fb.vb - e.za).abs().max() <= 1e-12
    assert (P1.t() @ fa.va - e.zb).abs().max() <= 1e-12
    assert (torch.logsumexp(S, 1) * X.L2E - e.lse_a).abs().max() <= 1e-9
    assert (torch.logsumexp(S, 0) * X.L2E - e.lse_b).abs().max() <= 1e-9
    # out-of-group weights underflow: the gap is 369 in log2 units, fp32's smallest is 2^-149
    assert (X.S_IN - X.S_OUT) * X.L2E > 149 + 126


def check_expectation(k):
    """Closed-form outputs of a stacked case: bf16-exact, and the gap of the normalisers."""
    for z in (k.za, k.zb):
        assert torch.isfinite(z).all() and torch.equal(rt(z, torch.bfloat16), z)
    for lse in (k.lse_a, k.lse_b):
        g = lse - X.S_IN * X.L2E                    # log2 |group|
        assert torch.equal(g, g.round()) and g.min() >= 0 and g.max() <= 5


def row_kinds(f):
    """Rows whose group has a key among the first 32 keys, and the others."""
    early = torch.isin(f.gq, f.gk[:32])
    return int(early.sum()), int((~early).sum())


@pytest.mark.parametrize("case", ALL_FWD, ids=X.case_id)
def test_forward_cases(case):
    n, hw, maxg, fixed = case
    k = X.make_case(*case)
    assert k.n == n and k.hw == hw and k.vat.shape == (n * hw, X.C)
    for p, f in enumerate(k.frames_a):
        check_frame(f, maxg)
        if fixed:
            assert f.sizes[:hw // maxg] == [maxg] * (hw // maxg)
        if hw > 64:   # both kinds of rows: with and without a key of theirs in the first key tile
            early, later = row_kinds(f)
            assert early > 0 and later > 0, (early, later)
        if hw <= DENSE_HW or p == 0:
            check_pair_dense(f, f, X.pair_expect(f, f))
    # pairs of one launch differ
    for a, b in zip(k.frames_a, k.frames_a[1:]):
        assert not torch.equal(a.gk, b.gk) and not torch.equal(a.vb, b.vb)
    check_expectation(k)
    print("%s: groups %s, rows with / without an early key (pair 0): %s" % (
        X.case_id(case), [f.G for f in k.frames_a], row_kinds(k.frames_a[0])))


@pytest.mark.parametrize("hw,maxg", X.BANK_CASES)
def test_bank_cases(hw, maxg):
    k = X.make_bank(hw, maxg)
    assert len(k.frames) == X.BANK_T == 3 and k.n == len(X.BANK_IA) == len(X.BANK_IB)
    assert X.BANK_IA != list(range(k.n)) and X.BANK_IB != list(range(k.n))
    assert len(set(X.BANK_IA)) < k.n and len(set(X.BANK_IB)) < k.n          # frames repeat
    assert max(X.BANK_IA + X.BANK_IB) < X.BANK_T
    for f in k.frames:
        check_frame(f, maxg)
        assert f.sizes == k.frames[0].sizes
    for a, b in zip(k.frames, k.frames[1:]):
        assert not torch.equal(a.gq, b.gq) and not torch.equal(a.gk, b.gk) and not torch.equal(a.vb, b.vb)
    for fa, fb in zip(k.frames_a, k.frames_b):
        check_pair_dense(fa, fb, X.pair_expect(fa, fb))
    check_expectation(k)
    assert k.bank_vat.shape == (X.BANK_T * hw, X.C)


@pytest.mark.parametrize("which", X.WHICH)
@pytest.mark.parametrize("case", X.BWD_CASES, ids=X.case_id)
def test_backward_cases(case, which):
    n, hw, maxg, fixed = case
    assert maxg <= 8
    b = X.make_backward(*case, which)
    for f, e in zip(b.case.frames_a, b.pairs):
        ex = X.pair_expect(f, f)
        S, P0, P1 = dense(f, f)
        d0, d1 = (f.dza * ex.za).sum(1), (f.dzb * ex.zb).sum(1)
        assert torch.equal(d0, e.d0) and torch.equal(d1, e.d1)
        ds = torch.zeros_like(S)
        if which in ("both", "a_only"):
            ds = ds + P0 * (f.dza @ f.vb.t() - d0[:, None])
        if which in ("both", "b_only"):
            ds = ds + P1 * (f.va @ f.dzb.t() - d1[None, :])
        # the group blocks are dS: the dense fp64 one is zero outside them and agrees inside
        blocks = torch.zeros_like(S)
        qi, ki = e.qi[:, :, None].expand_as(e.ds), e.ki[:, None, :].expand_as(e.ds)
        on = e.m2.bool()
        blocks[qi[on], ki[on]] = e.ds[on]
        assert (ds - blocks).abs().max() <= 1e-11
        assert (ds @ f.vb - e.dvat).abs().max() <= 1e-10
        assert (P1 @ f.dzb - e.pv).abs().max() <= 1e-11
        # exactly representable: D0, D1, dVa_t and the PV product in fp32, dS in bf16
        for x in (e.d0, e.d1, e.dvat, e.pv):
            assert torch.equal(rt(x, torch.float32), x)
        assert torch.equal(rt(e.ds, torch.bfloat16), e.ds)
        assert torch.equal(rt(e.p, torch.bfloat16), e.p)
        # ... with room to spare: every term is a multiple of 2^-8 below 2^12, so any order of
        # summation is exact in fp32
        for x in (e.ds, e.dvat, e.pv):
            assert torch.equal(x * 256, (x * 256).round()) and x.abs().max() < 4096
    if hw > 1:
        assert b.dvat.abs().max() > 0 and b.pv.abs().max() > 0
    old = X.old_dva(n * hw, 17 + hw)
    assert torch.equal(rt(old, torch.bfloat16), old) and old.abs().max() <= 255
    tot = old + b.pv
    assert torch.equal(rt(tot, torch.float32), tot)
    if hw >= 33:   # the accumulation rounds, and some roundings are exact ties
        assert (rt(tot, torch.bfloat16) != tot).any() and is_tie(tot).any()


# ---- the comparison bites --------------------------------------------------------------------
def z_of(S, vb, va):
    return torch.softmax(S, 1) @ vb, torch.softmax(S, 0).t() @ va


def mutants(f, nxt):
    """{name: (za, zb)} of dense fp64 references that go wrong the way a kernel could."""
    hw = f.hw
    S = f.vat @ f.vb.t()
    out = {}
    pad = -hw % 32
    if pad:   # padding up to the next multiple of 32 left unmasked: zero rows, logit 0
        Sp = torch.zeros((hw + pad, hw + pad), dtype=f64)
        Sp[:hw, :hw] = S
        zero = torch.zeros((pad, X.C), dtype=f64)
        za, _ = z_of(Sp[:hw], torch.cat([f.vb, zero]), f.va)
        _, zb = z_of(Sp[:, :hw], f.vb, torch.cat([f.va, zero]))
        out["unmasked padding"] = (za, zb)
    # the last key (for Z_b: the last query) dropped
    za, _ = z_of(S[:, :-1], f.vb[:-1], f.va)
    _, zb = z_of(S[:-1], f.vb, f.va[:-1])
    out["last key dropped"] = (za, zb)
    if nxt is not None:   # the first key (query) of the next pair included
        za, _ = z_of(torch.cat([S, f.vat @ nxt.vb[:1].t()], 1), torch.cat([f.vb, nxt.vb[:1]]), f.va)
        _, zb = z_of(torch.cat([S, nxt.vat[:1] @ f.vb.t()], 0), f.vb, torch.cat([f.va, nxt.va[:1]]))
        out["next pair's first key"] = (za, zb)
    # two key splits folded with the first one's weight doubled: for the un-normalised partial
    # O and its row sum alike (a wrong common factor), or for O alone
    h = (hw + 1) // 2
    for name, wl in (("split weighted by 2", 2.0), ("split's O weighted by 2", 1.0)):
        if wl == 2.0 and hw == 1:
            continue   # one key, one split: a common factor cancels
        pa = torch.exp(S - S.max(1, keepdim=True).values)
        za = (2 * pa[:, :h] @ f.vb[:h] + pa[:, h:] @ f.vb[h:]) / \
            (wl * pa[:, :h].sum(1) + pa[:, h:].sum(1))[:, None]
        pb = torch.exp(S - S.max(0, keepdim=True).values).t()             # [key, query]
        zb = (2 * pb[:, :h] @ f.va[:h] + pb[:, h:] @ f.va[h:]) / \
            (wl * pb[:, :h].sum(1) + pb[:, h:].sum(1))[:, None]
        out[name] = (za, zb)
    return out


@pytest.mark.parametrize("case", [c for c in ALL_FWD if c[1] <= DENSE_HW], ids=X.case_id)
def test_mutated_references_differ_after_rounding(case):
    n, hw, maxg, fixed = case
    k = X.make_case(*case)
    seen = set()
    for p, f in enumerate(k.frames_a):
        e = X.pair_expect(f, f)
        # the unmutated dense reference does round to the closed form
        za, zb = z_of(f.vat @ f.vb.t(), f.vb, f.va)
        assert torch.equal(X.rne_bf16(za), X.rne_bf16(e.za)) and torch.equal(X.rne_bf16(zb), X.rne_bf16(e.zb))
        nxt = k.frames_a[p + 1] if p + 1 < n else None
        for name, (za, zb) in mutants(f, nxt).items():
            seen.add(name)
            da = int((X.rne_bf16(za) != X.rne_bf16(e.za)).sum())
            db = int((X.rne_bf16(zb) != X.rne_bf16(e.zb)).sum())
            print("%s pair %d, %s: %d elements of Z_a and %d of Z_b differ" % (X.case_id(case), p, name, da, db))
            assert da > 0 and db > 0, (name, p, da, db)
    want = {"last key dropped", "split's O weighted by 2"}
    if hw % 32:
        want.add("unmasked padding")
    if n > 1:
        want.add("next pair's first key")
    if hw > 1:
        want.add("split weighted by 2")
    assert seen == want


# ---- the Gaussian normaliser check -----------------------------------------------------------
@pytest.mark.parametrize("n,hw", X.GAUSS_CASES)
def test_fp32_reference_meets_the_lse_bound(n, hw):
    """An fp32 evaluation of the log2 normalisers (fp32 S, fp32 logsumexp) stays well inside
    LSE_TOL x max(1, max |lse|) of the fp64 reference on the Gaussian operands, so the bound
    asks nothing of the kernel that fp32 arithmetic cannot give."""
    k = X.gaussian_case(n, hw)
    S32 = k.vat.float().reshape(n, hw, X.C) @ k.vb.float().reshape(n, hw, X.C).transpose(1, 2)
    for dim, ref in ((2, k.lse_a), (1, k.lse_b)):
        got = torch.logsumexp(S32, dim) * torch.tensor(X.L2E, dtype=torch.float32)
        err = (got.double() - ref).abs().max().item()
        bound = X.LSE_TOL * max(1.0, ref.abs().max().item())
        print("n=%d hw=%d dim %d: fp32 lse error %.3e, bound %.3e, max |lse| %.1f" % (
            n, hw, dim, err, bound, ref.abs().max().item()))
        assert err <= bound / 4, (err, bound)
