"""The input families of tests/test_gpu_bn_exact.py, checked without a GPU: for every case of that
file the inputs and references are built here and must meet the conditions its bitwise comparisons
rest on -- fp32 evaluation in two summation orders and two association orders equals fp64, the
margin condition of the statistics, the shares of exact bf16 ties, zero pre-activations, e4m3
midpoints and saturated values, and the coverage table of launch layouts -- and the comparison
must bite: references mutated the way a kernel goes wrong differ after the rounding."""
import torch

import test_gpu_bn_exact as B
import test_gpu_exact_gemm as E

bf, f32, f64 = B.bf, B.f32, B.f64
TABLE = []    # (share name, case, value), printed by the last test (pytest -s)


def name_of(dt, p, c):
    return "%s %dx%d" % ("bf16" if dt == bf else "fp32", p, c)


def differs(a, b, dt):
    """The two references differ after the rounding to dt."""
    return not torch.equal(B.expect(a, dt), B.expect(b, dt))


def trunc_bf16(ref):
    """fp32 -> bf16 by dropping the low 16 bits."""
    return (ref.to(f32).contiguous().view(torch.int32) & -65536).view(f32).to(bf)


def sum32(terms, how):
    """Column sums of `terms` [P, C] accumulated in fp32: row after row forwards, backwards, and
    pairwise (torch's own reduction)."""
    t = terms.to(f32)
    if how == "pairwise":
        return t.sum(0).double()
    acc = torch.zeros(t.shape[1], dtype=f32)
    for r in (range(t.shape[0]) if how == "forward" else reversed(range(t.shape[0]))):
        acc = acc + t[r]
    return acc.double()


def test_layout_coverage():
    """Every launch layout the issue names is reached by some shape of the list."""
    cov = B.coverage()
    for name in B.COVERED:
        assert cov.get(name), name
        TABLE.append(("layout " + name, ", ".join(name_of(*k) for k in cov[name][:4]), len(cov[name])))
    # the named examples: C = 40 in bf16 is 5 chunk columns x 51 rows with one idle thread and
    # six partial sums a column; C = 320 at P = 2294 has more than 32 splits and, in bf16, a
    # reduction grid whose last column block is partial and an apply block with 16 idle threads
    assert B.layout(40, bf, True) == (5, 5, 51) and 256 - 5 * 51 == 1 and 256 // 40 == 6
    t = B.launch_table(bf, 2294, 320)
    assert t.stat_splits == 36 and t.bwd_splits == 72 and t.partial_col_block_red
    assert B.layout(320, bf, False) == (40, 40, 6) and 256 - 40 * 6 == 16
    assert B.launch_table(bf, 64, 2560).partial_col_block_apply
    assert B.launch_table(f32, 64, 2560).partial_col_block_apply
    assert tuple(B.TUNING) == (1024, 8, 2048, 4, 512, 4, 2048, 4)


def test_statistics_cases():
    """Sums below 2^24, the margin condition in every channel, a constant channel and one that
    differs from a constant in its last row; a dropped row, a doubled last row, the biased variance
    and swapped segments all move a float32 statistic."""
    for dt, p, c in B.CASES:
        nseg = B.STATS_NSEG[p]
        pr = B.stats_problem(dt, p, c, nseg)
        assert pr.ok and pr.bound < 2 ** 24
        x = pr.x
        assert torch.equal(x[:, :, 0], x[:, :1, 0].expand(nseg, p)) and (x[:, :-1, 1] == x[:, :1, 1]).all()
        assert (x[:, -1, 1] != x[:, 0, 1]).all()
        eps = E.BN_EPS32
        assert torch.equal(pr.invstd.view(nseg, c)[:, 0], torch.full((nseg,), 1 / eps ** 0.5, dtype=f64).to(f32))
        # against torch's own fp64 statistics (a check of the reference, not of the kernel)
        assert torch.allclose(pr.mean.view(nseg, c).double(), x.mean(1), rtol=1e-6, atol=1e-6)
        assert torch.allclose(pr.invstd.view(nseg, c).double(), (x.var(1, unbiased=False) + eps).rsqrt(), rtol=1e-6)
        m = E.BN_MOMENTUM32

        def running(segs, unbiased=True, cnt=p):
            rm, rv = pr.rm0.clone(), pr.rv0.clone()
            for s in segs:
                rm = ((1 - m) * rm + m * s.mean(0)).to(f32).double()
                var = s.var(0, unbiased=False) * (cnt / (cnt - 1) if unbiased else 1.0)
                rv = ((1 - m) * rv + m * var).to(f32).double()
            return rm.to(f32), rv.to(f32)

        rm, rv = running(list(x))
        # the plain fp64 chain reproduces the reference but for a last-bit rounding here and there
        assert (rm != pr.running_mean).double().mean() <= 0.01 and (rv != pr.running_var).double().mean() <= 0.01
        varying = torch.arange(c) >= 2
        if p > 2:
            dropped = B.stats_of(x[:, :-1], pr.rm0, pr.rv0)
            doubled = B.stats_of(torch.cat([x, x[:, -1:]], 1), pr.rm0, pr.rv0)
            for mut in (dropped, doubled):
                moved = (mut.mean != pr.mean) | (mut.invstd != pr.invstd)
                assert moved.view(nseg, c)[:, varying].double().mean() > 0.9, name_of(dt, p, c)
                assert moved.view(nseg, c)[:, 1].all()
        assert (running(list(x), unbiased=False)[1] != rv)[varying].all()
        if nseg > 1:
            swapped = running([x[1], x[0]] + list(x[2:]))
            assert (swapped[0] != rm).double().mean() > 0.9 and (swapped[1] != rv)[varying].double().mean() > 0.5


def test_apply_cases():
    """Exact operands and activations; tie, zero, midpoint and saturation shares; truncation, a
    residual added after the rounding, a `>= 0` mask, and fp8 bytes / amax taken from the rounded
    y all differ from the reference."""
    for dt, p, c in B.CASES:
        for nseg in (1, 2):
            for form in B.FORMS:
                pr = B.apply_problem(dt, p, c, nseg, form)
                case = "%s %s nseg %d" % (name_of(dt, p, c), form, nseg)
                zeros = B.zero_share(pr)
                assert zeros >= B.MIN_ZEROS, (case, zeros)
                TABLE.append(("apply zero share", case, zeros))
                if form == "res":
                    assert ((pr.res == -pr.pre) & (pr.pre != 0)).any()       # zeros reached as +x - x
                if form == "xr":
                    ch = torch.arange(c) % 8 == B.CANCEL
                    assert (pr.sum[:, ch] == 0).all() and (pr.pre[:, ch] != 0).any()
                # fp32 evaluation as the kernel's: sc = gamma * invstd, sf = beta - mean * sc, t = x * sc + sf
                par = pr.par
                sc = (par.gamma.to(f32) * par.invstd.to(f32))
                sf = par.beta.to(f32) - par.mean.to(f32) * sc
                t32 = pr.x.to(f32).view(nseg, p, c) * sc[:, None, :] + sf[:, None, :]
                assert torch.equal(t32.double().view(nseg * p, c), pr.pre)
                for act in (0, 1, 2):
                    t = pr.t[act]
                    mask_ge = B.mask_bytes((B.expect(t, dt).double() >= 0).double(), dt)
                    assert not torch.equal(mask_ge, B.mask_bytes(B.expect(t, dt).double(), dt)), case
                if form == "plain" or dt == f32:
                    continue
                ties = E.is_tie(pr.sum).double().mean().item()
                assert ties >= E.MIN_TIES, (case, ties)
                TABLE.append(("apply tie share", case, ties))
                for act in (0, 1, 2):
                    t = pr.t[act]
                    assert not torch.equal(trunc_bf16(t), E.rne_bf16(t)), case
                    assert differs(B.late_add(pr, act), t, dt), case      # first BN rounded, then the add
    for p, c in B.shapes(bf):
        for nseg in (1, 2):
            pr = B.apply_problem(bf, p, c, nseg, "fp8")
            case = "%s fp8 nseg %d" % (name_of(bf, p, c), nseg)
            for act in (0, 1, 2):
                t = pr.t[act]
                code, v = B.e4m3_of(t, pr.qinv)
                assert torch.equal(B.fp8_bytes(code.view(B.E4M3).double(), B.E4M3), code)
                mid, sat = B.e4m3_midpoint(v).double().mean().item(), (v.abs() == 448).double().mean().item()
                y = E.rne_bf16(t).double()
                assert not torch.equal(B.e4m3_of(y, pr.qinv)[0], code), case          # bytes of the rounded y
                assert y.abs().max().item() != t.abs().max().item(), case            # amax of the rounded y
                if p * c * nseg >= 512:
                    assert mid >= 0.02 and sat >= 0.02, (case, mid, sat)
                if act == 1:
                    TABLE.append(("fp8 midpoint share", case, mid))
                    TABLE.append(("fp8 saturation share", case, sat))


def test_backward_cases():
    """Sums and dx exact in fp32 whatever the order (two summation orders against fp64, two
    association orders of dx); zero pre-activations; dx's tie share; a `>= 0` mask, the mask taken
    from x under a residual, a dropped tail row and dres = dy all differ from the reference."""
    for dt, p, c in B.CASES:
        prs = [B.bwd_problem(dt, p, c)] + ([B.bwd_problem(dt, p, c, True)] if p & (p - 1) else [])
        for pr in prs:
            case = name_of(dt, p, c) + (" paired" if pr.paired else "")
            zeros = B.bwd_zero_share(pr)
            assert zeros >= B.MIN_ZEROS, (case, zeros)
            TABLE.append(("bwd zero share", case, zeros))
            for name, m in pr.modes.items():
                B.verify_bwd(pr, m)
                if p * c <= 64 * 320:
                    for how in ("forward", "backward", "pairwise"):
                        assert torch.equal(sum32(m.dz, how), m.dbeta)
                        assert torch.equal(sum32(m.dz * pr.xhat, how), m.dgamma)
                else:
                    assert torch.equal(sum32(m.dz, "pairwise"), m.dbeta)
                    assert torch.equal(sum32(m.dz * pr.xhat, "pairwise"), m.dgamma)
                    assert torch.equal(sum32(m.dz.flip(0), "pairwise"), m.dbeta)
                    assert torch.equal(sum32((m.dz * pr.xhat).flip(0), "pairwise"), m.dgamma)
                if not pr.paired and p >= 64:
                    assert m.dbeta.any() and m.dgamma.any()
                    # a tail row dropped from the sums
                    assert not torch.equal(m.dz[:-1].sum(0).to(f32), m.dbeta.to(f32))
                if m.has_dx:
                    k1, dz, xh = pr.k1.to(f32), m.dz.to(f32), pr.xhat.to(f32)
                    m1 = m.dbeta.to(f32) * (1.0 / p if p & (p - 1) == 0 else 0.0)
                    m2 = m.dgamma.to(f32) * (1.0 / p if p & (p - 1) == 0 else 0.0)
                    a = k1 * ((dz - m1) - xh * m2)
                    b = k1 * (dz - (m1 + xh * m2))
                    assert torch.equal(a.double(), m.dx) and torch.equal(b.double(), m.dx), case
                    if dt == bf and not pr.paired:
                        ties = E.is_tie(m.dx).double().mean().item()
                        TABLE.append(("bwd dx tie share (%s)" % name, case, ties))
                        if p >= 64:
                            assert ties > 0, case
                            assert not torch.equal(trunc_bf16(m.dx), E.rne_bf16(m.dx))
                # dres = dy instead of dz
                if m.act != 0:
                    assert differs(pr.dy, m.dz, dt), case
            # `>= 0` instead of `> 0`, and the mask from x where a residual was added
            for name in ("relu_y", "relu_x", "relu_bits"):
                assert torch.equal(pr.modes[name].dz, pr.modes["relu_y"].dz)
            ge = torch.where(pr.pre >= 0, pr.dy, 0.0)
            assert differs(ge, pr.modes["relu_y"].dz, dt), case
            assert differs(pr.modes["relu_y"].dz, pr.modes["relu_y_res"].dz, dt), case
            if not pr.paired and p >= 64:      # (the paired sums are 0 under any mask of x)
                assert differs(ge.sum(0), pr.modes["relu_y"].dbeta, f32), case
                assert differs(pr.modes["relu_y"].dbeta, pr.modes["relu_y_res"].dbeta, f32), case
            pre_ge = torch.where(pr.pre >= 0, 1.0, B.PRELU_A) * pr.dy
            assert differs(pre_ge, pr.modes["prelu"].dz, dt), case
        B.bwd_apply_problem(dt, p, c)


def test_epilogue_statistics_cases():
    """The conv-epilogue statistics of test_gpu_exact_gemm.py that are compared bitwise: the
    per-tile shifted sums stay below 2^24 and the margin condition holds in every channel."""
    n_exact = 0
    for case in E.BN_CASES:
        n, cin, h, w, cout, k, s, p, d, nseg = case
        out = E.conv_problem((nseg * n,) + case[1:9], E.REPR, 3, False).outs["fwd"]
        ref = E.tile_stats_reference(out.ref, n, nseg, cout)
        assert ref is not None, case
        n_exact += ref is not None
    assert n_exact >= 2


def test_print_the_share_table():
    """pytest -s: the measured shares, minimum and maximum per kind."""
    if not TABLE:      # run on its own
        test_layout_coverage(), test_apply_cases(), test_backward_cases()
    kinds = {}
    for kind, case, val in TABLE:
        kinds.setdefault(kind, []).append((val, case))
    for kind, vals in kinds.items():
        lo, hi = min(vals), max(vals)
        if kind.startswith("layout"):
            print("%-40s %d shapes, e.g. %s" % (kind, lo[0], lo[1]))
        else:
            print("%-40s min %5.1f %% (%s)  max %5.1f %% (%s)  over %d cases" % (
                kind, 100 * lo[0], lo[1], 100 * hi[0], hi[1], len(vals)))
    assert kinds
