"""Whole-sequence inference against the per-target path on one seeded synthetic sequence
(defaults: T = 12 frames, N = 5 references, 473 x 473, bf16; configs[3]'s shape per target).

  per-target: cosnet_amd.inference.multi_reference_x1 once per frame, as test.py runs it: every
              call encodes the target and its N references and runs both sides of the head;
  bank:       cosnet_amd.inference.segment_sequence: every frame encoded once (FeatureBank), the a
              side of the head over index maps (head_a_indexed), one grouped mean.

References are drawn like the loader draws them (sbm_rgbd_loader.py:538-579):
random.Random(seed).sample(range(T), N) per target.  The two paths alternate on the same device
(--rounds times each after --warmup untimed rounds), each timing is HIP events around a whole
sequence; the spread is the (max - min) / mean of a path's own rounds.  A second, separately timed
pass splits each path into its encoder stage and its head stage with events between the stages
(the per-target stages are multi_reference_x1's own calls, in its order).  One JSON line.

--coatt mxfp8 runs the bank path's co-attention on MX-fp8 images of the bank (bf16 only; default
bf16, the indexed bf16 kernel).  The result then also holds the one-off image build of the bank
(both modalities, timed on its own over the rounds; it is part of the bank's encoder stage) and
the outputs against the bf16 bank's on the same sequence.  To compare the two settings, alternate
runs of this tool with --coatt bf16 and --coatt mxfp8 on one device.

--dtype fp8 times the bank path with static-scale fp8 encoders (cosnet_amd/fp8_infer.py),
calibrated on the tool's own sequence before timing; the per-target path stays bf16 and the result
also holds the fp8 bank's outputs against the bf16 bank's.  Alternate runs with --dtype bf16 and
--dtype fp8 to compare.

--head split runs the bank path's head with the reduce convs split by input-channel half
(model.set_head_split, cosnet_amd/head_split.py; composes with every setting above); the result
then also holds its outputs against the default ("cat") head's in the same setting.  Alternate runs
with --head cat and --head split to compare.
"""
import argparse
import json
import os
import random
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import cosnet_amd as C  # noqa: E402
from cosnet_amd import _native as nv  # noqa: E402
from cosnet_amd import ops  # noqa: E402
from cosnet_amd.inference import FeatureBank, multi_reference_x1, plan_pairs, segment_sequence  # noqa: E402
from cosnet_amd.init_recipe import BGR_MEAN, recipe_state_dict  # noqa: E402


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=12)
    ap.add_argument("--nref", type=int, default=5)
    ap.add_argument("--size", type=int, default=473)
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp32", "fp8"],
                    help="fp8: the bank path's encoders on static-scale e4m3 conv GEMMs, calibrated on "
                         "this sequence before timing (the per-target path stays bf16)")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--encode-chunk", type=int, default=8)
    ap.add_argument("--pair-chunk", type=int, default=10)
    ap.add_argument("--coatt", default="bf16", choices=["bf16", "mxfp8"],
                    help="the bank path's co-attention (mxfp8: MX-fp8 images, --dtype bf16 only)")
    ap.add_argument("--fold-bn", action="store_true",
                    help="the bank path with eval-mode BN folded into the conv GEMMs (model.set_bn_fold; "
                         "--dtype bf16 / fp32); its outputs are also held against the default bank's")
    ap.add_argument("--fp8-fold-bn", action="store_true",
                    help="--dtype fp8: eval-mode BN folded into the static-scale fp8 conv GEMMs "
                         "(model.set_fp8_static(calibration, fold_bn=True))")
    ap.add_argument("--head", default="cat", choices=["cat", "split"],
                    help="the bank path's head: cat (default), the reduce convs over the concat per pair; split, "
                         "their pass-through half once per frame (model.set_head_split)")
    a = ap.parse_args()
    if a.fold_bn and a.dtype == "fp8":
        ap.error("--fold-bn runs the bf16 / fp32 encoders")
    if a.fp8_fold_bn and a.dtype != "fp8":
        ap.error("--fp8-fold-bn needs --dtype fp8")
    if a.coatt == "mxfp8" and a.dtype == "fp32":
        ap.error("--coatt mxfp8 needs --dtype bf16 or fp8")
    return a


def timed(fn):
    """Milliseconds of fn() by HIP events (the stream is idle before and drained after)."""
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    r = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), r


class Stages:
    """Event pairs around alternating stages of one pass; totals per stage name after a sync."""

    def __init__(self):
        self.ev = []

    def run(self, name, fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        r = fn()
        e1.record()
        self.ev.append((name, e0, e1))
        return r

    def totals(self):
        torch.cuda.synchronize()
        out = {}
        for name, e0, e1 in self.ev:
            out[name] = out.get(name, 0.0) + e0.elapsed_time(e1)
        return out


def main():
    a = parse()
    if not torch.cuda.is_available():
        raise SystemExit("seq_infer_bench: needs the GPU (no timing without one)")
    dev = torch.device("cuda:0")
    T, N, H = a.frames, a.nref, a.size
    dt = torch.float32 if a.dtype == "fp32" else torch.bfloat16
    m = C.build_model(dt)
    sd = recipe_state_dict(m.state_dict())
    calib = os.path.join(REPO, "tests", "golden", "bn_calibration_473.npz")
    if os.path.exists(calib):   # running statistics of this initialisation (activations stay in range)
        z = np.load(calib, allow_pickle=False)
        for k in z.files:
            sd[k[len("calib/"):]] = torch.from_numpy(z[k])
    m.load_state_dict(sd)
    m = m.to(dev).eval()

    g = torch.Generator().manual_seed(a.seed)
    mean = torch.tensor(BGR_MEAN, dtype=torch.float32).view(1, 3, 1, 1)
    rgbs = (torch.rand((T, 3, H, H), generator=g) * 255.0 - mean).to(dev)
    deps = (torch.rand((T, 1, H, H), generator=g) * 255.0).to(dev)
    rng = random.Random(a.seed)
    refs = [rng.sample(range(T), N) for _ in range(T)]
    ridx = [torch.tensor(r, device=dev) for r in refs]

    def per_target():
        return torch.cat([multi_reference_x1(m, rgbs[t:t + 1], deps[t:t + 1], rgbs[ridx[t]], deps[ridx[t]])
                          for t in range(T)])

    # --dtype fp8: calibrated on this sequence, tables and e4m3 weights built once; the bank path
    # switches the built state on around its calls (two attribute writes), the per-target path and
    # the bf16 reference bank run with it off
    static = None
    if a.dtype == "fp8":
        from cosnet_amd.fp8_infer import calibrate
        static = m.set_fp8_static(calibrate(m, rgbs, deps, a.encode_chunk), fold_bn=a.fp8_fold_bn).fp8_static
        m.set_fp8_static(None)

    # --fold-bn: the tables are built once, here; the bank path switches the built state on around
    # its calls, the per-target path and the default reference bank run with it off
    fold = None
    if a.fold_bn:
        fold = m.set_bn_fold().bn_fold
        m.set_bn_fold(False)

    if a.head == "split":   # the weight halves (and tables) are built once, here
        m.set_head_split()

    def with_static(fn):
        if fold is not None:
            m.set_bn_fold(fold)
            try:
                return fn()
            finally:
                m.set_bn_fold(False)
        if static is None:
            return fn()
        m.set_fp8_static(static)
        try:
            return fn()
        finally:
            m.set_fp8_static(None)

    def bank():
        return with_static(lambda: segment_sequence(m, rgbs, deps, refs, encode_chunk=a.encode_chunk,
                                                    pair_chunk=a.pair_chunk, coatt=a.coatt, head=a.head))

    # ---- stage split: the same calls with events between the stages -------------------------------
    @torch.no_grad()
    def per_target_stages(st):
        hw_out = H * H
        for t in range(T):
            def enc():
                va, _ = m.encoder.features_nhwc(rgbs[t:t + 1])
                da, _ = m.depth_encoder.features_nhwc(deps[t:t + 1])
                vb, geo = m.encoder.features_nhwc(rgbs[ridx[t]])
                db, _ = m.depth_encoder.features_nhwc(deps[ridx[t]])
                return va, da, vb, db, geo

            def head(va, da, vb, db, geo):
                p1 = va.shape[0]
                va_n = torch.empty((N * p1, va.shape[1]), dtype=va.dtype, device=dev)
                da_n = torch.empty_like(va_n)
                for i in range(N):
                    ops.cast_copy(va, va_n[i * p1:(i + 1) * p1])
                    ops.cast_copy(da, da_n[i * p1:(i + 1) * p1])
                x1, _ = m.head_nhwc(va_n, vb, da_n, db, geo, (H, H))
                out = torch.empty((1, hw_out), dtype=torch.float32, device=dev)
                nv.call("cn_mean_rows", x1.contiguous().data_ptr(), N, hw_out, out.data_ptr(), nv.stream())
                return out

            f = st.run("encoder", enc)
            st.run("head", lambda: head(*f))

    @torch.no_grad()
    def bank_stages(st):
        ia, ib = plan_pairs(T, list(range(T)), refs)
        b = st.run("encoder", lambda: with_static(
            lambda: FeatureBank.encode(m, rgbs, deps, a.encode_chunk, a.coatt)))
        step = max(1, a.pair_chunk // N)

        def head():
            out = torch.empty((T, H * H), dtype=torch.float32, device=dev)
            for t0 in range(0, T, step):
                t1 = min(T, t0 + step)
                x1 = m.head_a_indexed(b, ia[t0 * N:t1 * N], ib[t0 * N:t1 * N], split=a.head == "split")
                ops.mean_groups(x1.view((t1 - t0) * N, H * H), t1 - t0, N, out=out[t0:t1])
            return out

        st.run("head", lambda: with_static(head))

    m._set_dtype()
    for _ in range(max(1, a.warmup)):   # every shape of the timed window, both paths
        out_a, out_b = per_target(), bank()
    ta, tb = [], []
    for _ in range(a.rounds):           # alternating, same device, same process
        ta.append(timed(per_target)[0])
        tb.append(timed(bank)[0])
    sa, sb = Stages(), Stages()
    for _ in range(a.rounds):
        per_target_stages(sa)
        bank_stages(sb)
    split_a = {k: v / a.rounds for k, v in sa.totals().items()}
    split_b = {k: v / a.rounds for k, v in sb.totals().items()}

    extra = {}
    if a.coatt == "mxfp8":
        with torch.no_grad():
            b = FeatureBank.encode(m, rgbs, deps, a.encode_chunk)
            hw = b.geo[1] * b.geo[2]
            build = lambda: (ops.coatt_f8_bank(b.vat, b.va, T, hw), ops.coatt_f8_bank(b.dat, b.da, T, hw))
            build()
            tm = [timed(build)[0] for _ in range(a.rounds)]
            imgs = build()
        ref = segment_sequence(m, rgbs, deps, refs, encode_chunk=a.encode_chunk,
                               pair_chunk=a.pair_chunk).double().cpu()
        fm = out_b.double().cpu()
        extra = {"image_build_ms": {"mean": float(np.mean(tm)), "min": float(np.min(tm)), "max": float(np.max(tm))},
                 "image_bytes_per_frame_and_modality": imgs[0].numel() // T,
                 "vs_bf16_bank": {"mask_agreement": float(((fm > 0.5) == (ref > 0.5)).double().mean()),
                                  "mean_abs_diff": float((fm - ref).abs().mean()),
                                  "max_abs_diff": float((fm - ref).abs().max())}}
    if static is not None:   # the static-fp8 bank against the bf16 bank (same co-attention setting)
        ref = segment_sequence(m, rgbs, deps, refs, encode_chunk=a.encode_chunk, pair_chunk=a.pair_chunk,
                               coatt=a.coatt).double().cpu()
        fm = out_b.double().cpu()
        extra["fp8_vs_bf16_bank"] = {"mask_agreement": float(((fm > 0.5) == (ref > 0.5)).double().mean()),
                                     "mean_abs_diff": float((fm - ref).abs().mean()),
                                     "max_abs_diff": float((fm - ref).abs().max())}
    if a.fold_bn:   # the folded bank against the default bank (same co-attention setting)
        ref = segment_sequence(m, rgbs, deps, refs, encode_chunk=a.encode_chunk, pair_chunk=a.pair_chunk,
                               coatt=a.coatt).double().cpu()
        fm = out_b.double().cpu()
        extra["fold_vs_default_bank"] = {"mask_agreement": float(((fm > 0.5) == (ref > 0.5)).double().mean()),
                                         "mean_abs_diff": float((fm - ref).abs().mean()),
                                         "max_abs_diff": float((fm - ref).abs().max())}
    if a.head == "split":   # the split head against the default head, every other setting the same
        ref = with_static(lambda: segment_sequence(m, rgbs, deps, refs, encode_chunk=a.encode_chunk,
                                                   pair_chunk=a.pair_chunk, coatt=a.coatt)).double().cpu()
        fm = out_b.double().cpu()
        extra["split_vs_cat_head"] = {"mask_agreement": float(((fm > 0.5) == (ref > 0.5)).double().mean()),
                                      "mean_abs_diff": float((fm - ref).abs().mean()),
                                      "max_abs_diff": float((fm - ref).abs().max())}
    fa, fb = out_a.double().cpu(), out_b.double().cpu()
    stat = lambda v: {"mean": float(np.mean(v)), "min": float(np.min(v)), "max": float(np.max(v)),
                      "spread": float((np.max(v) - np.min(v)) / np.mean(v))}
    ma, mb = float(np.mean(ta)), float(np.mean(tb))
    res = {
        "tool": "seq_infer_bench", "frames": T, "nref": N, "size": H, "dtype": a.dtype, "coatt": a.coatt,
        "fold_bn": bool(a.fold_bn), "fp8_fold_bn": bool(a.fp8_fold_bn), "head": a.head,
        "seed": a.seed, "rounds": a.rounds, "warmup": max(1, a.warmup), "encode_chunk": a.encode_chunk,
        "pair_chunk": a.pair_chunk, "device": torch.cuda.get_device_name(0),
        "per_target": {"frames_per_s": T / (ma * 1e-3), "ms_per_sequence": stat(ta),
                       "encoder_ms": split_a["encoder"], "head_ms": split_a["head"],
                       "encoder_passes": T * (1 + N)},
        "bank": {"frames_per_s": T / (mb * 1e-3), "ms_per_sequence": stat(tb),
                 "encoder_ms": split_b["encoder"], "head_ms": split_b["head"], "encoder_passes": T, **extra},
        "speedup": ma / mb,
        # faster by more than the run-to-run spread: the slowest bank round against the fastest
        # per-target round
        "speedup_worst_case": float(np.min(ta) / np.max(tb)),
        "outputs": {"mask_agreement": float(((fa > 0.5) == (fb > 0.5)).double().mean()),
                    "mean_abs_diff": float((fa - fb).abs().mean()),
                    "max_abs_diff": float((fa - fb).abs().max())},
        "lib": nv.build_info(),
    }
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
