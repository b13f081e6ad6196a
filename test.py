"""Drop-in for the reference's evaluation CLI (test.py:61-83, :168-344) for --model raa:

    python test.py --dataset sbmrgbd --model raa --gpus 0 [--checkpoint snapshot.pth]

For every target frame: the mean over `sample_range` reference frames of the model's x1
(test.py:287-305), resized to output_WH with bilinear half-pixel interpolation (cv2.resize
INTER_LINEAR, :309-314), quantised (output * 255).astype(uint8) (:317), scored with the soft
IoU of evaluation.py:3-22 (:321), logged as "##== seq: S frame: F IOU: J==##" (:322) and saved
as a PNG mask (:332-340); the run ends with "##== final IOU: mean==##" (:342-344).

MI355X-native: the N references run as ONE batched forward with the target encoded once
(cosnet_amd.inference.multi_reference_x1; equal to the reference's loop in eval mode), the
average and the resize are HIP kernels; only the uint8 masks cross to the host.  Checkpoints
load with torch.load(weights_only=True); "module." prefixes are stripped (test.py:140-161).
`--dataset sbmrgbd` reads the SBM-RGBD tree (cosnet_amd/sbm_rgbd.py, GPU frame preparation);
`--dataset synthetic` evaluates seeded frame pairs (cosnet_amd/data.py).
`--feature-bank` (sbmrgbd): the references of a target are frames of its own sequence, so each
sequence's frames are loaded and encoded ONCE and the pairs are formed by index
(cosnet_amd.inference.segment_sequence); same log lines, order and PNGs.  With it,
`--coatt mxfp8` (bf16 only) runs the bank's co-attention on MX-fp8 images of the features, and
`--dtype fp8 [--fp8-calibration FILE]` runs the encoders' conv GEMMs on e4m3 operands under
calibrated, frozen scales (cosnet_amd/fp8_infer.py); the two compose.  `--split-reduce` runs the
head's reduce convs split by input-channel half, the pass-through half once per frame
(model.set_head_split(), segment_sequence(head="split")); it composes with all of the above.
"""
import argparse
import datetime
import os
import sys

REPO = os.path.dirname(os.path.abspath(__file__))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

LOG_START, LOG_END = "##==", "==##"


def get_arguments(argv=None):
    p = argparse.ArgumentParser(description="RGBDCoAttention")
    p.add_argument("--dataset", type=str, default="synthetic")
    p.add_argument("--cuda", default=True)
    p.add_argument("--gpus", type=str, default="0")
    p.add_argument("--seq_name", default="bmx-bumps")
    p.add_argument("--use_crf", default="True")
    p.add_argument("--save_seg_img", default="True")
    p.add_argument("--sample_range", default=5)
    p.add_argument("--epoches", default=0)
    p.add_argument("--batch_size", default=0)
    p.add_argument("--model", default="raa")
    # this build
    p.add_argument("--config", default=os.path.join(REPO, "config.yaml"))
    p.add_argument("--checkpoint", default=None, help="overrides test.model.<name>.pretrained_params")
    p.add_argument("--dtype", default="bf16", choices=["bf16", "fp32", "fp8"],
                   help="bf16 (default): the MI355X throughput path, fused co-attention; fp32: the reference "
                        "arithmetic; fp8 (--feature-bank): the bf16 path with the encoders' conv GEMMs on e4m3 "
                        "operands under calibrated, frozen scales (cosnet_amd/fp8_infer.py)")
    p.add_argument("--result-root", default=".")
    p.add_argument("--frames", type=int, default=None, help="synthetic: number of target frames")
    p.add_argument("--feature-bank", action="store_true",
                   help="whole-sequence inference: encode every frame of a sequence once and form the "
                        "(target, reference) pairs by index (cosnet_amd.inference.segment_sequence)")
    p.add_argument("--coatt", default="bf16", choices=["bf16", "mxfp8"],
                   help="--feature-bank: the bank's co-attention.  bf16 (default): the bf16 indexed kernel; "
                        "mxfp8: MX-fp8 images of the bf16 features, each frame quantised once per sequence")
    p.add_argument("--fold-bn", action="store_true",
                   help="--feature-bank (bf16 / fp32): every conv + eval-mode BatchNorm pair of the encoders and "
                        "of the head's reduce convs as one launch (cosnet_amd/bn_fold.py)")
    p.add_argument("--fp8-fold-bn", action="store_true",
                   help="--feature-bank --dtype fp8: every fp8 conv + eval-mode BatchNorm pair of the encoders as "
                        "one launch (cn_conv_fwd_fp8_affine) and the head's reduce convs folded "
                        "(model.set_fp8_static(calibration, fold_bn=True))")
    p.add_argument("--split-reduce", action="store_true",
                   help="--feature-bank: the head's 3x3 reduce convs split by input-channel half -- the "
                        "pass-through half V_a once per frame, the gated half per pair with that partial added "
                        "in the GEMM epilogue (model.set_head_split(), segment_sequence(head='split'))")
    p.add_argument("--fp8-calibration", default=None, metavar="FILE",
                   help="--dtype fp8: the calibration (JSON).  Loaded if the file exists; otherwise made "
                        "before evaluation from the first --fp8-calibration-frames test frames and written there")
    p.add_argument("--fp8-calibration-frames", type=int, default=16)
    args = p.parse_args(argv)
    if args.coatt == "mxfp8" and not args.feature_bank:
        p.error("--coatt mxfp8 needs --feature-bank")
    if args.coatt == "mxfp8" and args.dtype not in ("bf16", "fp8"):
        p.error("--coatt mxfp8 needs --dtype bf16 (or fp8, whose features are bf16)")
    if args.dtype == "fp8" and not args.feature_bank:
        p.error("--dtype fp8 needs --feature-bank")
    if args.fold_bn and not args.feature_bank:
        p.error("--fold-bn needs --feature-bank")
    if args.fold_bn and args.dtype == "fp8":
        p.error("--fold-bn runs the bf16 / fp32 encoders (not --dtype fp8)")
    if args.fp8_fold_bn and not (args.feature_bank and args.dtype == "fp8"):
        p.error("--fp8-fold-bn needs --feature-bank --dtype fp8")
    if args.split_reduce and not args.feature_bank:
        p.error("--split-reduce needs --feature-bank")
    if args.dtype == "fp8" and args.fp8_calibration_frames < 1:
        p.error("--fp8-calibration-frames must be at least 1")
    if args.dtype != "fp8" and args.fp8_calibration:
        p.error("--fp8-calibration needs --dtype fp8")
    return args


def config(args, user_config):
    """test.py:86-137 (sbmrgbd / synthetic)."""
    ds = user_config["test"]["dataset"].get(args.dataset)
    if ds is None:
        raise SystemExit("dataset error: %r" % args.dataset)
    args.batch_size = int(args.batch_size) if args.batch_size else 1
    args.epoches = int(args.epoches) if args.epoches else 15
    args.num_classes = 2
    args.data_path = ds.get("data_path", "")
    args.sample_range = int(ds["sample_range"])  # the YAML overrides the flag (test.py:132)
    h, w = map(int, str(ds["image_HW_4_model"]).split(","))
    args.image_HW_4_model = (h, w)
    w, h = map(int, str(ds["output_WH"]).split(","))
    args.output_WH = (w, h)
    args.frames = args.frames if args.frames is not None else int(ds.get("frames", 8))
    args.subset = ds.get("subset") or None


def main(argv=None):
    args = get_arguments(argv)
    os.environ["CUDA_VISIBLE_DEVICES"] = args.gpus  # test.py:175, before HIP starts
    import numpy as np
    import torch
    import yaml

    import cosnet_amd as C
    from cosnet_amd.checkpoint import convert_state_dict, load_checkpoint
    from cosnet_amd.data import SyntheticRGBDPairs
    from cosnet_amd.inference import multi_reference_x1, resize_linear, segment_sequence, soft_iou

    with open(args.config) as f:
        user_config = yaml.safe_load(f)
    config(args, user_config)
    if args.model not in ("raa", "resnet_aspp_add"):
        print("Invalid model name!")
        return 1
    args.full_model_name = "resnet_aspp_add"
    if not torch.cuda.is_available():
        raise Exception("No GPU found or Wrong gpu id, please run without --cuda")
    dev = torch.device("cuda:0")
    stamp = datetime.datetime.now().strftime("%Y%m%d_%H%M%S")
    args.result_dir = os.path.join(args.result_root, "vos_test_results", args.dataset,
                                   args.full_model_name, stamp)
    os.makedirs(args.result_dir, exist_ok=True)
    log_name = os.path.join(args.result_dir, "%s__%s_%s_test_log.txt" % (args.dataset, args.full_model_name, stamp))
    logger = open(log_name, "a")
    ckpt = args.checkpoint or user_config["test"]["model"][args.full_model_name].get("pretrained_params", "")
    args.pretrained_params = ckpt
    logger.write(LOG_START + str(args) + LOG_END + "\n")
    logger.flush()

    model = C.build_model(torch.float32 if args.dtype == "fp32" else torch.bfloat16)
    if ckpt:
        model.load_state_dict(convert_state_dict(load_checkpoint(ckpt)["model"]))
    else:
        print("no pretrained_params given: seeded initialisation (scores are meaningless)")
    model.eval()
    model.to(dev)
    if args.fold_bn:
        model.set_bn_fold()
    if args.split_reduce:
        model.set_head_split()
    head = "split" if args.split_reduce else "cat"

    out_dir = None
    if str(args.save_seg_img) not in ("False", "0", ""):
        out_dir = os.path.join(args.result_dir, "obj_seg_imgs")
        os.makedirs(out_dir, exist_ok=True)
    out_hw = (args.output_WH[1], args.output_WH[0])
    score = {"sum": 0.0, "n": 0}

    def emit(x1, gt, seq, frame):
        """Resize, quantise, score, log and save one target's mean x1 [1,1,h,w] (test.py:307-340)."""
        gt = gt.unsqueeze(1).float()
        if tuple(gt.shape[2:]) != out_hw:
            gt = torch.nn.functional.interpolate(gt, size=out_hw, mode="nearest")
        # uint8 quantisation (:317) + soft-J (evaluation.py:3-22) in one HIP kernel
        masks, ious, _ = soft_iou(resize_linear(x1, out_hw), gt[:, 0].to(torch.uint8).to(dev))
        mask = masks[0].cpu().numpy()                                  # [H,W] uint8
        iou = float(ious[0].item())
        logger.write(LOG_START + " seq: " + seq + " frame: " + frame + " IOU: " + str(iou) + LOG_END + "\n")
        score["sum"] += iou
        score["n"] += 1
        if out_dir:
            from PIL import Image
            d = os.path.join(out_dir, seq)
            os.makedirs(d, exist_ok=True)
            Image.fromarray(mask).save(os.path.join(d, "%s.png" % frame))

    def static_fp8(load_frames):
        """--dtype fp8: the calibration file if it exists, else one made from load_frames(k) =
        (rgbs, depths) of the first k test frames (and written to the file, if one is named)."""
        from cosnet_amd.fp8_infer import Fp8Calibration, calibrate
        path = args.fp8_calibration
        if path and os.path.exists(path):
            calib = Fp8Calibration.load(path)
        else:
            calib = calibrate(model, *load_frames(args.fp8_calibration_frames))
            if path:
                calib.save(path)
        model.set_fp8_static(calib, fold_bn=args.fp8_fold_bn)

    db = None
    if args.dataset == "sbmrgbd":
        from cosnet_amd.sbm_rgbd import SBMRGBD
        if not args.data_path or not os.path.isdir(args.data_path):
            raise SystemExit("sbmrgbd: data_path %r not found (config.yaml test.dataset.sbmrgbd)" % args.data_path)
        sbm = SBMRGBD(args.data_path, args.sample_range, args.image_HW_4_model, for_training=False,
                      batch_size=args.batch_size, subset_percentage=1, subset=args.subset or None,
                      device=dev)  # test.py:271-272
        if args.feature_bank:
            # the plans of all targets in index order (the RNG draws of __getitem__, no pixels), then
            # sequence by sequence (a sequence's frames are contiguous): every distinct frame loaded
            # and encoded once, targets scored and logged in index order
            frames = sbm.sets[sbm.stage]["names_of_frames"]
            n = len(sbm)
            if args.dtype == "fp8":   # test-stage frames in list order; loading draws nothing from the RNG
                def first_frames(k):
                    fr = [sbm.load_frame(frames[i]) for i in range(min(k, n))]
                    return torch.stack([f[0] for f in fr]), torch.stack([f[1] for f in fr])
                static_fp8(first_frames)
            plans = [sbm.reference_plan(i) for i in range(n)]
            k = 0
            while k < n:
                k1 = k
                while k1 < n and frames[k1].seq_name == frames[k].seq_name:
                    k1 += 1
                used = sorted({f for pl in plans[k:k1] for f in pl})
                pos = {f: i for i, f in enumerate(used)}
                loaded = [sbm.load_frame(frames[f]) for f in used]
                x1 = segment_sequence(model, torch.stack([l[0] for l in loaded]),
                                      torch.stack([l[1] for l in loaded]),
                                      [[pos[f] for f in pl[1:]] for pl in plans[k:k1]],
                                      targets=[pos[pl[0]] for pl in plans[k:k1]], coatt=args.coatt,
                                      head=head)
                for i in range(k, k1):
                    if i % args.batch_size == 0:
                        print("%d processd" % (i // args.batch_size))
                    emit(x1[i - k:i - k + 1], loaded[pos[i]][2][None], frames[i].seq_name, frames[i].id)
                k = k1
        else:
            db = [sbm.collate([sbm[j] for j in range(i, i + args.batch_size)])
                  for i in range(0, len(sbm), args.batch_size)]
    elif args.dataset == "synthetic":
        db = SyntheticRGBDPairs(args.frames // args.batch_size, args.image_HW_4_model, args.batch_size,
                                sample_range=args.sample_range, seed=4321)
        if args.dtype == "fp8":
            def first_targets(k):
                bs = [db[i] for i in range(min(len(db), -(-k // args.batch_size)))]
                return (torch.cat([b["target"] for b in bs])[:k].to(dev),
                        torch.cat([b["target_depth"] for b in bs])[:k].to(dev))
            static_fp8(first_targets)
    else:
        raise SystemExit("dataset %r: only sbmrgbd and synthetic are provided by this build" % args.dataset)
    for index, batch in enumerate(db or ()):
        print("%d processd" % index)
        for j in range(args.batch_size):
            tgt = batch["target"][j:j + 1].to(dev)
            tdep = batch["target_depth"][j:j + 1].to(dev)
            srch = torch.cat([batch["search_%d" % i][j:j + 1] for i in range(args.sample_range)]).to(dev)
            sdep = torch.cat([batch["search_%d_depth" % i][j:j + 1] for i in range(args.sample_range)]).to(dev)
            if args.feature_bank:
                # synthetic frames belong to no sequence: a bank of the target and its own references
                x1 = segment_sequence(model, torch.cat([tgt, srch]), torch.cat([tdep, sdep]),
                                      [list(range(1, args.sample_range + 1))], targets=[0],
                                      coatt=args.coatt, head=head)
            else:
                x1 = multi_reference_x1(model, tgt, tdep, srch, sdep)      # [1,1,h,w]
            emit(x1, batch["target_gt"][j:j + 1], batch["seq_name"][j], batch["frame_index"][j])
    iou_sum, iou_n = score["sum"], score["n"]
    final = iou_sum / max(iou_n, 1)
    logger.write(LOG_START + " final IOU: " + str(final) + LOG_END + "\n")
    logger.close()
    print("final IOU: %.6f over %d frames (log: %s)" % (final, iou_n, log_name))
    return 0


if __name__ == "__main__":
    sys.exit(main())
