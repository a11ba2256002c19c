#!/usr/bin/env python
"""MI355X drop-in for the reference's evaluation scripts of the composed KDH3D test set `test_mpaug`
(third_party_methods/evaluate/evaluation_rtpose_light3d_kdh3d_mpaug_ablation.py and evaluation_yolo_posenet_kdh3d_mpaug.py): frames are
composed per batch as KDH3D_Keypoints.generate_test_batch does -- a random index, the random sources of its aug_mods entry z-buffered over
a background, then Rotate / RenderDepth(max_ratio=--max-aug-ratio) / Resize, no Crop -- and the network sees that tensor.  The same
``eval_data.json`` keys in --output-dir, the same 2D (2 % of the frame diagonal) and 3D (10 cm) tables.

    python scripts/evaluate_mpaug.py --net rtpose --annotations labels/labels_test_*.json --image-dir depth_maps --bg-file labels/labels_bg.json \
        --bg-dir bg_maps --seg-dir seg_maps --weight best_pose.pth --output-dir out [--num-batches 100] [--batch-size 15] [--seed 0] [--ablation]

--net rtpose: human_pred_set_{2d,3d}, visibility_pred_set and the ground truth; --ablation adds the three depth-ablation arms and
human_gt_set_2d_visible (the nine keys of the first script) and prints the five blocks of popnet_amd.metrics.evaluate_ablation_blocks.  The
"raw depth" of the arms is the network input un-normalised, as in the script.  --net yolo: conf_threshold 0.5, nms_threshold 0.5, every
person of a frame, the -1 placeholder person when there is none.

Departures from the reference scripts:
  * the host draws come from Python's `random` in the reference's order, so --seed N gives the frames `random.seed(N)` at the top of the
    reference script gives; without --seed the run is not repeatable (as the reference's);
  * the composition, the transform's image half, the network, the parse and the arms run on the GPU; --precision fp32 (default) is the
    parity mode, bf16 the throughput mode;
  * the principal point of Rotate / RenderDepth and the intrinsics of the back-projection are the annotation files' `intrinsics` entry (the
    reference hard-codes the same numbers in its dataset module);
  * --ablation is a switch: the first script always computes the arms;
  * the script never draws (the reference hard-codes vis=True and shows every frame);
  * frames are not sharded over GPUs: every frame depends on the one host random stream;
  * the 2D ground truth is scaled back to --w-org x --h-org on the transformed labels like the script does; no throughput is claimed for
    this path.
"""
import argparse
import json
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--net", required=True, choices=["rtpose", "yolo"])
    ap.add_argument("--annotations", "--val-annotations", dest="annotations", nargs="+", required=True)
    ap.add_argument("--image-dir", "--val-image-dir", dest="image_dir", required=True)
    ap.add_argument("--bg-file", required=True)
    ap.add_argument("--bg-dir", required=True)
    ap.add_argument("--seg-dir", required=True)
    ap.add_argument("--weight", required=True, help="reference checkpoint (state_dict, 'module.'-prefixed or not)")
    ap.add_argument("--output-dir", required=True)
    ap.add_argument("--batch-size", type=int, default=15)
    ap.add_argument("--num-batches", type=int, default=100, help="the total number of batches to evaluate a method")
    ap.add_argument("--input-size", type=int, default=224)
    ap.add_argument("--w-org", type=int, default=480)
    ap.add_argument("--h-org", type=int, default=512)
    ap.add_argument("--max-aug-ratio", type=float, default=1.7, help="the max augment depth ratio")
    ap.add_argument("--seed", type=int, default=None, help="random.seed before the dataset is built")
    ap.add_argument("--ablation", action="store_true", help="--net rtpose: the depth-ablation keys and their five metric blocks")
    ap.add_argument("--precision", default="fp32", choices=["fp32", "bf16"], help="fp32 = parity mode, bf16 = throughput mode")
    ap.add_argument("--no-metrics", action="store_true")
    args = ap.parse_args(argv)
    if args.ablation and args.net != "rtpose":
        ap.error("--ablation applies to --net rtpose only (the reference's Yolo-Pose+ script has no ablation keys)")
    return args


def main(argv=None):
    args = parse_args(argv)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("evaluate_mpaug.py needs a GPU: the HIP path has no CPU fallback")
    import popnet_amd  # noqa: F401
    from popnet_amd import evalsets, targets
    from popnet_amd.config import DEPTH_MAX, DEPTH_MEAN, DEPTH_STD
    from popnet_amd.pipeline import PoseEngine, YoloEngine

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    if args.seed is not None:
        random.seed(args.seed)
    ts = targets.MPAugTrainSet(args.image_dir, args.annotations, args.bg_file, args.bg_dir, args.seg_dir, device=dev)
    intr = {k: float(v) for k, v in ts.annos[0]["intrinsics"].items()} if all(k in ts.annos[0].get("intrinsics", {}) for k in ("fx", "fy", "cx", "cy")) else None
    kw = dict(precision=args.precision, state_dict=evalsets.load_state_dict(args.weight), device=dev, max_batch=args.batch_size, input_size=args.input_size,
              w_org=args.w_org, h_org=args.h_org, intrinsics=intr)
    eng = PoseEngine(**kw) if args.net == "rtpose" else YoloEngine(conf_threshold=0.5, nms_threshold=0.5, **kw)
    data = {}
    for batch_i in range(args.num_batches):
        fd, fm, n_src, bg, k2, k3, npers, aug = ts.test_batch(args.batch_size, input_size=args.input_size, max_aug_ratio=args.max_aug_ratio)
        if tuple(fd.shape[2:]) != (args.h_org, args.w_org):
            raise SystemExit("the frames are %dx%d, --w-org x --h-org says %dx%d" % (fd.shape[3], fd.shape[2], args.w_org, args.h_org))
        image = targets.compose_depth(fd, fm, n_src, bg, DEPTH_MAX)
        x = targets.augment_resize(image, aug, args.input_size, DEPTH_MAX, DEPTH_MEAN, DEPTH_STD)
        kp, kz, _ = aug.transform_labels(k2, k3)
        g2, g3 = targets.composed_ground_truth(kp, k3, kz, npers, args.w_org, args.h_org, args.input_size)
        lists = evalsets.predict_batch(eng, x, g2, ablation=args.ablation)
        lists["human_gt_set_2d"], lists["human_gt_set_3d"] = g2, g3
        for k, v in lists.items():
            data.setdefault(k, []).extend(v)
    os.makedirs(args.output_dir, exist_ok=True)
    path = os.path.join(args.output_dir, "eval_data.json")
    json.dump(data, open(path, "w"), indent=4)
    print("wrote %s (%d frames, %s)" % (path, args.num_batches * args.batch_size, args.precision))
    if args.no_metrics:
        return None
    return evalsets.evaluate(data, args.w_org, args.h_org, args.ablation)


if __name__ == "__main__":
    main()
