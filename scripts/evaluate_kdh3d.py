#!/usr/bin/env python
"""MI355X drop-in for the reference's evaluation scripts of the single-person KDH3D sets
(third_party_methods/evaluate/evaluation_rtpose_light3d_kdh3d_ablation.py and evaluation_yolo_posenet_kdh3d.py): `val` (--bg-aug 0) and
`test_bgaug` (--bg-aug 1: the frame's foreground pasted over background index % n_bg of a list shuffled once).  The same
``eval_data.json`` keys in --output-dir, the same 2D (2 % of the frame diagonal) and 3D (10 cm) tables.

    python scripts/evaluate_kdh3d.py --net rtpose --annotations labels/labels_val.json --image-dir depth_maps --weight best_pose.pth \
        --output-dir out [--bg-aug 1 --bg-file labels/labels_bg.json --bg-dir bg_maps --seg-dir seg_maps] [--drop-last] [--ablation]

--net rtpose: only the first parsed person of a frame is kept (the script's "HARD-CODED for single person"), a frame without one stays
empty; --ablation adds the three depth-ablation arms and human_gt_set_2d_visible and prints the five blocks of
popnet_amd.metrics.evaluate_ablation_blocks.  --net yolo: conf_threshold 0.1, the first person or the -1 placeholder person.

Departures from the reference scripts:
  * the background swap is a select on the mask (> 0) on the GPU; with the dataset's 0 / 1 masks that is the script's
    image * mask + bg * (1 - mask);
  * --bg-aug is an argument that is obeyed (the first script parses one and never hands it to its dataset); --seed N stands for
    `random.seed(N)` before the dataset shuffles its background list;
  * the tail of the frame list is evaluated unless --drop-last is given (the reference's loader has drop_last=True);
  * the intrinsics of the back-projection are the annotation file's `intrinsics` entry when it has one;
  * --ablation is a switch, --precision fp32 (default) the parity mode; the script never draws (the reference hard-codes vis=True);
  * no throughput is claimed for this path.
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
    ap.add_argument("--annotations", "--val-annotations", dest="annotations", required=True)
    ap.add_argument("--image-dir", "--val-image-dir", dest="image_dir", required=True)
    ap.add_argument("--bg-aug", type=int, default=0, choices=[0, 1], help="1: swap the background (test_bgaug); needs --bg-file, --bg-dir, --seg-dir")
    ap.add_argument("--bg-file")
    ap.add_argument("--bg-dir")
    ap.add_argument("--seg-dir")
    ap.add_argument("--weight", required=True, help="reference checkpoint (state_dict, 'module.'-prefixed or not)")
    ap.add_argument("--output-dir", required=True)
    ap.add_argument("--batch-size", type=int, default=15)
    ap.add_argument("--input-size", type=int, default=224)
    ap.add_argument("--w-org", type=int, default=480)
    ap.add_argument("--h-org", type=int, default=512)
    ap.add_argument("--seed", type=int, default=None, help="random.seed before the dataset is built")
    ap.add_argument("--drop-last", action="store_true", help="skip the tail like the reference's drop_last=True loader")
    ap.add_argument("--ablation", action="store_true", help="--net rtpose: the depth-ablation keys and their five metric blocks")
    ap.add_argument("--precision", default="fp32", choices=["fp32", "bf16"], help="fp32 = parity mode, bf16 = throughput mode")
    ap.add_argument("--no-metrics", action="store_true")
    args = ap.parse_args(argv)
    if args.ablation and args.net != "rtpose":
        ap.error("--ablation applies to --net rtpose only (the reference's Yolo-Pose+ script has no ablation keys)")
    if args.bg_aug and not (args.bg_file and args.bg_dir and args.seg_dir):
        ap.error("--bg-aug 1 needs --bg-file, --bg-dir and --seg-dir")
    return args


def main(argv=None):
    args = parse_args(argv)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("evaluate_kdh3d.py needs a GPU: the HIP path has no CPU fallback")
    import popnet_amd  # noqa: F401
    from popnet_amd import evalsets, targets
    from popnet_amd.pipeline import PoseEngine, YoloEngine

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    if args.seed is not None:
        random.seed(args.seed)
    ds = targets.KDH3DSingleSet(args.image_dir, args.annotations, bg_aug=bool(args.bg_aug), bg_file=args.bg_file, bg_dir=args.bg_dir,
                                seg_dir=args.seg_dir, device=dev)
    intr = ds.anno_dic.get("intrinsics", {})
    intr = {k: float(intr[k]) for k in ("fx", "fy", "cx", "cy")} if all(k in intr for k in ("fx", "fy", "cx", "cy")) else None
    kw = dict(precision=args.precision, state_dict=evalsets.load_state_dict(args.weight), device=dev, max_batch=args.batch_size, input_size=args.input_size,
              w_org=args.w_org, h_org=args.h_org, intrinsics=intr)
    eng = PoseEngine(**kw) if args.net == "rtpose" else YoloEngine(conf_threshold=0.1, **kw)
    n = len(ds) - (len(ds) % args.batch_size if args.drop_last else 0)
    data = {}
    for s in range(0, n, args.batch_size):
        chunk = list(range(s, min(s + args.batch_size, n)))
        frames = ds.frames(chunk)
        if tuple(frames.shape[1:]) != (args.h_org, args.w_org):
            raise SystemExit("the frames are %dx%d, --w-org x --h-org says %dx%d" % (frames.shape[2], frames.shape[1], args.w_org, args.h_org))
        x = ds.inputs(chunk, args.input_size, frames=frames)
        g2, g3 = ds.ground_truth(chunk)
        lists = evalsets.predict_batch(eng, x, g2, ablation=args.ablation, first_person=True)
        lists["human_gt_set_2d"], lists["human_gt_set_3d"] = g2, g3
        for k, v in lists.items():
            data.setdefault(k, []).extend(v)
    os.makedirs(args.output_dir, exist_ok=True)
    path = os.path.join(args.output_dir, "eval_data.json")
    json.dump(data, open(path, "w"), indent=4)
    print("wrote %s (%d frames, %s)" % (path, n, args.precision))
    if args.no_metrics:
        return None
    return evalsets.evaluate(data, args.w_org, args.h_org, args.ablation)


if __name__ == "__main__":
    main()
