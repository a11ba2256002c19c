#!/usr/bin/env python
"""MI355X drop-in for the reference's Yolo-A2J evaluation of MP-3DHP
(third_party_methods/A2J_experiments/evaluation_yolo_posenet_kdh3d_mpreal_a2j_preprocess.py followed by a2j_test_pred_box_new.py):
YoloPoseNet finds the boxes, A2J regresses 15 joints per box crop.  The arguments of scripts/evaluate_mpreal.py plus --a2j-weight; the
same ``eval_data.json`` in --output-dir and the same four metric blocks (popnet_amd.metrics).  This script runs one GPU and one batch at a
time: --net (only ``yolo`` makes the boxes), --pipeline and --gpus 1 are accepted for a carried-over command line and say what they do
here; --gpus above 1 and --ablation (Open-Pose+ only) are refused with the reason.

    python scripts/evaluate_mpreal_a2j.py --annotations labels.json --image-dir depth_maps --weight best_pose.pth \
        --a2j-weight net_47.pth --output-dir out [--precision fp32|bf16|bf16x3] [--batch-size 32] [--drop-last]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _state_dict(path):
    sd = torch.load(path, map_location="cpu")
    return {(k[len("module."):] if k.startswith("module.") else k): v for k, v in sd.items()}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--annotations", "--val-annotations", dest="annotations", required=True)
    ap.add_argument("--image-dir", "--val-image-dir", dest="image_dir", required=True)
    ap.add_argument("--batch-size", type=int, default=32)
    ap.add_argument("--input-size", type=int, default=224)
    ap.add_argument("--w-org", type=int, default=480)
    ap.add_argument("--h-org", type=int, default=640)
    ap.add_argument("--weight", required=True, help="YoloPoseNet checkpoint (state_dict, 'module.'-prefixed or not)")
    ap.add_argument("--a2j-weight", required=True, help="A2J_model checkpoint (the reference's 410 keys)")
    ap.add_argument("--output-dir", required=True)
    ap.add_argument("--precision", default="fp32", choices=["fp32", "bf16", "bf16x3"])
    ap.add_argument("--crop", type=int, default=288)
    ap.add_argument("--drop-last", action="store_true")
    ap.add_argument("--no-metrics", action="store_true")
    ap.add_argument("--net", default="yolo", choices=["rtpose", "yolo"], help="the box stage; Yolo-A2J takes YoloPoseNet's boxes, so only 'yolo'")
    ap.add_argument("--pipeline", type=int, default=1, help="accepted, not used: the two stages run one batch at a time")
    ap.add_argument("--gpus", type=int, default=1, help="only 1: the box rows of a frame and its crops stay on one GPU")
    ap.add_argument("--ablation", action="store_true", help="refused: the depth-ablation arms exist for Open-Pose+ only")
    args = ap.parse_args(argv)
    if args.net != "yolo":
        ap.error("--net %s: the Yolo-A2J baseline takes its boxes from YoloPoseNet (--net yolo)" % args.net)
    if args.ablation:
        ap.error("--ablation applies to scripts/evaluate_mpreal.py --net rtpose only")
    if args.gpus != 1:
        ap.error("--gpus %d: this script runs on one GPU" % args.gpus)
    if args.pipeline != 1:
        print("--pipeline %d ignored: the box stage and the A2J stage run one batch at a time" % args.pipeline)

    import popnet_amd  # noqa: F401
    from popnet_amd import dataset, metrics
    from popnet_amd.pipeline import A2JEngine, YoloEngine, lists_from_a2j_records, yolo_box_rows
    import numpy as np

    dev = torch.device("cuda", torch.cuda.current_device())
    frames = dataset.MP3DHPFrames(args.image_dir, args.annotations)
    yolo = YoloEngine(precision=args.precision, state_dict=_state_dict(args.weight), device=dev, max_batch=args.batch_size, input_size=args.input_size,
                      w_org=args.w_org, h_org=args.h_org, intrinsics=frames.intrinsics)
    a2j = A2JEngine(precision=args.precision, state_dict=_state_dict(args.a2j_weight), device=dev, max_batch=args.batch_size, crop=args.crop,
                    intrinsics=frames.intrinsics)
    n = len(frames)
    if args.drop_last:
        n -= n % args.batch_size
    data = {"human_pred_set_2d": [], "human_pred_set_3d": [], "human_pred_set_part_conf": []}
    for chunk, host in frames.batches(list(range(n)), args.batch_size):
        depth = torch.from_numpy(host).to(dev)
        rows = yolo_box_rows(yolo.predict_host(depth))
        p2, p3, pc = lists_from_a2j_records(a2j.predict_host(depth, rows), len(chunk))
        data["human_pred_set_2d"] += p2
        data["human_pred_set_3d"] += p3
        data["human_pred_set_part_conf"] += pc
    g2, g3 = frames.ground_truth()
    data["human_gt_set_2d"], data["human_gt_set_3d"] = g2[:n], g3[:n]
    os.makedirs(args.output_dir, exist_ok=True)
    path = os.path.join(args.output_dir, "eval_data.json")
    json.dump(data, open(path, "w"), indent=4)
    print("wrote %s (%d frames, %s, drop_last=%s)" % (path, n, args.precision, args.drop_last))
    if args.no_metrics:
        return None
    gt = os.path.join(args.output_dir, "labels_used.json")
    json.dump({k: frames.anno_dic[k] for k in ["intrinsics"] * ("intrinsics" in frames.anno_dic) + frames.ids[:n]}, open(gt, "w"))
    return metrics.evaluate_mp_human_3d(gt, path)


if __name__ == "__main__":
    main()
