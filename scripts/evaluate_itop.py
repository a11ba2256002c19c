#!/usr/bin/env python
"""MI355X drop-in for the reference's ITOP evaluation scripts (third_party_methods/evaluate/evaluation_rtpose_light3d_itop.py and
evaluation_yolo_posenet_itop.py): the same arguments that matter, the same ``eval_data.json`` keys in --output-dir, the same 2D and 3D
tables (popnet_amd.metrics.eval_human_dataset_2d at 2 % of the frame diagonal, eval_human_dataset_3d at 10 cm) and, like the first
script, ``eval_res2d.json`` / ``eval_res3d.json``.

    python scripts/evaluate_itop.py --net rtpose --annotations annotations/ITOP_side_test_labels.json \
        --image-dir ITOP_side_test_depth_map --weight best_pose.pth --output-dir out [--precision fp32|bf16] [--batch-size 15]

--net rtpose: every parsed person goes into the lists; a joint's depth is the one pose-depth cell under its peak (channel joint2chn[j]),
read in network-input pixels for visible joints only -- the ITOP profile's read-out in the parse kernels.  --net yolo: conf_threshold 0.1,
the first person of the prior parse or the script's -1 placeholder, depth from the prior pose.  Both flip 3D Y (the profile's fy = -f).
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--net", required=True, choices=["rtpose", "yolo"])
    ap.add_argument("--annotations", "--val-annotations", dest="annotations", required=True)
    ap.add_argument("--image-dir", "--val-image-dir", dest="image_dir", required=True)
    ap.add_argument("--weight", required=True, help="reference checkpoint (state_dict, 'module.'-prefixed or not)")
    ap.add_argument("--output-dir", required=True)
    ap.add_argument("--batch-size", type=int, default=15)
    ap.add_argument("--input-size", type=int, default=224)
    ap.add_argument("--precision", default="fp32", choices=["fp32", "bf16"], help="fp32 = parity mode, bf16 = throughput mode")
    ap.add_argument("--drop-last", action="store_true", help="skip the tail like the reference's drop_last=True loader")
    ap.add_argument("--no-metrics", action="store_true")
    return ap.parse_args(argv)


def print_table(kind, unit, th, names, kcp, dist):
    print('\nevaluation result of %s poses:' % kind)
    print('     %s threshold: %03f%s' % (kind, th, ' meter' if kind == '3D' else ''))
    for i, name in enumerate(names):
        print('     joint: {},  PCK: {:03f}, avg {} error: {:03f}'.format(name, kcp[i], unit, dist[i]))
    print('\n     Overall: PCK: {:03f}, avg {} error: {:03f} \n'.format(np.average(kcp), unit, np.average(dist)))


def main(argv=None):
    args = parse_args(argv)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("evaluate_itop.py needs a GPU: the HIP path has no CPU fallback")
    import popnet_amd  # noqa: F401
    from popnet_amd import dataset, metrics, targets
    from popnet_amd.pipeline import PoseEngine, YoloEngine
    from popnet_amd.profiles import ITOP

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    frames = targets.ItopSet(args.image_dir, args.annotations, device=dev, profile=ITOP)
    sd = torch.load(args.weight, map_location="cpu")
    sd = {(k[len("module."):] if k.startswith("module.") else k): v for k, v in sd.items()}
    kw = dict(precision=args.precision, state_dict=sd, device=dev, max_batch=args.batch_size, input_size=args.input_size, profile=ITOP)
    eng = PoseEngine(**kw) if args.net == "rtpose" else YoloEngine(conf_threshold=0.1, **kw)
    if args.net == "rtpose":
        # the lists, batch by batch: a frame whose fixed-size record overflows is parsed again without capacities (predict_lists)
        n = len(frames) - (len(frames) % args.batch_size if args.drop_last else 0)
        data = {"human_pred_set_2d": [], "human_pred_set_3d": [], "visibility_pred_set": []}
        for chunk, host in frames.batches(range(n), args.batch_size):
            lists = eng.predict_lists(torch.from_numpy(host).to(dev))
            for k in data:
                data[k] += lists[k]
    else:
        recs = dataset.run_sweep(eng, frames, args.batch_size, drop_last=args.drop_last)
        data = dataset.yolo_records_to_lists(recs, profile=ITOP)
        n = len(recs)
    g2, g3 = frames.ground_truth()
    data["human_gt_set_2d"], data["human_gt_set_3d"] = g2[:n], g3[:n]
    os.makedirs(args.output_dir, exist_ok=True)
    path = os.path.join(args.output_dir, "eval_data.json")
    json.dump(data, open(path, "w"), indent=4)
    print("wrote %s (%d frames, %s)" % (path, n, args.precision))
    if args.no_metrics:
        return None
    th = ITOP.dist_th_2d()
    d2, k2 = metrics.eval_human_dataset_2d(data["human_pred_set_2d"], data["human_gt_set_2d"], num_joints=15, dist_th=th, iou_th=0.5)
    print_table('2D', '2D', th, ITOP.keypoints, k2, d2)
    json.dump({'dist_th_2d': th, 'joint_names': ITOP.keypoints, 'joint_avg_2d_error': d2, 'joint_KCP': k2, 'overall_avg_2d_error': np.average(d2),
               'overall_KCP': np.average(k2)}, open(os.path.join(args.output_dir, 'eval_res2d.json'), 'w'), indent=4)
    print('evaluating in 3D...')
    d3, k3 = metrics.eval_human_dataset_3d(data["human_pred_set_2d"], data["human_gt_set_2d"], data["human_pred_set_3d"], data["human_gt_set_3d"],
                                           num_joints=15, dist_th=0.1, iou_th=0.5)
    print_table('3D', '3D', 0.1, ITOP.keypoints, k3, d3)
    json.dump({'dist_th_3d': 0.1, 'joint_names': ITOP.keypoints, 'joint_avg_3d_error': d3, 'joint_KCP': k3, 'overall_avg_3d_error': np.average(d3),
               'overall_KCP': np.average(k3)}, open(os.path.join(args.output_dir, 'eval_res3d.json'), 'w'), indent=4)
    return {"pck2d": k2, "err2d": d2, "pck3d": k3, "err3d": d3}


if __name__ == "__main__":
    main()
