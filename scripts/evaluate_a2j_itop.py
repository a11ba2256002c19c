#!/usr/bin/env python
"""MI355X drop-in for test() of third_party_methods/A2J_experiments/itop_train_64.py:439-462: the ITOP test split through the trained
A2J net -- crops (pn_a2j_train_crop), A2J_model (pn_a2j_forward), the anchor vote (pn_a2j_vote) -- then the result text file of writeTxt
(one line per frame, 15 x (u, v, depth)) and the error of errorCompute.

    python scripts/evaluate_a2j_itop.py --annotations ITOP_side_test_labels.json --image-dir ITOP_side_test_depth_map \\
        --centres center_test.txt --mean-file itop_side_mean.npy --std-file itop_side_std.npy --weight net_34_....pth --output-dir result/itop64

Where this differs from the reference's script, on purpose: the reference's test loader runs with augment=True and here the crops are
un-augmented (--test-augment 1 reproduces it); the printed error maps the votes back through writeTxt's box, the one the result file
holds, where errorCompute's own box has no width (--reference-error 1 prints its number); a `center_test.txt` line containing `invalid`
drops that frame, where the reference shifts every later centre by one frame; nothing is downloaded.
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--annotations", required=True)
    ap.add_argument("--image-dir", required=True)
    ap.add_argument("--centres", required=True)
    ap.add_argument("--mean-file", required=True)
    ap.add_argument("--std-file", required=True)
    ap.add_argument("--weight", required=True)
    ap.add_argument("--output-dir", default="./result/itop64")
    ap.add_argument("--result-file", default="result_itop64.txt")
    ap.add_argument("--batch-size", type=int, default=32)
    ap.add_argument("--crop", type=int, default=288)
    ap.add_argument("--precision", default="fp32", choices=("fp32", "bf16", "bf16x3"))
    ap.add_argument("--seed", type=int, default=None)
    ap.add_argument("--test-augment", type=int, choices=(0, 1), default=0)
    ap.add_argument("--reference-error", type=int, choices=(0, 1), default=0)
    args = ap.parse_args(argv)

    import popnet_amd  # noqa: F401
    from popnet_amd import a2j_crops, targets
    from popnet_amd.pipeline import A2JEngine, a2j_set_votes

    dev = torch.device("cuda", torch.cuda.current_device())
    if args.seed is not None:
        np.random.seed(args.seed)
    test_set = targets.ItopA2JSet(args.image_dir, args.annotations, args.centres, device=dev)
    eng = A2JEngine(precision=args.precision, state_dict=torch.load(args.weight, map_location="cpu"), device=dev, max_batch=args.batch_size, crop=args.crop)
    eng.cfg.mean, eng.cfg.std = float(np.load(args.mean_file).reshape(-1)[-1]), float(np.load(args.std_file).reshape(-1)[-1])
    sampler = a2j_crops.A2JCropSampler("itop", args.crop, args.crop)
    draw = (lambda n: sampler.draws(n)) if args.test_augment else (lambda n: None)
    votes = a2j_set_votes(eng, lambda idx: test_set.batch(idx, draws=draw(len(idx)), crop=args.crop), len(test_set), args.batch_size)
    os.makedirs(args.output_dir, exist_ok=True)
    result = os.path.join(args.output_dir, args.result_file)
    a2j_crops.write_txt(result, a2j_crops.write_txt_rows(votes, test_set.centres, crop_w=args.crop, crop_h=args.crop))
    error = a2j_crops.error_compute(votes, test_set.keypoints, test_set.centres, as_reference=bool(args.reference_error), crop_w=args.crop, crop_h=args.crop)
    print('Error:', error)
    return dict(votes=votes, error=error, result_file=result, test_set=test_set)


if __name__ == "__main__":
    main()
