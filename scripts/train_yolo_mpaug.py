#!/usr/bin/env python
"""MI355X drop-in for the reference's trainer third_party_methods/train_yolo_posenet_kdh3d_mpaug.py (CR line endings): same data
layout and the command-line arguments that matter, the whole per-batch body on the GPU -- multi-person composition + prior targets
(popnet_amd.targets.mpaug_batch_yolo) -> train-mode forward, yolo_loss_fgweight_poseweight (--rarity-weight 1, the default) or
yolo_loss_fgweight, backward, Nesterov SGD (popnet_amd.train_yolo.YoloTrainEngine) -- validation loss per epoch,
ReduceLROnPlateau and the best checkpoint saved as `best_pose.pth` with the DataParallel `module.` prefix the evaluation scripts
expect.  Built like scripts/train_mpaug.py (and reuses its Plateau).  The annotations need `bbox` and `pose_weight` per person.

    python scripts/train_yolo_mpaug.py --train-annotations labels_train_*.json --val-annotations labels_test_*.json \
        --image-dir depth_maps --bg-file labels_bg.json --bg-dir bg_maps --seg-dir seg_maps --output-dir out [--epochs 200]

`--augment 1` / `--max-aug-ratio` as in train_mpaug.py: the reference's random Rotate / RenderDepth / Crop on the training batches
(:290-297 of the reference's trainer), boxes shifted and scaled with the joints but not rotated; validation never augments.

Not reproduced: hipGraph capture of the step; several GPUs.
"""
import argparse
import os
import random
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from train_mpaug import Plateau  # noqa: E402

ANCHORS = [(6., 3.), (12., 6.)]


def eval_loss(module, batch, rarity_weight):
    """Validation loss as the reference's validate(): eval-mode forward, the same loss, no update."""
    from popnet_amd.network.losses import yolo_loss_fgweight, yolo_loss_fgweight_poseweight
    img, prior, conf, coord, weight = batch
    with torch.no_grad():
        pred = module(img)
        if rarity_weight:
            total, _ = yolo_loss_fgweight_poseweight(pred, prior, conf, coord, weight, module.num_parts, len(module.anchors))
        else:
            total = yolo_loss_fgweight(pred, prior, conf, coord, module.num_parts, len(module.anchors))
    return float(total)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--train-annotations", nargs="+", required=True)
    ap.add_argument("--val-annotations", nargs="+", default=None)
    ap.add_argument("--image-dir", required=True)
    ap.add_argument("--bg-file", required=True)
    ap.add_argument("--bg-dir", required=True)
    ap.add_argument("--seg-dir", required=True)
    ap.add_argument("--output-dir", default="./trained_model/yolo_posenet_kdh3d_mpaug")
    ap.add_argument("--batch-size", type=int, default=30)
    ap.add_argument("--lr", "--learning-rate", type=float, default=1.0)
    ap.add_argument("--momentum", type=float, default=0.9)
    ap.add_argument("--weight-decay", "--wd", type=float, default=0.0)
    ap.add_argument("--epochs", type=int, default=200)
    ap.add_argument("--square-edge", type=int, default=224)
    ap.add_argument("--num-parts", type=int, default=15)
    ap.add_argument("--rarity-weight", type=int, default=1)
    ap.add_argument("--print-freq", type=int, default=20)
    ap.add_argument("--seed", type=int, default=None)
    ap.add_argument("--weight", default=None, help="start from this checkpoint instead of the module's initial state")
    ap.add_argument("--augment", type=int, choices=(0, 1), default=0, help="1: random Rotate / RenderDepth / Crop on the training batches (the reference's training transform)")
    ap.add_argument("--max-aug-ratio", type=float, default=1.7, help="RenderDepth's max_ratio (the reference's --max_aug_ratio)")
    args = ap.parse_args(argv)

    import popnet_amd  # noqa: F401
    from popnet_amd import targets
    from popnet_amd.network.yolo_posenet import YoloPoseNet
    from popnet_amd.train_yolo import LOSS_NAMES, YoloTrainEngine

    dev = torch.device("cuda", torch.cuda.current_device())
    if args.seed is not None:
        random.seed(args.seed)
        torch.manual_seed(args.seed)
    train_set = targets.MPAugTrainSet(args.image_dir, args.train_annotations, args.bg_file, args.bg_dir, args.seg_dir, device=dev)
    val_set = targets.MPAugTrainSet(args.image_dir, args.val_annotations, args.bg_file, args.bg_dir, args.seg_dir, device=dev, shuffle=False) if args.val_annotations else None
    module = YoloPoseNet(args.num_parts, input_dim=1, anchors=ANCHORS)
    if args.weight:
        module.load_state_dict(torch.load(args.weight, map_location="cpu"))
    eng = YoloTrainEngine.from_module(module, device=dev, lr=args.lr, momentum=args.momentum, weight_decay=args.weight_decay,
                                      rarity_weight=bool(args.rarity_weight))
    module = module.to(dev).eval()
    module.precision = "fp32"
    rw = bool(args.rarity_weight)

    def make(ds, idx, augment=False):
        if augment:
            *parts, aug = ds.batch(idx, with_boxes=True, input_size=args.square_edge, augment=True, max_aug_ratio=args.max_aug_ratio)
        else:
            parts, aug = ds.batch(idx, with_boxes=True, input_size=args.square_edge), None
        return [t.contiguous() for t in targets.mpaug_batch_yolo(*parts, input_size=args.square_edge, aug=aug)]

    plateau, best = Plateau(), float("inf")
    os.makedirs(args.output_dir, exist_ok=True)
    for epoch in range(args.epochs):
        order = list(range(len(train_set)))
        random.shuffle(order)
        n_batches = len(order) // args.batch_size     # drop_last=True
        t0, run = time.time(), 0.0
        for i in range(n_batches):
            img, prior, conf, coord, weight = make(train_set, order[i * args.batch_size:(i + 1) * args.batch_size], augment=bool(args.augment))
            terms = eng.step(img, prior, conf, coord, weight if rw else None)
            if i % args.print_freq == 0:
                tl = terms.cpu().tolist()
                run = tl[0]
                print("Epoch: [%d][%d/%d]\tLoss %.4f\t%s\t(%.1f frames/s)" % (epoch, i, n_batches, run, "  ".join("%s %.4f" % (n, v) for n, v in zip(LOSS_NAMES, tl)),
                                                                              (i + 1) * args.batch_size / max(time.time() - t0, 1e-9)))
        val = run
        if val_set is not None:
            module.load_state_dict(eng.state_dict())
            module.eval()
            vals = [eval_loss(module, make(val_set, list(range(s, s + args.batch_size))), rw)
                    for s in range(0, len(val_set) - args.batch_size + 1, args.batch_size)]
            val = sum(vals) / max(len(vals), 1)
        eng.lr = plateau.step(val, eng.lr)
        print("Epoch %d: val loss %.5f  lr %.4g" % (epoch, val, eng.lr))
        if val < best:
            best = val
            torch.save(eng.state_dict(prefix="module."), os.path.join(args.output_dir, "best_pose.pth"))
    return best


if __name__ == "__main__":
    main()
