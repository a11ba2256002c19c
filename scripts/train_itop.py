#!/usr/bin/env python
"""MI355X drop-in for the reference's two ITOP trainers, third_party_methods/train_rtpose_light3d_itop.py (--net rtpose) and
train_yolo_posenet_itop.py (--net yolo): the ITOP data layout, their hyperparameters (batch 30, lr 1, momentum 0.9, Nesterov, no weight
decay, 100 epochs, ReduceLROnPlateau(0.8, patience 5, cooldown 3); yolo: the pose-weighted loss), the whole per-batch body on the GPU --
frames as they are (no composition), the random transform Compose([Cvt2ndarray, Rotate(), RenderDepth(), Hflip(swap), Crop(), Resize])
as one launch (popnet_amd.targets.itop_batch / itop_batch_yolo), then the train-mode forward, loss, backward and Nesterov SGD of
popnet_amd.train.TrainEngine / popnet_amd.train_yolo.YoloTrainEngine -- a validation loss per epoch (evaluation transform) and the best
checkpoint as `best_pose.pth` with the DataParallel `module.` prefix, which scripts/evaluate_itop.py loads.

    python scripts/train_itop.py --net rtpose --train-annotations annotations/ITOP_side_train_labels.json --train-image-dir ITOP_side_train_depth_map \
        --val-annotations annotations/ITOP_side_test_labels.json --val-image-dir ITOP_side_test_depth_map --output-dir out [--epochs 100]

`--augment 0` trains on the evaluation transform (Cvt2ndarray + Resize) instead.
"""
import argparse
import os
import random
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

ANCHORS = [(6., 3.), (12., 6.)]


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--net", required=True, choices=["rtpose", "yolo"])
    ap.add_argument("--train-annotations", required=True)
    ap.add_argument("--train-image-dir", required=True)
    ap.add_argument("--val-annotations", default=None)
    ap.add_argument("--val-image-dir", default=None)
    ap.add_argument("--output-dir", default=None, help="default ./trained_model/rtpose_light3d_itop or ./trained_model/yolo_posenet_itop")
    ap.add_argument("--batch-size", type=int, default=30)
    ap.add_argument("--lr", "--learning-rate", type=float, default=1.0)
    ap.add_argument("--momentum", type=float, default=0.9)
    ap.add_argument("--weight-decay", "--wd", type=float, default=0.0)
    ap.add_argument("--epochs", type=int, default=100)
    ap.add_argument("--square-edge", type=int, default=224)
    ap.add_argument("--z-radius", type=int, default=2, help="--net rtpose: half width of the z-map window")
    ap.add_argument("--rarity-weight", type=int, default=1, help="--net yolo: 1 = the pose-weighted loss")
    ap.add_argument("--print-freq", type=int, default=20)
    ap.add_argument("--seed", type=int, default=None)
    ap.add_argument("--weight", default=None, help="start from this checkpoint instead of the module's initial state")
    ap.add_argument("--augment", type=int, choices=(0, 1), default=1, help="1: Rotate / RenderDepth / Hflip / Crop on the training batches, as both trainers do")
    args = ap.parse_args(argv)
    if (args.val_annotations is None) != (args.val_image_dir is None):
        ap.error("--val-annotations and --val-image-dir go together")
    if args.output_dir is None:
        args.output_dir = "./trained_model/" + ("rtpose_light3d_itop" if args.net == "rtpose" else "yolo_posenet_itop")
    return args


def main(argv=None):
    args = parse_args(argv)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("train_itop.py needs a GPU: the HIP path has no CPU fallback")
    import popnet_amd  # noqa: F401
    from popnet_amd import targets
    from popnet_amd.profiles import ITOP
    from train_mpaug import Plateau, eval_loss as rtpose_eval_loss
    from train_yolo_mpaug import eval_loss as yolo_eval_loss

    dev = torch.device("cuda", torch.cuda.current_device())
    if args.seed is not None:
        random.seed(args.seed)
        torch.manual_seed(args.seed)
    S, rw = args.square_edge, bool(args.rarity_weight)
    train_set = targets.ItopSet(args.train_image_dir, args.train_annotations, device=dev, profile=ITOP)
    val_set = targets.ItopSet(args.val_image_dir, args.val_annotations, device=dev, profile=ITOP) if args.val_annotations else None
    if args.net == "rtpose":
        from popnet_amd.network.rtpose_light3d import rtpose_light3d
        from popnet_amd.train import LOSS_NAMES, TrainEngine
        module = rtpose_light3d(15, 14, 2, input_dim=1)
    else:
        from popnet_amd.network.yolo_posenet import YoloPoseNet
        from popnet_amd.train_yolo import LOSS_NAMES, YoloTrainEngine
        module = YoloPoseNet(15, input_dim=1, anchors=ANCHORS)
    if args.weight:
        module.load_state_dict(torch.load(args.weight, map_location="cpu"))
    if args.net == "rtpose":
        eng = TrainEngine.from_module(module, device=dev, lr=args.lr, momentum=args.momentum, weight_decay=args.weight_decay)
    else:
        eng = YoloTrainEngine.from_module(module, device=dev, lr=args.lr, momentum=args.momentum, weight_decay=args.weight_decay, rarity_weight=rw)
    module = module.to(dev).eval()
    module.precision = "fp32"

    def make(ds, idx, augment=False):
        frames, k2, k3, _, pw, *rest = ds.batch(idx, input_size=S, augment=augment)
        aug = rest[0] if rest else None
        if args.net == "rtpose":
            out = targets.itop_batch(frames, k2, k3, input_size=S, z_radius=args.z_radius, aug=aug, profile=ITOP)
        else:
            out = targets.itop_batch_yolo(frames, k2, k3, pw, input_size=S, aug=aug, profile=ITOP)
        return [t.contiguous() for t in out]

    def step(batch):
        if args.net == "rtpose":
            return eng.step(*batch)
        img, prior, conf, coord, weight = batch
        return eng.step(img, prior, conf, coord, weight if rw else None)

    plateau, best = Plateau(), float("inf")
    os.makedirs(args.output_dir, exist_ok=True)
    for epoch in range(args.epochs):
        order = list(range(len(train_set)))
        random.shuffle(order)
        n_batches = len(order) // args.batch_size     # drop_last=True
        t0, run = time.time(), 0.0
        for i in range(n_batches):
            terms = step(make(train_set, order[i * args.batch_size:(i + 1) * args.batch_size], augment=bool(args.augment)))
            if i % args.print_freq == 0:
                tl = terms.cpu().tolist()
                run = sum(tl) if args.net == "rtpose" else tl[0]
                print("Epoch: [%d][%d/%d]\tLoss %.4f\t%s\t(%.1f frames/s)" % (epoch, i, n_batches, run, "  ".join("%s %.4f" % (n, v) for n, v in zip(LOSS_NAMES, tl)),
                                                                              (i + 1) * args.batch_size / max(time.time() - t0, 1e-9)))
        val = run
        if val_set is not None:
            module.load_state_dict(eng.state_dict())
            module.eval()
            vals = []
            for s in range(0, len(val_set) - args.batch_size + 1, args.batch_size):
                batch = make(val_set, list(range(s, s + args.batch_size)))
                vals.append(rtpose_eval_loss(module, batch) if args.net == "rtpose" else yolo_eval_loss(module, batch, rw))
            val = sum(vals) / max(len(vals), 1)
        eng.lr = plateau.step(val, eng.lr)
        print("Epoch %d: val loss %.5f  lr %.4g" % (epoch, val, eng.lr))
        if val < best:
            best = val
            torch.save(eng.state_dict(prefix="module."), os.path.join(args.output_dir, "best_pose.pth"))
    return best


if __name__ == "__main__":
    main()
