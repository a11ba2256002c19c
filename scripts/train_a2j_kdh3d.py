#!/usr/bin/env python
"""MI355X drop-in for the reference's single-person KDH3D A2J trainers third_party_methods/A2J_experiments/train_a2j_base.py and, with
--bg-aug 1, train_a2j_bgaug_new.py: the same files and the hyperparameters that matter, the per-batch body on the GPU -- (the background
swap, pn_compose_bg,) the crop-level augmentation of dataPreprocess / transform as one launch (pn_a2j_train_crop; draws, integer geometry
and labels by popnet_amd.a2j_crops.box_items) -> train-mode forward, A2J_loss, backward, Adam 0.00035 / weight decay 1e-4
(popnet_amd.train_a2j.A2JTrainEngine), StepLR(10, 0.2) stepped by epoch.  After every epoch the test split runs through the eval-mode net,
the 2D accuracy (2 % of the 480 x 512 diagonal) and the 10 cm accuracy of the script are printed and one `.pth` (the reference's 410 keys,
named as the script names it) is written.

    python scripts/train_a2j_kdh3d.py --train-annotations labels_train.json --test-annotations labels_test.json --image-dir depth_maps \\
        --output-dir result [--bg-aug 1 --bg-file labels_bg.json --bg-dir bg_maps --seg-dir seg_maps]

Where this differs from the reference's scripts, on purpose:
  * train_a2j_bgaug_new.py's test loader runs with augment=True; here the test split is un-augmented (--test-augment 1 reproduces it).
    The background of frame i is entry i % (number of backgrounds) of --bg-file, in file order; the reference takes i % 8680.
  * at most 31 crops per replica (A2JTrainEngine); the reference's batch of 64 is --batch-size 64 --gpus 4, or any split into replicas of at
    most 31.  The unused block of normal draws is skipped unless --exact-stream 1.
  * a box whose crop is empty (the reference raises in cv2.resize) drops out of its batch.
  * --gpus N (not measured: no multi-GPU run of this script has been made) needs --seed, so that the ranks agree on the frame order; a
    step in which one rank has no usable crop (the tail of an epoch, empty boxes) is skipped by all ranks together; the replicas' gradients
    are averaged with equal weight even where the last batch of an epoch gives them unequal numbers of crops.
  * the per-step debug images and TensorBoard logs are not written; random_erasing is imported by the reference and never called; nothing is
    downloaded: --weight takes a local `.pth`, otherwise the module's own initialisation is the start (no ImageNet weights).
"""
import argparse
import os
import random
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

REG_LOSS_FACTOR, SPATIAL_FACTOR, RAND_CROP_SHIFT = 3, 0.5, 5


def accuracies(votes, bndbox, keypoints_2d, keypoints_3d, intrinsics, crop, img_wh):
    """train_a2j_base.py:489-519: the votes back in the frame through the RAW box, then the 2D rule and the 10 cm rule.  -> (2D, 3D)"""
    f = np.float32
    x = votes[:, :, 1] * (bndbox[:, 2] - bndbox[:, 0])[:, None] / f(crop) + bndbox[:, 0][:, None]
    y = votes[:, :, 0] * (bndbox[:, 3] - bndbox[:, 1])[:, None] / f(crop) + bndbox[:, 1][:, None]
    z = votes[:, :, 2]
    th = 0.02 * np.sqrt(img_wh[0] ** 2 + img_wh[1] ** 2)
    acc2d = float(np.mean(np.square(x - keypoints_2d[:, :, 0]) + np.square(y - keypoints_2d[:, :, 1]) < np.square(th)))
    X = (x - intrinsics["cx"]) * z / intrinsics["fx"]
    Y = (y - intrinsics["cy"]) * z / intrinsics["fy"]
    d2 = np.square(X - keypoints_3d[:, :, 0]) + np.square(Y - keypoints_3d[:, :, 1]) + np.square(z - keypoints_3d[:, :, 2])
    return acc2d, float(np.mean(d2 < np.square(0.1)))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--train-annotations", required=True)
    ap.add_argument("--test-annotations", required=True)
    ap.add_argument("--image-dir", required=True)
    ap.add_argument("--bg-aug", type=int, choices=(0, 1), default=0, help="1: train_a2j_bgaug_new.py, the background swap on every frame")
    ap.add_argument("--bg-file", default=None)
    ap.add_argument("--bg-dir", default=None)
    ap.add_argument("--seg-dir", default=None)
    ap.add_argument("--output-dir", default=None, help="default ./result, ./bg_result with --bg-aug 1")
    ap.add_argument("--batch-size", type=int, default=31, help="crops per step over all replicas; at most 31 per replica")
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--epochs", type=int, default=None, help="default 35, 100 with --bg-aug 1")
    ap.add_argument("--crop", type=int, default=288)
    ap.add_argument("--seed", type=int, default=None)
    ap.add_argument("--precision", choices=("fp32", "bf16x3"), default="fp32",
                    help="the training step's arithmetic (A2JTrainEngine): exact fp32, or split bf16 on the matrix cores for the stride-1 1x1 and 3x3 convolutions")
    ap.add_argument("--weight", default=None, help="start from this local checkpoint instead of the module's initial state")
    ap.add_argument("--lr", "--learning-rate", type=float, default=0.00035)
    ap.add_argument("--weight-decay", "--wd", type=float, default=1e-4)
    ap.add_argument("--max-steps", type=int, default=None, help="stop every epoch after this many steps")
    ap.add_argument("--print-freq", type=int, default=10)
    ap.add_argument("--test-augment", type=int, choices=(0, 1), default=0)
    ap.add_argument("--exact-stream", type=int, choices=(0, 1), default=0)
    args = ap.parse_args(argv)
    if args.bg_aug and not (args.bg_file and args.bg_dir and args.seg_dir):
        ap.error("--bg-aug 1 needs --bg-file, --bg-dir and --seg-dir")
    epochs = args.epochs if args.epochs is not None else (100 if args.bg_aug else 35)
    output_dir = args.output_dir or ("./bg_result" if args.bg_aug else "./result")

    import popnet_amd  # noqa: F401
    from popnet_amd import launch
    if args.gpus > 1 and not launch.under_torchrun():
        sys.exit(launch.relaunch(os.path.abspath(__file__), sys.argv[1:] if argv is None else list(argv), args.gpus))
    world, rank, local_rank = int(os.environ.get("WORLD_SIZE", "1")), int(os.environ.get("RANK", "0")), int(os.environ.get("LOCAL_RANK", "0"))
    from popnet_amd.train_a2j import MAX_BATCH, A2JTrainEngine
    if args.batch_size % world or not 1 <= args.batch_size // world <= MAX_BATCH:
        ap.error("--batch-size %d over %d replicas: every replica takes the same 1 .. %d crops" % (args.batch_size, world, MAX_BATCH))
    if args.crop % 16:
        ap.error("--crop must be a multiple of 16")
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    if world > 1:
        if args.seed is None:
            ap.error("--gpus %d needs --seed: every rank shuffles the frame order with it, and the ranks must agree on the order" % world)
        import torch.distributed as dist
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        dist.init_process_group(backend="nccl", device_id=dev)
    if args.seed is not None:
        random.seed(args.seed)
        torch.manual_seed(args.seed)
        np.random.seed(args.seed + rank)

    from popnet_amd import a2j_crops, targets
    from popnet_amd.network.a2j import A2J_model
    from popnet_amd.pipeline import A2JEngine, a2j_set_votes

    kw = dict(bg_aug=bool(args.bg_aug), bg_file=args.bg_file, bg_dir=args.bg_dir, seg_dir=args.seg_dir, device=dev, shuffle=False, boxes=True)
    train_set = targets.KDH3DSingleSet(args.image_dir, args.train_annotations, **kw)
    test_set = targets.KDH3DSingleSet(args.image_dir, args.test_annotations, **kw)
    module = A2J_model(15)
    if args.weight:
        module.load_state_dict(torch.load(args.weight, map_location="cpu"))
    eng = A2JTrainEngine.from_module(module, device=dev, lr=args.lr, weight_decay=args.weight_decay, spatial_factor=SPATIAL_FACTOR,
                                     reg_loss_factor=REG_LOSS_FACTOR, world_size=world, precision=args.precision)
    per_rank = args.batch_size // world
    infer = A2JEngine(precision="fp32", state_dict=module.state_dict(), device=dev, max_batch=per_rank, crop=args.crop)      # mean 3, std 2, img 480 x 512
    intrinsics = dict(fx=infer.cfg.fx, fy=infer.cfg.fy, cx=infer.cfg.cx, cy=infer.cfg.cy)
    img_wh = (infer.cfg.img_w, infer.cfg.img_h)
    sampler = a2j_crops.A2JCropSampler("box", args.crop, args.crop, exact_stream=bool(args.exact_stream))
    os.makedirs(output_dir, exist_ok=True)
    losses, accs, votes, path = [], [], None, None
    for epoch in range(epochs):
        order = list(range(len(train_set)))
        random.shuffle(order)
        n_batches = -(-len(order) // args.batch_size)          # the DataLoader keeps the last, smaller batch
        if args.max_steps is not None:
            n_batches = min(n_batches, args.max_steps)
        t0, seen, loss_sum = time.time(), 0, 0.0
        for i in range(n_batches):
            chunk = order[i * args.batch_size:(i + 1) * args.batch_size]
            mine = chunk[rank::world]
            frames, items, labels = train_set.crop_batch(mine, draws=sampler.draws(len(mine)), crop=args.crop, img_wh=img_wh)
            keep = [k for k, it in enumerate(items) if it.sh >= 1 and it.sw >= 1]
            crops, _ = infer.train_crops(frames, items)
            if len(keep) < len(mine):
                crops, labels = crops[keep].contiguous(), labels[keep]
            usable = len(keep) * (args.crop // 16) ** 2 >= 2
            if world > 1:          # a step is a collective (the gradient all-reduce): every rank takes it, or none does
                ok = torch.tensor([int(usable)], device=dev)
                dist.all_reduce(ok, op=dist.ReduceOp.MIN)
                usable = bool(ok.item())
            if not usable:
                continue
            terms = eng.step(crops, torch.from_numpy(labels).to(dev)).cpu().tolist()
            loss = terms[0] + REG_LOSS_FACTOR * terms[1]
            losses.append(loss)
            seen += len(keep)
            loss_sum += loss * len(keep)
            if i % args.print_freq == 0 and rank == 0:
                print('epoch: ', epoch, ' step: ', i, 'Cls_loss ', terms[0], 'Reg_loss ', terms[1], ' total loss ', loss)
        if rank == 0:
            print('==> time to learn 1 sample = %f (ms)' % ((time.time() - t0) / max(seen, 1) * 1000))
            print('mean train_loss_add of 1 sample: %f, #train_indexes = %d' % (loss_sum / max(seen, 1), seen))
        eng.lr = args.lr * 0.2 ** (epoch // 10)         # lr_scheduler.StepLR(step_size=10, gamma=0.2) after scheduler.step(epoch)
        if rank == 0:
            sd = eng.state_dict()
            infer.model.load_state_dict(sd)
            draw = (lambda n: sampler.draws(n)) if args.test_augment else (lambda n: None)
            votes = a2j_set_votes(infer, lambda idx: test_set.crop_batch(idx, draws=draw(len(idx)), crop=args.crop, img_wh=img_wh), len(test_set), per_rank)
            acc2d, acc3d = accuracies(votes, test_set.bndbox, test_set.keypoints_2d, test_set.keypoints_3d, intrinsics, args.crop, img_wh)
            accs.append((acc2d, acc3d))
            print("Accuracy 2d:", acc2d)
            print('Accuracy:', acc3d)
            path = '%s/net_%d_wetD_' % (output_dir, epoch) + str(args.weight_decay) + '_depFact_' + str(SPATIAL_FACTOR) + '_RegFact_' + str(
                REG_LOSS_FACTOR) + '_rndShft_' + str(RAND_CROP_SHIFT) + '.pth'
            torch.save(sd, path)
    return dict(losses=losses, accuracies=accs, votes=votes, checkpoint=path, test_set=test_set)


if __name__ == "__main__":
    main()
