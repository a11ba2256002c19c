#!/usr/bin/env python
"""MI355X drop-in for the reference's ITOP A2J trainer third_party_methods/A2J_experiments/itop_train_64.py: the same files and the
hyperparameters that matter, the per-batch body on the GPU -- the crop-level augmentation of dataPreprocess / transform as one launch
(pn_a2j_train_crop; the draws, the integer geometry and the labels by popnet_amd.a2j_crops) -> train-mode forward, A2J_loss, backward,
Adam 0.00035 / weight decay 1e-4 (popnet_amd.train_a2j.A2JTrainEngine), StepLR(10, 0.2) stepped by epoch.  After every epoch the test
split runs through the eval-mode net (A2JEngine.train_crops + votes), the error of errorCompute is printed and one `.pth` (the
reference's 410 keys, named as the script names it) is written.

    python scripts/train_a2j_itop.py --train-annotations ITOP_side_train_labels.json --train-image-dir ITOP_side_train_depth_map \\
        --train-centres center_train.txt --test-annotations ITOP_side_test_labels.json --test-image-dir ITOP_side_test_depth_map \\
        --test-centres center_test.txt --mean-file itop_side_mean.npy --std-file itop_side_std.npy --output-dir result/itop64

Where this differs from the reference's script, on purpose:
  * the reference's TEST loader runs with augment=True (random offsets, rotation and scale on the test crops); here the test split is
    evaluated un-augmented.  --test-augment 1 reproduces the reference.
  * errorCompute builds its box from the centre WITHOUT +- xy_thres, so every joint maps back to the centre pixel; the printed error uses
    writeTxt's box instead.  --reference-error 1 prints the script's own number (a2j_crops.error_compute(as_reference=True)).
  * a `center_*.txt` line containing `invalid` drops that frame; the reference compacts the centre list only, which pairs every later frame
    and label with the wrong centre.
  * at most 31 crops per replica (A2JTrainEngine: the BatchNorm primitives take N * C <= 65535 and layer4 has 2048 channels); the reference's
    batch of 64 is --batch-size 64 --gpus 4, or any split into replicas of at most 31.
  * the unused block of normal draws is skipped unless --exact-stream 1, which consumes it so that a seeded run meets the stream of a
    single-worker run of the reference.
  * --gpus N (not measured: no multi-GPU run of this script has been made) needs --seed, so that the ranks agree on the frame order; a
    step in which one rank has no usable crop (the tail of an epoch, empty boxes) is skipped by all ranks together; the replicas' gradients
    are averaged with equal weight even where the last batch of an epoch gives them unequal numbers of crops.
  * random_erasing is constructed by the reference and never called.  Nothing is downloaded: --weight takes a local `.pth`, otherwise the
    module's own initialisation is the start (no ImageNet weights).
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

REG_LOSS_FACTOR, SPATIAL_FACTOR, RAND_CROP_SHIFT = 3, 0.5, 5          # RegLossFactor, spatialFactor, RandCropShift (:44-46), also in the file name


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    for split in ("train", "test"):
        ap.add_argument("--%s-annotations" % split, required=True)
        ap.add_argument("--%s-image-dir" % split, required=True)
        ap.add_argument("--%s-centres" % split, required=True)
    ap.add_argument("--mean-file", required=True)
    ap.add_argument("--std-file", required=True)
    ap.add_argument("--output-dir", default="./result/itop64")
    ap.add_argument("--batch-size", type=int, default=31, help="crops per step over all replicas; at most 31 per replica")
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--epochs", type=int, default=35)
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
    ap.add_argument("--reference-error", type=int, choices=(0, 1), default=0)
    ap.add_argument("--exact-stream", type=int, choices=(0, 1), default=0)
    args = ap.parse_args(argv)

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
        random.seed(args.seed)                       # every rank shuffles the order identically, then takes its share of each batch
        torch.manual_seed(args.seed)
        np.random.seed(args.seed + rank)             # the crop draws

    from popnet_amd import a2j_crops, targets
    from popnet_amd.network.a2j import A2J_model
    from popnet_amd.pipeline import A2JEngine, a2j_set_votes

    train_set = targets.ItopA2JSet(args.train_image_dir, args.train_annotations, args.train_centres, device=dev)
    test_set = targets.ItopA2JSet(args.test_image_dir, args.test_annotations, args.test_centres, device=dev)
    module = A2J_model(15)
    if args.weight:
        module.load_state_dict(torch.load(args.weight, map_location="cpu"))
    eng = A2JTrainEngine.from_module(module, device=dev, lr=args.lr, weight_decay=args.weight_decay, spatial_factor=SPATIAL_FACTOR,
                                     reg_loss_factor=REG_LOSS_FACTOR, world_size=world, precision=args.precision)
    per_rank = args.batch_size // world
    infer = A2JEngine(precision="fp32", state_dict=module.state_dict(), device=dev, max_batch=per_rank, crop=args.crop)
    infer.cfg.mean, infer.cfg.std = float(np.load(args.mean_file).reshape(-1)[-1]), float(np.load(args.std_file).reshape(-1)[-1])      # mean[-1], std[-1]
    sampler = a2j_crops.A2JCropSampler("itop", args.crop, args.crop, exact_stream=bool(args.exact_stream))
    os.makedirs(args.output_dir, exist_ok=True)
    losses, errors, votes, path = [], [], None, None
    for epoch in range(args.epochs):
        order = list(range(len(train_set)))
        random.shuffle(order)
        n_batches = -(-len(order) // args.batch_size)          # the DataLoader keeps the last, smaller batch
        if args.max_steps is not None:
            n_batches = min(n_batches, args.max_steps)
        t0, seen, loss_sum = time.time(), 0, 0.0
        for i in range(n_batches):
            chunk = order[i * args.batch_size:(i + 1) * args.batch_size]
            mine = chunk[rank::world]
            frames, items, labels = train_set.batch(mine, draws=sampler.draws(len(mine)), crop=args.crop)
            keep = [k for k, it in enumerate(items) if it.sh >= 1 and it.sw >= 1]          # an empty box: the reference raises there
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
            votes = a2j_set_votes(infer, lambda idx: test_set.batch(idx, draws=draw(len(idx)), crop=args.crop), len(test_set), per_rank)
            error = a2j_crops.error_compute(votes, test_set.keypoints, test_set.centres, as_reference=bool(args.reference_error), crop_w=args.crop, crop_h=args.crop)
            errors.append(error)
            print('epoch: ', epoch, 'Test error:', error)
            path = '%s/net_%d_wetD_' % (args.output_dir, epoch) + str(args.weight_decay) + '_depFact_' + str(SPATIAL_FACTOR) + '_RegFact_' + str(
                REG_LOSS_FACTOR) + '_rndShft_' + str(RAND_CROP_SHIFT) + '.pth'
            torch.save(sd, path)
    return dict(losses=losses, errors=errors, votes=votes, checkpoint=path, test_set=test_set)


if __name__ == "__main__":
    main()
