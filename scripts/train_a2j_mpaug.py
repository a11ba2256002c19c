#!/usr/bin/env python
"""MI355X drop-in for the reference's trainer third_party_methods/A2J_experiments/train_a2j_mpaug_new.py: the same data layout and the
hyperparameters that matter, the whole per-batch body on the GPU -- multi-person composition (popnet_amd.targets.MPAugTrainSet /
compose_depth), the random Rotate / RenderDepth / Resize of the training batches (pn_augment_resize), one person per frame cropped to
288 x 288 (pn_a2j_crop: img 480 x 512 in the reference, mean 3, std 2), its label by popnet_amd.train_a2j.crop_labels -> train-mode forward,
A2J_loss, backward, Adam (popnet_amd.train_a2j.A2JTrainEngine) -- a validation loss per epoch through the eval-mode module and
popnet_amd.network.a2j.A2J_loss, StepLR(10, 0.2) stepped by epoch, and one `.pth` per epoch (the reference's 410 keys) that
A2J_model.load_state_dict and scripts/evaluate_mpreal_a2j.py accept.

    python scripts/train_a2j_mpaug.py --train-annotations labels_train_*.json --val-annotations labels_test_*.json \\
        --image-dir depth_maps --bg-file labels_bg.json --bg-dir bg_maps --seg-dir seg_maps --output-dir out [--epochs 200]

Where this differs from the reference's script, on purpose:
  * frames are resized to --frame-size x --frame-size (512, square: the augmentation kernel's Resize) instead of 480 x 512; the boxes and
    joints scale with them and every box is resampled to the crop size afterwards, so a crop shows the same person at the same scale.  The
    augmentation's Crop runs with zero fractions (it still drops the frame's last row and column, as data_augmentation_2d3d.Crop does).
  * one RANDOM person per frame gives both the crop and the label.  (The reference's dataPreprocess draws a random index as well, but every
    entry of its image and label lists aliases one buffer, so it always trains on the frame's LAST person.)  A person whose box is empty
    after the augmentation is skipped; a frame without a usable person drops out of its batch.
  * at most 31 crops per step (A2JTrainEngine); the reference's batch of 64 needs data-parallel replicas, which this script does not start.
  * nothing is downloaded: --weight takes a local `.pth`, otherwise the module's own initialisation is the start (no ImageNet weights).
  * random_erasing is imported by the reference and never called; the validation set is not augmented.
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


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--train-annotations", nargs="+", required=True)
    ap.add_argument("--val-annotations", nargs="+", default=None)
    ap.add_argument("--image-dir", required=True)
    ap.add_argument("--bg-file", required=True)
    ap.add_argument("--bg-dir", required=True)
    ap.add_argument("--seg-dir", required=True)
    ap.add_argument("--output-dir", default="./mp_result")
    ap.add_argument("--batch-size", type=int, default=31)
    ap.add_argument("--lr", "--learning-rate", type=float, default=0.00035)
    ap.add_argument("--weight-decay", "--wd", type=float, default=1e-4)
    ap.add_argument("--spatial-factor", type=float, default=0.5)
    ap.add_argument("--reg-loss-factor", type=float, default=3)
    ap.add_argument("--epochs", type=int, default=200)
    ap.add_argument("--frame-size", type=int, default=512)
    ap.add_argument("--crop", type=int, default=288)
    ap.add_argument("--num-classes", type=int, default=15)
    ap.add_argument("--print-freq", type=int, default=10)
    ap.add_argument("--seed", type=int, default=None)
    ap.add_argument("--precision", choices=("fp32", "bf16x3"), default="fp32",
                    help="the training step's arithmetic (A2JTrainEngine): exact fp32, or split bf16 on the matrix cores for the stride-1 1x1 and 3x3 convolutions")
    ap.add_argument("--weight", default=None, help="start from this local checkpoint instead of the module's initial state")
    ap.add_argument("--augment", type=int, choices=(0, 1), default=1, help="1: random Rotate / RenderDepth on the training batches (the reference's preprocess)")
    ap.add_argument("--max-aug-ratio", type=float, default=1.7, help="RenderDepth's max_ratio")
    args = ap.parse_args(argv)

    import popnet_amd  # noqa: F401
    from popnet_amd import targets
    from popnet_amd.network.a2j import A2J_loss, A2J_model
    from popnet_amd.pipeline import A2JEngine
    from popnet_amd.train_a2j import MAX_BATCH, A2JTrainEngine, crop_labels

    if not 1 <= args.batch_size <= MAX_BATCH:
        ap.error("--batch-size must be 1 .. %d (the BatchNorm primitives take N * C <= 65535 and layer4 has 2048 channels)" % MAX_BATCH)
    if args.crop % 16:
        ap.error("--crop must be a multiple of 16")
    dev = torch.device("cuda", torch.cuda.current_device())
    if args.seed is not None:
        random.seed(args.seed)
        torch.manual_seed(args.seed)
    S = args.frame_size
    train_set = targets.MPAugTrainSet(args.image_dir, args.train_annotations, args.bg_file, args.bg_dir, args.seg_dir, device=dev)
    val_set = targets.MPAugTrainSet(args.image_dir, args.val_annotations, args.bg_file, args.bg_dir, args.seg_dir, device=dev, shuffle=False) if args.val_annotations else None
    module = A2J_model(args.num_classes)
    if args.weight:
        module.load_state_dict(torch.load(args.weight, map_location="cpu"))
    eng = A2JTrainEngine.from_module(module, device=dev, lr=args.lr, weight_decay=args.weight_decay, spatial_factor=args.spatial_factor,
                                     reg_loss_factor=args.reg_loss_factor, precision=args.precision)
    module = module.to(dev).eval()
    module.precision = "fp32"
    cropper = A2JEngine(precision="fp32", state_dict=module.state_dict(), device=dev, max_batch=1, crop=args.crop, img_wh=(S, S))      # its crops() only: pn_a2j_crop
    criterion = A2J_loss(shape=[args.crop // 16, args.crop // 16], thres=[16.0, 32.0], stride=16, spatialFactor=args.spatial_factor,
                         img_shape=[args.crop, args.crop], P_h=None, P_w=None)

    def make(ds, idx, augment):
        """-> (crops [n, 1, crop, crop], labels [n, P, 3]) on the device, n <= len(idx)"""
        if augment:
            fd, fm, n_src, bg, k2, k3, npers, boxes, _, aug = ds.batch(idx, with_boxes=True, input_size=S, augment=True, max_aug_ratio=args.max_aug_ratio)
            for it in aug.items:            # Rotate and RenderDepth as drawn; the reference's A2J preprocess has no Crop
                it.update(targets.augmentation(it["rot"], it["a"], (0.0, 0.0, 0.0, 0.0), it["H"], it["W"], it["cx"], it["cy"], S))
            aug = targets.AugmentationBatch(aug.items)
            frames = targets.augment_resize(targets.compose_depth(fd, fm, n_src, bg), aug, S, targets.DEPTH_MAX)[:, 0]
            kp, kz, bx = aug.transform_labels(k2, k3, boxes)
        else:
            fd, fm, n_src, bg, k2, k3, npers, boxes, _ = ds.batch(idx, with_boxes=True, input_size=S)
            image = targets.compose_depth(fd, fm, n_src, bg)
            H, W = image.shape[1:]
            frames = targets._resize(image, S, targets.DEPTH_MAX)
            kp = k2.cpu().numpy().astype(np.float32)
            kp[..., 0] *= float(S) / W
            kp[..., 1] *= float(S) / H
            kz, bx = k3.cpu().numpy()[..., 2], boxes.cpu().numpy()
        rows, labels = [], []
        for b, n in enumerate(npers.cpu().tolist()):
            for p in random.sample(range(n), n):
                x0, y0, x1, y1 = (float(v) for v in bx[b, p])
                if int(x1 - x0) < 1 or int(y1 - y0) < 1 or min(x1, S - 1) <= max(x0, 0) + 1 or min(y1, S - 1) <= max(y0, 0) + 1:
                    continue                # nothing of the box is left in the frame
                rows.append([b, x0, y0, x1, y1, 1.0])
                labels.append(crop_labels((x0, y0, x1, y1), kp[b, p], np.stack([kp[b, p, :, 0], kp[b, p, :, 1], kz[b, p]], 1), frame_shape=(S, S),
                                          crop_w=args.crop, crop_h=args.crop))
                break
        if not rows:
            return None, None
        crops, _ = cropper.crops(frames.contiguous(), np.asarray(rows, np.float32))
        return crops, torch.from_numpy(np.stack(labels)).to(dev)

    def eval_loss(crops, labels):
        with torch.no_grad():
            c, r = criterion(module(crops), labels)
        return float(c + args.reg_loss_factor * r)

    os.makedirs(args.output_dir, exist_ok=True)
    last_val = float("nan")
    for epoch in range(args.epochs):
        order = list(range(len(train_set)))
        random.shuffle(order)
        n_batches = max(len(order) // args.batch_size, 1)
        t0, seen, loss_sum = time.time(), 0, 0.0
        for i in range(n_batches):
            crops, labels = make(train_set, order[i * args.batch_size:(i + 1) * args.batch_size], bool(args.augment))
            if crops is None or crops.shape[0] * (args.crop // 16) ** 2 < 2:
                continue
            terms = eng.step(crops, labels).cpu().tolist()
            loss = terms[0] + args.reg_loss_factor * terms[1]
            seen += crops.shape[0]
            loss_sum += loss * crops.shape[0]
            if i % args.print_freq == 0:
                print("epoch:  %d  step:  %d / %d Cls_loss  %.4f Reg_loss  %.4f  total loss  %.4f  (%.1f crops/s)" % (
                    epoch, i, n_batches, terms[0], terms[1], loss, seen / max(time.time() - t0, 1e-9)))
        print("mean train_loss_add of 1 sample: %f, #train_indexes = %d" % (loss_sum / max(seen, 1), seen))
        sd = eng.state_dict()
        if val_set is not None:
            module.load_state_dict(sd)
            module.eval()
            vs, vn = 0.0, 0
            for s in range(0, len(val_set), args.batch_size):
                crops, labels = make(val_set, list(range(s, min(s + args.batch_size, len(val_set)))), False)
                if crops is not None:
                    vs += eval_loss(crops, labels) * crops.shape[0]
                    vn += crops.shape[0]
            last_val = vs / max(vn, 1)
            print("mean val_loss of 1 sample: %f, #val_indexes = %d" % (last_val, vn))
        torch.save(sd, os.path.join(args.output_dir, "net_%d_wetD_%s_depFact_%s_RegFact_%s.pth" % (epoch, args.weight_decay, args.spatial_factor, args.reg_loss_factor)))
        eng.lr = args.lr * 0.2 ** (epoch // 10)         # lr_scheduler.StepLR(step_size=10, gamma=0.2) after scheduler.step(epoch)
        print("Epoch#%d: train loss=%.4f, val loss=%.4f, lr = %.6f" % (epoch, loss_sum / max(seen, 1), last_val, eng.lr))
    return loss_sum / max(seen, 1), last_val


if __name__ == "__main__":
    main()
