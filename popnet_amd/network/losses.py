"""The loss of the Open-Pose+ trainer with the reference's signature (tpm/lib/network/losses.py:65-106), so that
tpm/train_rtpose_light3d_kdh3d_mpaug.py:160-180 (CR) runs with the import swapped: per stage the mean squared error of the PAF
and heat maps and the foreground-weighted (0.1 background, 1.0 foreground) mean squared error of the depth maps, summed over
the stages; the log carries the six terms and the extrema the reference prints.  Element-wise torch glue around the outputs of
the HIP primitives (network/_autograd.py); popnet_amd.train.TrainEngine computes the same six terms inside pn_head_forward.
The prior losses of the YoloPoseNet trainer (losses.py:397-466) follow below; popnet_amd.train_yolo.YoloTrainEngine computes them
inside pn_yolo_loss."""
from collections import OrderedDict


def build_names(num_stages=2):
    """losses.py / train_rtpose_light3d_kdh3d_mpaug.py: 'l1_paf', 'l1_heat', 'l1_z', 'l2_paf', ..."""
    names = []
    for j in range(1, num_stages + 1):
        names += ["l%d_paf" % j, "l%d_heat" % j, "l%d_z" % j]
    return names


def rtpose_light3d_loss_fgweight(saved_for_loss, heat_gt, vec_temp, posedepth_temp, fg_mask, num_stages, names):
    log = OrderedDict()
    weight = fg_mask * 0.9 + 0.1
    total = 0
    for j in range(num_stages):
        paf, heat, z = saved_for_loss[3 * j], saved_for_loss[3 * j + 1], saved_for_loss[3 * j + 2]
        terms = (((paf - vec_temp) ** 2).mean(), ((heat - heat_gt) ** 2).mean(), (((z - posedepth_temp) ** 2) * weight).mean())
        for k, t in enumerate(terms):
            total = total + t
            log[names[3 * j + k]] = t.item()
    heat, paf, z = saved_for_loss[-2].detach(), saved_for_loss[-3].detach(), saved_for_loss[-1].detach()
    log["max_ht"], log["min_ht"] = heat[:, 0:-1].max().item(), heat[:, 0:-1].min().item()
    log["max_paf"], log["min_paf"] = paf.max().item(), paf.min().item()
    log["max_z"], log["min_z"] = z.max().item(), z.min().item()
    return total, log


# ---- YoloPoseNet (tpm/lib/network/losses.py:397-466): the prior loss on the cast output of YoloPoseNet in train mode ----
def _prior_views(pred, prior_map_gt, num_anchors, *cell_maps):
    """[b, A(5+3J), h, w] maps -> [b, A, 5+3J, h w]; per-cell maps [b, A, h, w] -> [b, A, 1, h w] (the reference permutes to
    [b, h w, A, .] first: the same elements, and the means below do not depend on the order)."""
    b, _, h, w = pred.shape
    views = [t.reshape(b, num_anchors, -1, h * w) for t in (pred, prior_map_gt)]
    return views + [m.reshape(b, num_anchors, 1, h * w) for m in cell_maps]


def _prior_terms(p, g, m_coord, m_conf, num_joints, weight=None):
    """(coord, obj, selfpose): mean squared errors of the box (x 4), confidence and joint slices (x 3J).  Plain form: the masks weight the
    squared error; pose-weighted form: the masks multiply both sides and the pose weight map weights the squared error."""
    def mse(a, t, m):
        return ((a - t) ** 2 * m).mean() if weight is None else ((a * m - t * m) ** 2 * weight).mean()
    coord = mse(p[:, :, 0:4], g[:, :, 0:4], m_coord) * 4
    obj = mse(p[:, :, 4:5], g[:, :, 4:5], m_conf)
    selfpose = mse(p[:, :, 5:], g[:, :, 5:], m_coord) * 3 * num_joints
    return coord, obj, selfpose


def _prior_log(coord, obj, selfpose, prior):
    log = OrderedDict()
    log["loss_prior"], log["loss_bbox"], log["loss_obj"], log["loss_selfpose"] = prior.item(), coord.item(), obj.item(), selfpose.item()
    return log


def yolo_loss_fgweight(pred, prior_map_gt, prior_mask_conf, prior_mask_coord, num_joints, num_anchors):
    """The plain prior loss; returns only the total, as the reference's does."""
    p, g, m_conf, m_coord = _prior_views(pred, prior_map_gt, num_anchors, prior_mask_conf, prior_mask_coord)
    coord, obj, selfpose = _prior_terms(p, g, m_coord, m_conf, num_joints)
    return coord + obj + selfpose


def yolo_loss_fgweight_poseweight(pred, prior_map_gt, prior_mask_conf, prior_mask_coord, prior_weight_map, num_joints, num_anchors):
    """The pose-rarity weighted prior loss (the trainer's default, --rarity-weight 1) -> (total, log of the four terms)."""
    p, g, m_conf, m_coord, wmap = _prior_views(pred, prior_map_gt, num_anchors, prior_mask_conf, prior_mask_coord, prior_weight_map)
    coord, obj, selfpose = _prior_terms(p, g, m_coord, m_conf, num_joints, weight=wmap)
    prior = coord + obj + selfpose
    return prior, _prior_log(coord, obj, selfpose, prior)
