"""What scripts/evaluate_mpaug.py and scripts/evaluate_kdh3d.py share: the per-batch body of the reference's composed and single-person
KDH3D evaluation scripts once the network input exists (third_party_methods/evaluate/evaluation_rtpose_light3d_kdh3d_mpaug_ablation.py:
196-330, evaluation_yolo_posenet_kdh3d_mpaug.py:165-225 and their single-person twins), and their metric tail."""
import numpy as np

from . import _lib, dataset, metrics
from .config import KEYPOINTS


def load_state_dict(path):
    """A reference checkpoint: a state_dict, 'module.'-prefixed (DataParallel) or not."""
    import torch
    sd = torch.load(path, map_location="cpu")
    return {(k[len("module."):] if k.startswith("module.") else k): v for k, v in sd.items()}


def engine_intrinsics(eng):
    """The intrinsics the engine's parse back-projects with (the profile's unless overridden)."""
    return {"fx": eng.cfg.fx, "fy": eng.cfg.fy, "cx": eng.cfg.cx, "cy": eng.cfg.cy}


def predict_batch(eng, x, gt_2d, ablation=False, first_person=False):
    """One batch of network inputs x [B,1,S,S] through a PoseEngine or YoloEngine -> the per-frame lists of the scripts' prediction keys.
    gt_2d: per frame the ground-truth persons' [15][2] joints (original-frame pixels), read by the depth-ablation arms (ablation=True,
    PoseEngine only).  first_person: the single-person scripts' rule (dataset.kdh3d_pose_lists / yolo_kdh3d_lists)."""
    from .pipeline import PoseEngine, records_to_numpy
    if not isinstance(eng, PoseEngine):
        if ablation:
            raise _lib.PopnetError("the depth-ablation arms are Open-Pose+'s: the Yolo-Pose+ scripts have none")
        recs = eng.predict_inputs(x).cpu().numpy().view(_lib.YOLO_FRAME_DTYPE).reshape(-1)
        return dataset.yolo_kdh3d_lists(recs, first_person=first_person, input_size=eng.S, w_org=eng.cfg.w_org, h_org=eng.cfg.h_org,
                                        intrinsics=engine_intrinsics(eng))
    recs = eng.predict_inputs(x)
    if ablation:
        raw, pm, pr = eng.ablation_arms(x, recs, gt_2d)
        lists = eng.ablation_lists(x, gt_2d, records_to_numpy(recs), raw, pm, pr)
    else:
        lists = eng.lists_from_records(records_to_numpy(recs))
    return dataset.kdh3d_pose_lists(lists, first_person=first_person)


def print_table(kind, th, names, kcp, dist):
    print('     %s threshold: %03f%s' % (kind, th, ' meter' if kind == '3D' else ''))
    for i, name in enumerate(names):
        print('     joint: {},  PCK: {:03f}, avg {} error: {:03f}'.format(name, kcp[i], kind, dist[i]))
    print('\n     Overall: PCK: {:03f}, avg {} error: {:03f} \n'.format(np.average(kcp), kind, np.average(dist)))


def evaluate(data, w_org, h_org, ablation=False, verbose=True):
    """The scripts' metric tail on the eval_data dictionary: 2D at 2 % of the frame diagonal, 3D at 10 cm, and with ablation the five
    blocks of metrics.evaluate_ablation_blocks.  -> dict of the numbers it prints."""
    th = 0.02 * np.sqrt(w_org ** 2 + h_org ** 2)
    d2, k2 = metrics.eval_human_dataset_2d(data["human_pred_set_2d"], data["human_gt_set_2d"], num_joints=15, dist_th=th, iou_th=0.5)
    d3, k3 = metrics.eval_human_dataset_3d(data["human_pred_set_2d"], data["human_gt_set_2d"], data["human_pred_set_3d"], data["human_gt_set_3d"],
                                           num_joints=15, dist_th=0.1, iou_th=0.5)
    if verbose:
        print('\nevaluating in 2D...')
        print_table('2D', th, KEYPOINTS, k2, d2)
        print('\nevaluating in 3D...')
        print_table('3D', 0.1, KEYPOINTS, k3, d3)
    out = {"dist_th_2d": th, "pck2d": k2, "err2d": d2, "pck3d": k3, "err3d": d3}
    if ablation:
        out.update(metrics.evaluate_ablation_blocks(data, data["human_gt_set_2d"], data["human_gt_set_3d"], verbose=verbose))
    return out
