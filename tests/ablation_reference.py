"""numpy restatement of the depth-ablation read-outs of the reference's evaluation script
(tpm/evaluate/evaluation_rtpose_light3d_kdh3d_mpreal_ablation.py:197-299), one frame at a time.  What the HIP entries
pn_ablation_pred_raw / pn_ablation_perfect_2d / pn_depth_probe are checked against, and itself pinned by
tests/golden/script_eval_data_ablation.json (tests/test_ablation_reference.py).

Every step keeps the reference's number formats: the network input and the pose-depth map are float32 and are un-normalised
in float32 (`*= std`, `+= mean`, two roundings), the index arithmetic is Python float / int(), the back-projection float64.
"""
import numpy as np

NUM_JOINTS = 15
INTRINSICS = {"fx": 504.1189880371094, "fy": 504.042724609375, "cx": 231.7421875, "cy": 320.62640380859375}


def unnormalise(a, depth_mean=3.0, depth_std=2.0):
    """`a *= depth_std; a += depth_mean` on a float32 array (:179-180, :183-185)."""
    a = np.array(a, dtype=np.float32, copy=True)
    a *= depth_std
    a += depth_mean
    return a


def back_project(xy, depth, intrinsics):
    """np.vstack([(x - cx) * d / fx, (y - cy) * d / fy, d]).T in float64 (:258-262 and its three twins)."""
    xy = np.asarray(xy, dtype=np.float64).reshape(-1, 2)
    depth = np.asarray(depth, dtype=np.float64)
    X = (xy[:, 0] - intrinsics["cx"]) * depth / intrinsics["fx"]
    Y = (xy[:, 1] - intrinsics["cy"]) * depth / intrinsics["fy"]
    return np.vstack([X, Y, depth]).T


def pred_raw(img, joint_list, person_joint, w_org, h_org, input_size, intrinsics=INTRINSICS):
    """human_pred_set_3d_read_raw_depth of one frame (:198-218, :245-274) -> float64 [P, 15, 3].
    img: the un-normalised S x S input; joint_list [N, >= 2] rows (x, y, ...) in the network frame, person_joint [P, 15] row
    ids (-1 = the person has no such joint)."""
    person_joint = np.asarray(person_joint).reshape(-1, NUM_JOINTS).astype(np.int64)
    out = np.zeros((len(person_joint), NUM_JOINTS, 3), np.float64)
    for i, ids in enumerate(person_joint):
        human = np.full((NUM_JOINTS, 2), -1.0)
        raw = np.ones(NUM_JOINTS) * -1
        for j, k in enumerate(ids):
            if k >= 0:
                x, y = float(joint_list[k][0]), float(joint_list[k][1])
                raw[j] = img[int(y), int(x)]
                human[j] = [x / input_size * w_org, y / input_size * h_org]
        out[i] = back_project(human, raw, intrinsics)
    return out


def perfect_2d(img, z, gt_2d, w_org, h_org, input_size, downsample=8, depth_mean=3.0, depth_std=2.0, intrinsics=INTRINSICS):
    """(human_pred_set_3d_perfect_2d, human_pred_set_3d_perfect_2d_read_raw_depth) of one frame (:220-242, :279-299) ->
    two float64 [G, 15, 3].  z [15, h, w]: the pose-depth map as the network emits it (normalised float32);
    gt_2d [G][15][2]: the labels' joints (Python floats or ints)."""
    posedepth = unnormalise(z, depth_mean, depth_std)
    G = len(gt_2d)
    out_map, out_raw = np.zeros((G, NUM_JOINTS, 3), np.float64), np.zeros((G, NUM_JOINTS, 3), np.float64)
    for i, human in enumerate(gt_2d):
        d_map, d_raw = np.ones(NUM_JOINTS) * -1, np.ones(NUM_JOINTS) * -1
        for j, joint in enumerate(human):
            gx, gy = float(joint[0]), float(joint[1])
            x2d = int(gx / w_org * input_size / downsample)
            y2d = int(gy / h_org * input_size / downsample)
            x2d = min(max(x2d, 0), int(input_size / downsample) - 1)
            y2d = min(max(y2d, 0), int(input_size / downsample) - 1)
            d_map[j] = posedepth[j, y2d, x2d]
            x2d = min(max(int(gx / w_org * input_size), 0), int(input_size) - 1)
            y2d = min(max(int(gy / h_org * input_size), 0), int(input_size) - 1)
            d_raw[j] = img[y2d, x2d]
        human = np.array(human, dtype=np.float64)
        out_map[i] = back_project(human, d_map, intrinsics)
        out_raw[i] = back_project(human, d_raw, intrinsics)
    return out_map, out_raw


def ablation_reference(x_norm, maps, parse, gt_2d, w_org=480, h_org=640, input_size=224, downsample=8, depth_mean=3.0,
                       depth_std=2.0, intrinsics=INTRINSICS):
    """The three computed arms of ONE frame.  x_norm [S, S] float32: the normalised network input (pn_preprocess's output);
    maps = (paf, heat, z) of the frame, channel first (only z [15, h, w] is read: the arms touch neither paf nor heat);
    parse = (joint_list, person_joint); gt_2d [G][15][2].  Returns a dict keyed like eval_data.json."""
    img = unnormalise(x_norm, depth_mean, depth_std)
    joint_list, person_joint = parse
    pm, pr = perfect_2d(img, np.asarray(maps[2]), gt_2d, w_org, h_org, input_size, downsample, depth_mean, depth_std, intrinsics)
    return {"human_pred_set_3d_read_raw_depth": pred_raw(img, joint_list, person_joint, w_org, h_org, input_size, intrinsics),
            "human_pred_set_3d_perfect_2d": pm, "human_pred_set_3d_perfect_2d_read_raw_depth": pr}
