"""The shapes of the split-bf16 1x1 convolutions (csrc/conv1x1_x3.hip): the 34 stride-1 1x1 layers of A2J_model at the trainer's
shapes, the small cases tests/test_gpu_conv1x1_x3.py runs, and the plan class of a call -- its kernel label together with the edge
conditions the kernel meets, all read from pn_conv1x1_x3_plan_info (the launch code's own planner; nothing is launched)."""
import ctypes as C
import json

ROLES = ("forward", "dgrad", "wgrad")
WHICH = {"forward": 0, "dgrad": 1, "wgrad": 3}           # PN_PLAN_FORWARD, PN_PLAN_DGRAD, PN_PLAN_WGRAD
SPLIT_KERNELS = ("conv1x1_x3_kernel", "conv1x1_wgrad_x3_kernel<vec>", "conv1x1_wgrad_x3_kernel<scalar>")
TRAIN_BATCHES, TRAIN_HW = (16, 31), (288, 288)

# (N, Cin, (rows, columns), Cout): the smallest shapes at which the kernels can still go wrong
GPU_CASES = [
    (2, 2048, (2, 3), 512),       # the longest K; the map smaller than any tile
    (2, 1024, (2, 3), 2048),      # the widest Cout
    (2, 64, (8, 12), 256),
    (3, 40, (5, 7), 72),          # K tail, ragged Cout block, odd HW: unaligned rows
    (1, 31, (9, 9), 17),          # K below one MFMA step
    (2, 64, (24, 40), 64),        # several pixel tiles, 4 even weight-gradient slices; HW % 32 == 0
    (2, 64, (24, 41), 64),        # HW % 32 != 0, HW % 4 == 0: chunk ends meet image ends on the vector path
    (3, 128, (32, 32), 128),      # whole 128-channel blocks, whole chunks, slices that divide evenly
    # the weight gradient's remaining classes at the trainer's shapes (the census of tests/test_conv1x1_x3_plan.py)
    (2, 64, (17, 32), 64),        # half a Cin block, whole chunks, 3 slices of 12 chunks for 34: ragged last slice
    (4, 128, (12, 20), 64),       # a ragged chunk per image, 2 even slices
    (2, 128, (24, 41), 64),       # a ragged chunk per image, ragged last slice
    (2, 128, (17, 32), 64),       # whole chunks, ragged last slice
    (1, 1, (1, 1), 1),
]


def a2j_layers(rows, cols):
    """(name, Cin, HW, Cout) of the 34 stride-1 1x1 convolutions of A2J_model (ResNet-50, layer4 dilated instead of strided) for an input of
    rows x cols: conv1 / conv3 of the 16 bottlenecks and the stride-1 downsample of layer1.0 and layer4.0."""
    out = []
    inplanes, red = 64, 4
    for layer, planes, blocks, stride in (("layer1", 64, 3, 1), ("layer2", 128, 4, 2), ("layer3", 256, 6, 2), ("layer4", 512, 3, 1)):
        for b in range(blocks):
            p = "Backbone.model.%s.%d" % (layer, b)
            hw_in = (rows // red) * (cols // red)
            if b == 0:
                red *= stride
            hw_out = (rows // red) * (cols // red)
            out.append((p + ".conv1", inplanes, hw_in, planes))
            out.append((p + ".conv3", planes, hw_out, planes * 4))
            if b == 0 and stride == 1:
                out.append((p + ".downsample.0", inplanes, hw_in, planes * 4))
            inplanes = planes * 4
    assert len(out) == 34
    return out


def plan(handle, role, N, Cin, HW, Cout):
    from popnet_amd import _lib
    buf = C.create_string_buffer(1024)
    rc = _lib.lib().pn_conv1x1_x3_plan_info(handle, WHICH[role], N, Cin, HW, Cout, buf, len(buf))
    if rc != 0:
        raise ValueError("pn_conv1x1_x3_plan_info(%s, %r) -> %d" % (role, (N, Cin, HW, Cout), rc))
    return json.loads(buf.value.decode())


def plan_class(role, p, N, Cin, HW, Cout):
    """The kernel label and the edge conditions of one call."""
    if role == "wgrad":
        return (role, p["kernel"], "ragged Cout block" if Cout % p["BM"] else "whole Cout blocks", "ragged Cin block" if Cin % p["BN"] else "whole Cin blocks",
                "ragged chunk at the image end" if HW % p["BK"] else "whole chunks", "one slice" if p["slices"] == 1 else "slices",
                "ragged last slice" if p["chunks"] % p["per_slice_chunks"] else "even slices", "aligned rows" if p["aligned"] else "unaligned rows")
    return (role, p["kernel"], "K tail" if p["K"] % p["BK"] else "whole K", "ragged channel block" if p["M"] % p["BM"] else "whole channel blocks",
            "ragged pixel tile" if p["P"] % p["BN"] else "whole pixel tiles", "one chunk" if p["chunks"] == 1 else "chunks")


def classes_of(handle, shapes):
    """{plan class: [shape, ...]} over the three roles of every (N, Cin, HW, Cout)"""
    out = {}
    for N, Cin, HW, Cout in shapes:
        for role in ROLES:
            out.setdefault(plan_class(role, plan(handle, role, N, Cin, HW, Cout), N, Cin, HW, Cout), []).append((N, Cin, HW, Cout))
    return out


def gpu_shapes():
    return [(N, Cin, h * w, Cout) for N, Cin, (h, w), Cout in GPU_CASES]


def trainer_shapes():
    return [(B, Cin, HW, Cout) for B in TRAIN_BATCHES for _, Cin, HW, Cout in a2j_layers(*TRAIN_HW)]
