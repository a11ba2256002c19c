"""The convolution levels of the two inference nets as data, the frame sizes of the small / ragged sweep, and the census of what they plan (no GPU).

popnet_amd/csrc/conv_plan.h decides kernel, tile and launch of every convolution from the map's height and width; pn_conv_level_plan_info
answers for one level without a device.  The tables below are transcribed from net.hip::build_rtpose / build_yolo (topology 15 parts /
14 limbs, input_dim 1: what the per-layer tests compile); tests/test_gpu_layer_shapes.py compares every field with pn_net_step_info of
the compiled net, so they cannot drift from the nets.

  RTPOSE_LEVELS / YOLO_LEVELS   (map scale, [(weight name, cin, cout, ks, stride), ...]): the convolutions of a level read the map
                                frame / scale.  cin = channels the K loop covers: the input BUFFER's where it is wider than the weight's
                                Cin -- Cin(bf16 / fp32, bf16x3): bf16x3 reads whole buffers, stage 1 reads the 192-channel concat buffer.
                                ks = EMBED3: YoloPoseNet's stride-2 shortcut, a 1x1 run as the centre tap of a 3x3 in bf16 / bf16x3.
  plan_net                      every convolution of a net at a frame size, planned level by level; Refused where finalize refuses
  SWEEP                         the sweep entries, each with the condition it is there for
  CONDITIONS                    the census: name -> predicate over one planned convolution
"""
import contextlib
import ctypes as C
import functools
import json
import os
from collections import namedtuple

from popnet_amd import _lib

PREC = {"fp32": 0, "bf16": 1, "bf16x3": 2}
CFG_C128, CFG_C64, CFG_C32, CFG_C16, CFG_C64W = range(5)
NUM_CUS = 256
EMBED3 = "embed3"
Cin = namedtuple("Cin", "plain x3")
_CAT = Cin(128, 192)

RTPOSE_LEVELS = [(2, [("model0.layer1.%d.conv%d" % (b, c), 64, 64, 3, 1)]) for b in (0, 1) for c in (1, 2)] + [
    (4, [("model0.layer2.0.conv1", 64, 128, 3, 1), ("model0.layer2.0.downsample.0", 64, 128, 1, 1)]),
    (4, [("model0.layer2.0.conv2", 128, 128, 3, 1)]),
    (4, [("model0.conv2", 128, 128, 1, 1)]),
]
for _s in (1, 2):
    _c0 = _CAT if _s == 1 else 192               # stage 2: the input-channel map covers the whole concat buffer in every precision
    _n = lambda br, i, _s=_s: "model%d_%d.%d" % (_s, br, i)
    RTPOSE_LEVELS += [
        (8, [(_n(1, 0), _c0, 256, 3, 1), (_n(2, 0), _c0, 128, 3, 1), (_n(3, 0), _c0, 128, 3, 1)]),
        (8, [(_n(1, 3), 256, 256, 3, 1), (_n(2, 3), 128, 128, 3, 1), (_n(3, 3), 128, 64, 3, 1)]),
        (8, [(_n(1, 6), 256, 256, 3, 1), (_n(2, 6), 128, 128, 3, 1), (_n(3, 6), 64, 64, 3, 1)]),
        (8, [(_n(1, 9), 256, 128, 1, 1), (_n(2, 9), 128, 128, 3, 1), (_n(3, 9), 64, 64, 3, 1)]),
        (8, [(_n(1, 12), 128, 28, 1, 1), (_n(2, 12), 128, 16, 3, 1), (_n(3, 12), 64, 15, 3, 1)]),
    ]

YOLO_LEVELS = [(4, [("model0.layer1.%d.conv%d" % (b, c), 64, 64, 3, 1)]) for b in (0, 1, 2) for c in (1, 2)] + [
    (4, [("model0.layer2.0.conv1", 64, 128, 3, 2), ("model0.layer2.0.downsample.0", 64, 128, EMBED3, 2)]),
    (8, [("model0.layer2.0.conv2", 128, 128, 3, 1)]),
] + [(8, [("model0.layer2.%d.conv%d" % (b, c), 128, 128, 3, 1)]) for b in (1, 2, 3) for c in (1, 2)] + [
    (8, [("model1.0", 128, 256, 3, 1)]),
] + [(8, [("model1.%d" % i, 256, 256, 3, 1)]) for i in (3, 6, 9, 12)] + [
    (8, [("model2_1.0", 256, 256, 3, 1)]),
    (16, [("model2_2.0", 256, 256, 3, 1)]),
    (16, [("model2_3.0", 256, 128, 3, 1)]),
    (16, [("model2_4.0", 128, 100, 3, 1)]),
]
LEVELS = {"rtpose": RTPOSE_LEVELS, "yolo": YOLO_LEVELS}
FRAME_STEP = {"rtpose": 8, "yolo": 16}

GEOM = ("kern", "cfg", "pitch", "R", "Wt", "wc", "wp", "nbuf", "pt", "rpg", "tiles_x", "tiles_per_img", "cout_blocks", "nblocks", "lds_two")
SWITCHES = ("POPNET_CONV3_PT14", "POPNET_CONV3_NBUF2", "POPNET_CONV3_RPG8", "POPNET_CONV4", "POPNET_NO_CONV3", "POPNET_GENERIC_C64", "POPNET_NO_EMBED3", "POPNET_NO_BBLOCK",
            "POPNET_BBLOCK_X3", "POPNET_NO_MIX", "POPNET_NO_TAILFUSE", "POPNET_NO_POOLFUSE")


class Refused(Exception):
    """The planner refuses the shape (PN_ERR_UNSUPPORTED): pn_net_finalize does too."""


@functools.lru_cache(None)
def _ctx():
    return _lib.lib().pn_create(-1)


@contextlib.contextmanager
def environment(env):
    """The kernel switches are read from the environment at every planning call, as pn_net_finalize reads them."""
    old = {k: os.environ.get(k) for k in SWITCHES}
    for k in SWITCHES:
        os.environ.pop(k, None)
    os.environ.update(env)
    try:
        yield
    finally:
        for k in SWITCHES:
            os.environ.pop(k, None)
        os.environ.update({k: v for k, v in old.items() if v is not None})


_BUF = C.create_string_buffer(4096)


def plan_level(prec, max_batch, B, H, W, convs, together, num_cus=NUM_CUS):
    """convs: [(cin, cout, ks, stride)] -> the plan dicts.  Reads the switches from the environment as it is."""
    n = len(convs)
    arr = [(C.c_int * n)(*[c[i] for c in convs]) for i in (1, 0, 2, 3)]          # cout, cin, ks, stride
    rc = _lib.lib().pn_conv_level_plan_info(_ctx(), PREC[prec], max_batch, num_cus, B, H, W, 1 if together else 0, n, *arr, _BUF, len(_BUF))
    if rc == -4:
        msg = C.create_string_buffer(512)
        _lib.lib().pn_last_error(_ctx(), msg, len(msg))
        raise Refused(msg.value.decode())
    assert rc == 0, rc
    return json.loads(_BUF.value.decode())["convs"]


def has_instance(prec, ks, stride, pitch, cfg):
    return bool(_lib.lib().pn_conv_has_instance(0 if prec == "fp32" else 1, ks, stride, pitch, cfg))


# H, W: the input map; p: the plan dict; own: the compiled net certainly launches this convolution as the kernel p["kernel"] names (own_launch)
Conv = namedtuple("Conv", "name cin cout ks stride H W Ho Wo B max_batch prec p own")


def _on(env, name):
    return name in env


def own_launch(kind, prec, env, level):
    """Which convolutions of a planned level [(name, plan)] are launched as the very kernel their plan names.  net.hip fuses AFTER planning: a
    BasicBlock(64) pair becomes one bb64_kernel / bb64x3_kernel step, a `1x1 128 -> <= 32` head becomes the tail of the 1x1 before it, model0.conv2
    takes the average pool into its launch (another instantiation under the same label), and a level's 128-cout 3x3 and 1x1 conv3 blocks may share
    one conv3_mix_kernel launch.  The plan view reports the unfused plan for all of them, so the census and the label guard count a convolution only
    where this returns True.  The rules here err on the side of False (they ignore the fusions' further conditions);
    tests/test_gpu_layer_shapes.py asserts for every compiled net that each convolution counted here sits in a plain conv step whose kernel label
    is the plan's."""
    env = env or {}
    conv3_on = not _on(env, "POPNET_NO_CONV3")
    bblock = conv3_on and not _on(env, "POPNET_NO_BBLOCK") and (prec == "bf16" or (prec == "bf16x3" and env.get("POPNET_BBLOCK_X3", "0") != "0"))
    mixable = [n for n, p in level if p["kern"] == 3 and (p["wc"], p["wp"], p["nbuf"], p["pt"], p["rpg"]) == (4, 1, 1, 7, 4)]
    mixed = kind == "rtpose" and not _on(env, "POPNET_NO_MIX") and len({p["kernel"] for n, p in level if n in mixable}) > 1
    plans = dict(level)
    out = {}
    for name, p in level:
        own = True
        if p["kern"] == 3:
            if bblock and name.startswith("model0.layer1."):
                own = False                               # bb64_kernel
            if kind == "rtpose" and name == "model0.conv2" and prec != "fp32" and not _on(env, "POPNET_NO_POOLFUSE"):
                own = False                               # the fused-pool instantiation
            if kind == "rtpose" and name.endswith("_1.9") and prec == "bf16" and not _on(env, "POPNET_NO_TAILFUSE"):
                own = False                               # the fused-tail instantiation
            if mixed and name in mixable:
                own = False                               # conv3_mix_kernel
        if kind == "rtpose" and name.endswith("_1.12") and prec == "bf16" and conv3_on and not _on(env, "POPNET_NO_TAILFUSE"):
            own = False                                   # runs as the tail of model<s>_1.9 where that is a conv3_kernel launch
        out[name] = own
    return out


def concrete(kind, prec, env=None):
    """The level table with cin and ks resolved for a precision (and POPNET_NO_EMBED3)."""
    embed = prec != "fp32" and "POPNET_NO_EMBED3" not in (env or {})
    out = []
    for scale, convs in LEVELS[kind]:
        lv = []
        for name, cin, cout, ks, stride in convs:
            if isinstance(cin, Cin):
                cin = cin.x3 if prec == "bf16x3" else cin.plain
            lv.append((name, cin, cout, (3 if embed else 1) if ks == EMBED3 else ks, stride))
        out.append((scale, lv))
    return out


def plan_net(kind, prec, max_batch, B, H, W, env=None):
    """Every convolution of the net at frame H x W, as [Conv].  Raises Refused("<weight name>: <reason>")."""
    out, same = [], {}
    with environment(env or {}):
        for scale, convs in concrete(kind, prec, env):
            h, w = H // scale, W // scale
            key = (scale, tuple(c[1:] for c in convs))          # the BasicBlocks and the two stages repeat their levels
            try:
                if key not in same:
                    same[key] = plan_level(prec, max_batch, B, h, w, [c[1:] for c in convs], together=kind == "rtpose")
                plans = same[key]
            except Refused as e:
                i = int(str(e).split()[1].rstrip(":"))
                raise Refused("%s: %s" % (convs[i][0], str(e).split(": ", 1)[1]))
            own = own_launch(kind, prec, env, [(c[0], p) for c, p in zip(convs, plans)])
            for (name, cin, cout, ks, stride), p in zip(convs, plans):
                ho, wo = (h + 2 * (ks // 2) - ks) // stride + 1, (w + 2 * (ks // 2) - ks) // stride + 1
                out.append(Conv(name, cin, cout, ks, stride, h, w, ho, wo, B, max_batch, prec, p, own[name]))
    return out


def existing_plans():
    """The dump behind tests/golden/plan_existing.json: {configuration id: [[weight name, plan], ...]} for test_gpu_layers.CONFIGS."""
    import test_gpu_layers as GL
    return {id_: [[c.name, c.p] for c in plan_net(kind, prec, B, B, H, W, env)] for id_, kind, prec, B, H, W, _, env in GL.CONFIGS}


def grid(kind):
    s = FRAME_STEP[kind]
    return [(h, w) for h in range(s, 513, s) for w in range(s, 513, s)]


# ---- the sweep ------------------------------------------------------------------------------------------------------------------------------------
# (network, H, W, B, max_batch, environment, precisions, what it is there for).  max_batch != B: the module is compiled with POPNET_MAX_BATCH.
ALL = ("bf16", "bf16x3", "fp32")
SWEEP = []


def _sw(kind, H, W, why, B=2, max_batch=None, env=None, precs=ALL):
    SWEEP.append((kind, H, W, B, max_batch or B, dict(env or {}), tuple(precs), why))


def sweep_id(e):
    kind, H, W, B, mb, env, _, _ = e
    return "%s_%dx%d_b%d%s%s" % ("rt" if kind == "rtpose" else "yolo", H, W, B, "of%d" % mb if mb != B else "",
                                  "".join("_" + k[7:].lower() + v for k, v in sorted(env.items())))


def cin_chunks(c):
    return ((3 if c.prec == "bf16x3" else 1) * c.cin + 63) // 64


# _cfg_pixels, _maxpx and _needed_pitch restate constants of conv_mfma.hip / conv_plan.h (pixels per tile configuration, staging capacity per pitch
# class, the pitch classes) so that the census can say WHY a plan looks as it does; they change together with those files.
def _cfg_pixels(cfg):
    return 112 if cfg == CFG_C128 else 224 if cfg == CFG_C64W else 128


def generic(c):
    return c.p["kern"] == 0


def _c64_by_cus(c):
    # pn_pick_cfg gives C128 for cout % 128 == 0; the plan says C64: the "fewer 128-cout blocks than CUs" rule (or C64W after it)
    return generic(c) and c.cout % 128 == 0 and c.p["cfg"] in (CFG_C64, CFG_C64W)


def _maxpx(c):
    if c.p["cfg"] == CFG_C64W or c.stride != 1:
        return 0
    px = 128 if c.ks == 1 else 192 if c.p["pitch"] <= 32 else 288 if c.p["pitch"] <= 64 else 360
    return px if (px * (8 if c.prec != "fp32" else 16) + 255) // 256 <= 12 else 0


def _r_nominal(c):
    return max(1, min(c.Ho, _cfg_pixels(c.p["cfg"]) // c.p["Wt"]))


def _needed_pitch(c):
    need = (c.p["Wt"] - 1) * c.stride + c.ks
    return next(k for k in (16, 32, 64, 120) if need <= k)


CONDITIONS = {
    "cfg C128": lambda c: generic(c) and c.p["cfg"] == CFG_C128,
    "cfg C64 by cout": lambda c: generic(c) and c.p["cfg"] == CFG_C64 and c.cout % 128 != 0,
    "cfg C64 by the CU-count rule": lambda c: _c64_by_cus(c) and c.p["cfg"] == CFG_C64,
    "cfg C64W": lambda c: generic(c) and c.p["cfg"] == CFG_C64W,
    "cfg C32": lambda c: generic(c) and c.p["cfg"] == CFG_C32,
    "cfg C16": lambda c: generic(c) and c.p["cfg"] == CFG_C16,
    "generic row in 2 segments": lambda c: generic(c) and c.p["tiles_x"] == 2,
    "generic row in 3 or more segments": lambda c: generic(c) and c.p["tiles_x"] >= 3,
    "generic ragged last segment": lambda c: generic(c) and c.Wo % c.p["Wt"] != 0,
    "generic ragged last row tile": lambda c: generic(c) and c.Ho % c.p["R"] != 0,
    "generic Ho below the tile's nominal rows": lambda c: generic(c) and c.Ho < _cfg_pixels(c.p["cfg"]) // c.p["Wt"],
    "generic Ho == 1": lambda c: generic(c) and c.Ho == 1,
    "generic Wo == 1": lambda c: generic(c) and c.Wo == 1,
    "generic R lowered by maxpx": lambda c: generic(c) and _maxpx(c) > 0 and c.p["R"] < _r_nominal(c),
    "generic R lowered by the LDS limit": lambda c: generic(c) and c.p["R"] < _r_nominal(c) and (c.p["R"] * c.stride + c.ks) * c.p["pitch"] * (256 if c.prec == "fp32" else 128) > 160 * 1024,
    "generic lds_two == 0": lambda c: generic(c) and c.p["lds_two"] == 0,
    "generic lds_two == 1": lambda c: generic(c) and c.p["lds_two"] == 1,
    "generic pitch widened by the fallback": lambda c: generic(c) and c.p["pitch"] > _needed_pitch(c),
    "conv3 strip width 30": lambda c: c.p["kern"] == 3 and c.p["Wt"] == 30,
    "conv3 map 31 wide: two 16-wide strips": lambda c: c.p["kern"] in (3, 4) and c.W == 31 and c.p["Wt"] == 16 and c.p["tiles_x"] == 2,
    "conv3 H % rows != 0": lambda c: c.p["kern"] == 3 and c.H % c.p["R"] != 0,
    "conv4 odd strip count": lambda c: c.p["kern"] == 4 and (c.B * c.p["tiles_per_img"]) % 2 == 1,
    "conv4 one cout block": lambda c: c.p["kern"] == 4 and c.p["cout_blocks"] == 1,
    "conv4 two cout blocks": lambda c: c.p["kern"] == 4 and c.p["cout_blocks"] == 2,
    "net run at B < max_batch": lambda c: c.B < c.max_batch,
}


def generic_class(c):
    return (c.ks, c.stride, c.p["pitch"])


def conv3_tuple(c):
    return (c.ks, c.p["wc"], c.p["wp"], c.p["nbuf"], c.p["pt"], c.p["rpg"])


# The issue's list, trimmed to what the census (tests/test_plan_cases.py) needs plus the small / ragged sizes it names.
_sw("rtpose", 8, 8, "1x1 stage maps: Ho == 1 and Wo == 1 on every stage kernel; 1x1 at pitch 16 -> 32 (fallback)")
_sw("rtpose", 16, 24, "2x3 stage maps; 4x6 / 8x12 backbone maps below one strip tile")
_sw("rtpose", 40, 64, "width <= 64: layer2.0.downsample and model0.conv2 on the generic 1x1 at the widened pitch")
_sw("rtpose", 40, 104, "13-wide stage maps, 26-wide layer2 maps; H % rows != 0")
_sw("rtpose", 72, 128, "16-wide stage maps: the widest that need the 1x1 pitch fallback")
_sw("rtpose", 72, 136, "17-wide stage maps: one column above the pitch-16 class")
_sw("rtpose", 24, 232, "29-wide stage maps, 58-wide layer2 maps (two 29-wide strips)")
_sw("rtpose", 32, 240, "conv3 strip width exactly 30")
_sw("rtpose", 40, 248, "stage map 31 wide: two 16-wide strips")
_sw("rtpose", 8, 464, "one-row stage maps 58 wide")
_sw("rtpose", 8, 512, "one-row maps 64 wide: pitch 120 on the 128-, 32- and 16-cout blocks; fp32: 256-wide layer1 rows in 3 segments of 86, the last ragged")
_sw("rtpose", 8, 264, "fp32: the 1x1 layer2 convolutions on one 66-wide segment, pitch 120 with 128-cout blocks")
_sw("rtpose", 480, 8, "one-column maps: Wo == 1 with many row tiles")
_sw("rtpose", 104, 488, "61-wide stage maps (3 strips), 122-wide layer2 maps; fp32: 244-wide layer1 rows in 3 segments of 82, the last one ragged")
_sw("yolo", 16, 16, "1x1 head map, 2x2 / 4x4 backbone maps; stride 2 at pitch 16 -> 64 (fallback)")
_sw("yolo", 256, 16, "tall 4-wide map into the stride-2 level: 32 output rows at pitch 64 exceed the LDS, R is lowered to fit")
_sw("yolo", 32, 96, "stride 2 with a 25-column halo: pitch 32 -> 64")
_sw("yolo", 48, 112, "the widest frame whose stride-2 level needs the pitch fallback (halo 29)")
_sw("yolo", 96, 128, "stride-2 halo 33: the first width with an instance of its own")
_sw("yolo", 64, 208, "26-wide layer2 maps, 13-wide head maps")
_sw("yolo", 48, 256, "stride-2 halo 65: pitch 120")
_sw("yolo", 48, 272, "34-wide layer2 maps: two 17-wide strips")
_sw("yolo", 32, 464, "stride-2 row of 58 outputs: halo 117, one segment")
_sw("yolo", 32, 480, "stride-2 row of 60 outputs: two segments")
_sw("yolo", 32, 496, "31-wide head maps: two 16-wide strips")
# the switches, each at a small size where it changes the plan (the census names the conv3_kernel variant); max_batch 32 at B = 2: the plan is made for
# max_batch (8-row tiles, WP = 2, need 1536 strip tiles), the run costs two frames
# (PT14=1 needs cin_chunks == 1, so bf16 only, and there the layer1 pairs it applies to are fused into bb64_kernel: POPNET_NO_BBLOCK=1 keeps the four launches)
_sw("rtpose", 96, 240, "POPNET_CONV3_PT14=1: conv3_kernel<3, 2, 1, 1, 14, 8> where the plan has WP = 2", max_batch=32, env={"POPNET_CONV3_PT14": "1", "POPNET_NO_BBLOCK": "1"},
    precs=("bf16",))
_sw("rtpose", 32, 88, "POPNET_CONV3_PT14=2: conv3_kernel<3, 4, 1, 1, 14, 8>", env={"POPNET_CONV3_PT14": "2"}, precs=("bf16", "bf16x3"))
_sw("rtpose", 96, 240, "POPNET_CONV3_NBUF2=1 with WP = 2: conv3_kernel<3, 2, 2, 2, 7, 4> (bf16x3)", max_batch=32, env={"POPNET_CONV3_NBUF2": "1"}, precs=("bf16", "bf16x3"))
_sw("rtpose", 16, 88, "POPNET_CONV3_NBUF2=1: conv3_kernel<3, 2, 1, 2, 7, 4> (bf16x3), <3, 4, 1, 2, 7, 4>", env={"POPNET_CONV3_NBUF2": "1"}, precs=("bf16", "bf16x3"))
_sw("rtpose", 24, 56, "POPNET_CONV3_RPG8=1: conv3_kernel<3, 4, 1, 1, 7, 8> on 14-wide maps", env={"POPNET_CONV3_RPG8": "1"}, precs=("bf16", "bf16x3"))
_sw("rtpose", 24, 240, "POPNET_CONV4=1 at B = 3: one 3-row strip per frame on the stage maps, so the last conv4 block holds one strip", B=3, env={"POPNET_CONV4": "1"}, precs=("bf16", "bf16x3"))
_sw("rtpose", 40, 104, "compiled for max_batch 5, run at B = 2", max_batch=5)

# Conditions no size of the grid reaches for these two nets (asserted over the grid in tests/test_plan_cases.py, not only over the sweep):
#   a map 31 wide on conv3_kernel / conv4_kernel: its two 16-wide strips of 4 rows hold 62 of a wave group's 112 pixel slots, below the 0.75
#   fill the planner asks, whatever the height -- such a map always runs the generic kernel (the sweep runs it there: 40x248, 32x496).
UNREACHABLE = ("conv3 map 31 wide: two 16-wide strips",)
# Kernel labels that the grid gives to a convolution launched as planned at max_batch 32 only: the 128-cout generic blocks of the bf16 nets, which at
# max_batch <= 3 always make fewer blocks than the chip has CUs and become 64-cout blocks (test_gpu_layers.CONFIGS runs B = 32 at 224 x 224 only); and the
# plain 1x1 conv3_kernel, which at small batches is always pool-fused, tail-fused or part of a conv3_mix_kernel launch and has a launch of its own only
# beside a conv4 level (by block count at B = 32: CONFIGS; by POPNET_CONV4=1: CONFIGS and the sweep's 24x240 entry).
LARGE_BATCH_ONLY = ("conv_mfma_kernel<1, 1, 1, 32, 0>", "conv_mfma_kernel<1, 1, 1, 64, 0>", "conv_mfma_kernel<1, 3, 1, 16, 0>", "conv_mfma_kernel<1, 3, 1, 32, 0>",
                    "conv_mfma_kernel<1, 3, 1, 64, 0>", "conv3_kernel<1, 4, 1, 1, 7, 4>")
