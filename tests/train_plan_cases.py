"""The planes training step (csrc/trainx.hip) as data: every op of the step with its shape-dependent plan, the classes those plans fall into, and
the small / ragged shapes of the sweep (no GPU).

  step_ops(B, H, W, prec)   every launching op of the step, transcribed from trainx.hip::build (the source of truth): kind, the names
                            pn_trainer_op_info reports (layer / bn / stage), map size, channels or planes, and the plan the engine makes for it --
                            wgrad_plan (trainx_wgrad.h::plan_wgrad), red_plan (trainx.hip::red_blocks), head_plan (op_heads), the pooled sizes, the
                            stem's tiles / slices (train.hip), and for forward / data-gradient convolutions the device-less plan view
                            (pn_conv_level_plan_info through plan_cases.plan_level, the level grouped as add_conv_group groups it, POPNET_CONV4 not
                            honoured).  tests/test_gpu_train_layer_shapes.py compares every field with pn_trainer_op_info, with the device's CU count.
  classify(op)              the classes of one op: (family, field, value) tuples, one per decision the kernels' code branches on, plus the pairs of
                            decisions that meet in one piece of code (the ring re-priming of the weight gradient: rows_per_block against the ring depth
                            together with a short last block; what a block's row range crosses together with the number of column strips; a full-width
                            strip together with the strip count).  Convolutions are classed by kernel label (it names kernel, pitch class and nbuf), by
                            ragged last strip / last row tile and full 30-wide strip instead of the raw R and Wt (the inference sweep,
                            tests/plan_cases.py, covers the tile geometry of these kernels; what the trainer adds is the data gradient, the
                            residual, the NCHW head output and the conv4 decision by block count), so the census stays a list a sweep can cover.
  SWEEP                     (name, B, H, W, why): `why` holds the classes the entry is there for
  census()                  classes on the grid / reached by SHAPES / by SHAPES + SWEEP / exempt
"""
import functools

import plan_cases as PC
from train_layer_reference import SHAPES

NUM_CUS = 256
HEAD_C = (28, 16, 15)
CAT_PLANE = 192
BR_C = ((256, 256, 256, 128), (128, 128, 128, 128), (128, 64, 64, 64))
BR_KS = ((3, 3, 3, 1, 1), (3, 3, 3, 3, 3), (3, 3, 3, 3, 3))
RING = 5                      # trainx_wgrad.h: both rings hold five rows
K4_BLOCKS = 448               # conv_plan.h::pn_plan_level
GENERIC_CONDITIONS = ("generic Ho == 1", "generic Wo == 1", "generic R lowered by maxpx", "generic R lowered by the LDS limit", "generic pitch widened by the fallback")
GRID_B = (1, 2, 3, 5, 8, 32)
GRID_SIDES = tuple(range(8, 257, 8))
SIZE_CAP = 8 * 64 * 256       # pixels B * H * W of the largest frame a sweep entry may have
# what pn_trainer_finalize answers for one frame on a 1 x 1 stage map, and the shape of the sweep that asserts it (name, B, H, W)
REFUSAL = "model1_1.1: train-mode BatchNorm over one value per channel"
REFUSED_SWEEP = [("b1_8x8", 1, 8, 8)]


def _cdiv(a, b):
    return -(-a // b)


# ---- the plans ------------------------------------------------------------------------------------------------------------------------------------
def wgrad_plan(B, H, W, cin_my, cout, ks, num_cus=NUM_CUS):
    """trainx_wgrad.h::plan_wgrad"""
    seg = 32 - 2 * (ks // 2)
    tiles_x = _cdiv(W, seg)
    Wt = _cdiv(W, tiles_x)
    pairs = _cdiv(cout, 64) * _cdiv(cin_my, 64)
    rows_total = B * tiles_x * H
    Sr = max(1, min(rows_total, _cdiv(num_cus, pairs)))
    rpb = _cdiv(rows_total, Sr)
    return dict(tiles_x=tiles_x, Wt=Wt, rows_per_block=rpb, Sr=_cdiv(rows_total, rpb), seg_max=seg, rows_total=rows_total, pairs=pairs,
                clamped=_cdiv(num_cus, pairs) >= rows_total)


def red_plan(npix, C, num_cus=NUM_CUS):
    """trainx.hip::red_blocks: pixels per block (ppb) and blocks of the channel reductions"""
    PL = 256 // (C // 8)
    share = _cdiv(npix, 4 * num_cus)
    per = max(share, 8 * PL)
    per = _cdiv(per, PL) * PL
    return dict(C=C, ppb=per, nblk=_cdiv(npix, per), PL=PL, npix=npix, floor=share < 8 * PL)


def head_plan(B, h, w):
    """trainx.hip::op_heads: one 256-thread block per 256 elements of each head's NCHW output"""
    total = [B * c * h * w for c in HEAD_C]
    return dict(total=total, nblk=[_cdiv(t, 256) for t in total])


def pooled(h, w):
    """AvgPool2d(3, 2, 1)"""
    return (h - 1) // 2 + 1, (w - 1) // 2 + 1


def stem_plan(B, H, W, num_cus=NUM_CUS):
    """train.hip: pn_stem_forward_planes (16 x 8 output tiles, at most two blocks per CU) and t_wgrad_pixel_slices (49 x 64: one tile)"""
    ho, wo = H // 2, W // 2
    ntiles = B * _cdiv(wo, 16) * _cdiv(ho, 8)
    P = B * ho * wo
    s = max(1, min(1024, _cdiv(P, 1024)))
    pps = _cdiv(_cdiv(P, s), 32) * 32
    return dict(ho=ho, wo=wo, tiles_x=_cdiv(wo, 16), tiles_y=_cdiv(ho, 8), ntiles=ntiles, blocks=min(ntiles, 2 * num_cus), P=P, pps=pps, slices=_cdiv(P, pps))


def _red_chain(npix, C):
    """pixels per thread of the channel reductions at 256 CUs, as train_layer_reference.chain reads it"""
    return red_plan(npix, C)


def _wgrad_plan(B, H, W, cin_my, cout, ks):
    p = wgrad_plan(B, H, W, cin_my, cout, ks)
    return {k: p[k] for k in ("tiles_x", "Wt", "rows_per_block", "Sr")}


def wgrad_blocks(p, H):
    """[(first row, end row)] of every block in the flattened (image, column strip, row) space"""
    return [(r, min(r + p["rows_per_block"], p["rows_total"])) for r in range(0, p["rows_total"], p["rows_per_block"])]


def wgrad_span(p, H):
    """What the row ranges of a plan's blocks cross: a subset of {"strip seam", "image seam", "whole column"} ("strip seam": into the next column strip of
    the same image; "whole column": a block holds every row of at least one column strip)."""
    out = set()
    for r0, r1 in wgrad_blocks(p, H):
        c0, c1 = r0 // H, (r1 - 1) // H
        for c in range(c0, c1):
            out.add("image seam" if (c + 1) % p["tiles_x"] == 0 else "strip seam")
        first_whole = _cdiv(r0, H)
        if (first_whole + 1) * H <= r1:
            out.add("whole column")
    return out


def _same_launch(a, b):
    """conv_plan.h::pn_conv_same_launch on plan-view dicts (ks and stride are equal by construction of the caller's key)"""
    if any(a[k] != b[k] for k in ("pitch", "R", "Wt", "kern")):
        return False
    if a["kern"] == 4:
        return True
    if a["kern"] == 3:
        return all(a[k] == b[k] for k in ("wc", "wp", "nbuf", "pt", "rpg"))
    return a["cfg"] == b["cfg"]


@functools.lru_cache(None)
def _level(prec, B, h, w, convs, num_cus):
    with PC.environment({}):
        return PC.plan_level(prec, B, B, h, w, list(convs), together=True, num_cus=num_cus)


def k4_blocks(B, h, w, uses):
    """pn_plan_level's block count of a level: uses = [(kplane, rows, ks)]"""
    return sum(_cdiv(B * _cdiv(h, 4) * _cdiv(w, 30), 2) * _cdiv(rows, 128) for _, rows, ks in uses if ks == 3 and rows >= 64)


def conv_group(prec, B, h, w, uses, num_cus=NUM_CUS):
    """uses: [dict(layer, dgrad, kplane, rows, ks, res, nchw)] of one add_conv_group call -> the conv ops it pushes (one per kernel instantiation, first-fit in
    order), each problem with its plan-view dict under "p"."""
    plans = _level(prec, B, h, w, tuple((u["kplane"], u["rows"], u["ks"], 1) for u in uses), num_cus)
    blocks = k4_blocks(B, h, w, [(u["kplane"], u["rows"], u["ks"]) for u in uses])
    probs = [dict(u, p=p, H=h, W=w, B=B, prec=prec, level_blocks=blocks) for u, p in zip(uses, plans)]
    ops, used = [], [False] * len(probs)
    for i, a in enumerate(probs):
        if used[i]:
            continue
        members = []
        for j in range(i, len(probs)):
            if not used[j] and probs[j]["ks"] == a["ks"] and _same_launch(a["p"], probs[j]["p"]):
                members.append(probs[j])
                used[j] = True
        ops.append(dict(kind="conv", kernels=[a["p"]["kernel"]], problems=members))
    return ops


# ---- the layer table --------------------------------------------------------------------------------------------------------------------------------
def step_ops(B, H, W, prec, num_cus=NUM_CUS, convs=True):
    """Every launching op of the step in the engine's order (fork / join / pack apart).  convs=False leaves the convolution ops out (no plan view needed)."""
    assert H % 8 == 0 and W % 8 == 0 and H >= 8 and W >= 8 and B >= 1
    L2, L4, L8 = (H // 2, W // 2), (H // 4, W // 4), (H // 8, W // 8)
    if B * L8[0] * L8[1] < 2:                   # trainx.hip::build refuses it (PN_ERR_UNSUPPORTED)
        raise PC.Refused(REFUSAL)
    ops = []

    def conv(hw, uses):
        if convs:
            ops.extend(conv_group(prec, B, hw[0], hw[1], [dict(layer=u[0], dgrad=u[1], kplane=u[2], rows=u[3], ks=u[4], res=u[5], nchw=u[6]) for u in uses], num_cus))

    def bn(kind, hw, items):                  # items: [(bn name, C)]
        ops.append(dict(kind=kind, H=hw[0], W=hw[1], problems=[dict(bn=n, **red_plan(B * hw[0] * hw[1], c, num_cus)) for n, c in items]))

    def wgrad(hw, layer, ks, cin, cout, x_plane, cat=False, dbias_plane=None):
        if dbias_plane:
            ops.append(dict(kind="dbias", layer=layer, cout=cout, H=hw[0], W=hw[1], **red_plan(B * hw[0] * hw[1], dbias_plane, num_cus)))
        ops.append(dict(kind="wgrad", layer=layer, ks=ks, cin=cin, cout=cout, cat=int(cat), H=hw[0], W=hw[1], B=B,
                        **wgrad_plan(B, hw[0], hw[1], x_plane if cat else cin, cout, ks, num_cus)))

    def pool(kind, hw_in):
        ho, wo = pooled(*hw_in)
        ops.append(dict(kind=kind, H=hw_in[0], W=hw_in[1], Ho=ho, Wo=wo))

    # ---- forward ----
    ops.append(dict(kind="stem_fwd", layer="model0.conv1", **stem_plan(B, H, W, num_cus)))
    bn("bn_fwd", L2, [("model0.bn1", 64)])
    for blk in ("model0.layer1.0", "model0.layer1.1"):
        conv(L2, [(blk + ".conv1", 0, 64, 64, 3, 0, 0)])
        bn("bn_fwd", L2, [(blk + ".bn1", 64)])
        conv(L2, [(blk + ".conv2", 0, 64, 64, 3, 0, 0)])
        bn("bn_fwd", L2, [(blk + ".bn2", 64)])
    pool("pool_fwd", L2)
    conv(L4, [("model0.layer2.0.conv1", 0, 64, 128, 3, 0, 0), ("model0.layer2.0.downsample.0", 0, 64, 128, 1, 0, 0)])
    bn("bn_fwd", L4, [("model0.layer2.0.bn1", 128)])
    bn("bn_fwd", L4, [("model0.layer2.0.downsample.1", 128)])
    conv(L4, [("model0.layer2.0.conv2", 0, 128, 128, 3, 0, 0)])
    bn("bn_fwd", L4, [("model0.layer2.0.bn2", 128)])
    conv(L4, [("model0.conv2", 0, 128, 128, 1, 0, 0)])
    bn("bn_fwd", L4, [("model0.bn2", 128)])
    pool("pool_fwd", L4)
    pool("pool_fwd", L4)
    name = lambda st, b, i: "model%d_%d.%d" % (st + 1, b + 1, i)
    in_plane = lambda st, b, lv: (128 if st == 0 else CAT_PLANE) if lv == 0 else BR_C[b][lv - 1]
    for st in (0, 1):
        for lv in range(5):
            conv(L8, [(name(st, b, 3 * lv), 0, in_plane(st, b, lv), BR_C[b][lv] if lv < 4 else HEAD_C[b], BR_KS[b][lv], 0, int(lv == 4)) for b in range(3)])
            if lv < 4:
                bn("bn_fwd", L8, [(name(st, b, 3 * lv + 1), BR_C[b][lv]) for b in range(3)])

    # ---- backward ----
    def stage_bwd(st):
        ops.append(dict(kind="heads", stage=st, H=L8[0], W=L8[1], **head_plan(B, *L8)))
        for lv in range(4, -1, -1):
            if lv < 4:
                bn("bn_bwd", L8, [(name(st, b, 3 * lv + 1), BR_C[b][lv]) for b in range(3)])
            for b in range(3):
                cin = (128 if st == 0 else 187) if lv == 0 else BR_C[b][lv - 1]
                wgrad(L8, name(st, b, 3 * lv), BR_KS[b][lv], cin, BR_C[b][lv] if lv < 4 else HEAD_C[b], in_plane(st, b, lv), cat=st == 1 and lv == 0,
                      dbias_plane=64 if lv == 4 else None)
            conv(L8, [(name(st, b, 3 * lv), 1, 64 if lv == 4 else BR_C[b][lv], in_plane(st, b, lv), BR_KS[b][lv], 0, 0) for b in range(3)])
    stage_bwd(1)
    ops.append(dict(kind="add", C=CAT_PLANE, n=3, H=L8[0], W=L8[1]))
    stage_bwd(0)
    ops.append(dict(kind="add", C=128, n=4, H=L8[0], W=L8[1]))
    pool("pool_bwd", L4)
    bn("bn_bwd", L4, [("model0.bn2", 128)])
    wgrad(L4, "model0.conv2", 1, 128, 128, 128)
    conv(L4, [("model0.conv2", 1, 128, 128, 1, 0, 0)])

    def block_bwd(blk, hw, cin, cout, down):
        bn("bn_bwd", hw, [(blk + ".bn2", cout)])
        wgrad(hw, blk + ".conv2", 3, cout, cout, cout)
        conv(hw, [(blk + ".conv2", 1, cout, cout, 3, 0, 0)])
        bn("bn_bwd", hw, [(blk + ".bn1", cout)])
        wgrad(hw, blk + ".conv1", 3, cin, cout, cin)
        if down:
            bn("bn_bwd", hw, [(blk + ".downsample.1", cout)])
            wgrad(hw, blk + ".downsample.0", 1, cin, cout, cin)
            conv(hw, [(blk + ".downsample.0", 1, cout, cin, 1, 0, 0)])
        conv(hw, [(blk + ".conv1", 1, cout, cin, 3, 1, 0)])
    block_bwd("model0.layer2.0", L4, 64, 128, True)
    pool("pool_bwd", L2)
    block_bwd("model0.layer1.1", L2, 64, 64, False)
    block_bwd("model0.layer1.0", L2, 64, 64, False)
    bn("bn_bwd", L2, [("model0.bn1", 64)])
    ops.append(dict(kind="stem_wgrad", layer="model0.conv1", **stem_plan(B, H, W, num_cus)))
    return ops


# ---- classes ----------------------------------------------------------------------------------------------------------------------------------------
def _b3(n):
    return n if n < 3 else "3+"


def wgrad_classes(op):
    """op: a wgrad op of step_ops, or pn_trainer_op_info's wgrad dict with H, W, B added"""
    return _wgrad_classes(op["ks"], op["H"], op["W"], op["B"], op["tiles_x"], op["Wt"], op["rows_per_block"], op["Sr"])


@functools.lru_cache(None)
def _wgrad_classes(ks, H, W, B, tx, Wt, rpb, Sr):
    seg = 32 - 2 * (ks // 2)
    rows_total = B * tx * H
    p = dict(rows_per_block=rpb, rows_total=rows_total, tiles_x=tx)
    f = "wgrad%d" % ks
    tiles = _b3(tx)
    full = Wt == seg
    ring = "below the ring" if rpb < RING else "the ring" if rpb == RING else "above the ring"
    short_block = rows_total % rpb != 0
    span = wgrad_span(p, H) or {"inside one column"}
    per_lane = _cdiv(Sr, 16)
    out = {(f, "tiles_x", tiles), (f, "Wt == seg_max", full), (f, "short last strip", W % Wt != 0), (f, "rows_per_block", ring),
           (f, "short last block", short_block), (f, "slices per lane", "one slice" if Sr == 1 else _b3(per_lane)),
           (f, "Sr clamped to rows_total", Sr == rows_total and rpb == 1),
           (f, "rows_per_block x short last block", ring, short_block), (f, "Wt == seg_max x tiles_x", full, tiles)}
    for s in span:
        out |= {(f, "block range", s), (f, "block range x tiles_x", s, tiles)}
    return out


def red_classes(family, p):
    """p: red_plan's dict, or npix / C / ppb / nblk of a reported problem"""
    return _red_classes(family, p["npix"], p["ppb"], p["nblk"], p["C"])


@functools.lru_cache(None)
def _red_classes(family, npix, ppb, nblk, C):
    PL = 256 // (C // 8)
    last = npix - (nblk - 1) * ppb
    return {(family, "nblk", "1" if nblk == 1 else "2..64" if nblk <= 64 else "above 64"), (family, "ppb from", "the 8 PL floor" if ppb == 8 * PL else "npix / (4 CUs)"),
            (family, "last block partial", last != ppb), (family, "npix < ppb", npix < ppb), (family, "last block below PL pixels", last < PL), (family, "C", C),
            (family, "npix == 1", npix == 1)}          # one value per channel: bn_finish_kernel's n > 1 branch.  finalize refuses the one shape that has it


def classify(op):
    """The classes of one op (a set of tuples)."""
    k = op["kind"]
    if k == "wgrad":
        return wgrad_classes(op)
    if k in ("bn_fwd", "bn_bwd"):
        return set().union(*[red_classes(k, p) for p in op["problems"]])
    if k == "dbias":
        return red_classes(k, op)
    if k == "heads":
        return {("heads", "nblk == 1", n == 1) for n in op["nblk"]} | {("heads", "partial last block", t % 256 != 0) for t in op["total"]}
    if k in ("pool_fwd", "pool_bwd"):
        return {(k, "input height", "odd" if op["H"] % 2 else "even"), (k, "input width", "odd" if op["W"] % 2 else "even"), (k, "output 1 x 1", (op["Ho"], op["Wo"]) == (1, 1)),
                (k, "input 2 x 2", (op["H"], op["W"]) == (2, 2)), (k, "output height", "odd" if op["Ho"] % 2 else "even"), (k, "output width", "odd" if op["Wo"] % 2 else "even"),
                (k, "one-row map", op["Ho"] == 1), (k, "one-column map", op["Wo"] == 1)}
    if k == "stem_fwd":
        return {(k, "ragged tile column", op["wo"] % 16 != 0), (k, "ragged tile row", op["ho"] % 8 != 0), (k, "more tiles than blocks", op["ntiles"] > op["blocks"])}
    if k == "stem_wgrad":
        return {(k, "one slice", op["slices"] == 1), (k, "short last slice", op["P"] % op["pps"] != 0)}
    if k == "add":
        return {(k, "C", op["C"])}
    assert k == "conv", k
    out = set()
    for q in op["problems"]:
        p, f = q["p"], "dgrad" if q["dgrad"] else "conv"
        out |= {(f, "kernel", p["kernel"]), (f, "residual", bool(q["res"])), (f, "NCHW output", bool(q["nchw"])), (f, "ragged last strip", q["W"] % p["Wt"] != 0),
                (f, "ragged last row tile", q["H"] % p["R"] != 0), (f, "strips", _b3(p["tiles_x"])), (f, "lds_two", p["lds_two"]),
                (f, "problems in the launch", len(op["problems"]))}
        if p["kern"] == 0:                  # the generic kernel's plan conditions of tests/plan_cases.py that depend on the map: present where they hold
            c = PC.Conv(q["layer"], q["kplane"], q["rows"], q["ks"], 1, q["H"], q["W"], q["H"], q["W"], q["B"], q["B"], q.get("prec", "bf16x3"), p, True)
            out |= {(f, name) for name in GENERIC_CONDITIONS if PC.CONDITIONS[name](c)}
        if p["kern"] in (3, 4):
            out.add((f, "strip 30 wide", p["Wt"] == 30))
        if q["ks"] == 3 and q["rows"] >= 64 and p["kern"] in (3, 4):
            b = q["level_blocks"]
            out.add((f, "conv4 by block count", "at the threshold" if b == K4_BLOCKS else "above" if b > K4_BLOCKS else "just below" if b >= K4_BLOCKS - 16 else "below"))
            if p["kern"] == 4:
                out.add((f, "conv4 odd strip count", (q["B"] * p["tiles_per_img"]) % 2 == 1))
    return out


def classes_of(B, H, W, precs=("bf16x3", "fp32"), num_cus=NUM_CUS, convs=True):
    """{class: [op, ...]} of a whole step.  The plans of everything but the convolutions do not depend on the precision."""
    out = {}
    for i, prec in enumerate(precs):
        for op in step_ops(B, H, W, prec, num_cus, convs=convs):
            if i and op["kind"] != "conv":
                continue
            fam = lambda c: (c[0] + " " + prec,) + c[1:] if op["kind"] == "conv" else c
            for c in classify(op):
                out.setdefault(fam(c), []).append(op)
    return out


# ---- the sweep --------------------------------------------------------------------------------------------------------------------------------------
# (name, B, H, W, why); why: classes (classify's tuples) the entry is there for -- each is asserted present in an op of the step, on the CPU against the
# table and on the GPU against what pn_trainer_op_info reports.  The list is a greedy cover of the grid's classes by the smallest frames
# (tests/test_train_plan_cases.py asserts the cover), led by the shapes chosen for a named edge.
SWEEP = []
# the conv4-threshold entry: only the ops whose kernel label differs from the bench configuration's are checked (FILTERED)
K4_ENTRY = "b31_below_conv4"
FILTERED = {K4_ENTRY}


def _sw(name, B, H, W, *why):
    SWEEP.append((name, B, H, W, tuple(why)))


_sw("b2_8x8", 2, 8, 8,
    ('dbias', 'last block below PL pixels', True),
    ('heads', 'nblk == 1', True),
    ('pool_bwd', 'input 2 x 2', True),
    ('pool_bwd', 'one-column map', True),
    ('pool_bwd', 'one-row map', True),
    ('pool_bwd', 'output 1 x 1', True),
    ('pool_fwd', 'input 2 x 2', True),
    ('pool_fwd', 'one-column map', True),
    ('pool_fwd', 'one-row map', True),
    ('pool_fwd', 'output 1 x 1', True),
    ('stem_wgrad', 'one slice', True))
_sw("b1_8x240", 1, 8, 240,
    ('conv fp32', 'kernel', 'conv_mfma_kernel<0, 3, 1, 64, 1>'),
    ('conv fp32', 'strips', 2),
    ('dgrad fp32', 'strips', 2),
    ('wgrad1', 'slices per lane', 'one slice'),
    ('wgrad3', 'Wt == seg_max x tiles_x', True, '3+'),
    ('wgrad3', 'Wt == seg_max x tiles_x', True, 1),
    ('wgrad3', 'Wt == seg_max x tiles_x', True, 2),
    ('wgrad3', 'Wt == seg_max', True),
    ('wgrad3', 'slices per lane', 'one slice'))
_sw("b2_240x8", 2, 240, 8,
    ('conv bf16x3', 'lds_two', 0),
    ('dgrad bf16x3', 'lds_two', 0))
_sw("b2_16x120", 2, 16, 120,
    ('conv bf16x3', 'strip 30 wide', True),
    ('dgrad bf16x3', 'strip 30 wide', True))
_sw("b2_16x128", 2, 16, 128,
    ('conv fp32', 'kernel', 'conv_mfma_kernel<0, 3, 1, 120, 1>'),
    ('dgrad fp32', 'kernel', 'conv_mfma_kernel<0, 3, 1, 120, 1>'),
    ('wgrad1', 'Wt == seg_max x tiles_x', True, 1),
    ('wgrad1', 'Wt == seg_max', True))
_sw("b1_40x256", 1, 40, 256,
    ('conv bf16x3', 'kernel', 'conv_mfma_kernel<1, 3, 1, 64, 3>'),
    ('conv fp32', 'kernel', 'conv_mfma_kernel<0, 3, 1, 120, 0>'),
    ('conv fp32', 'kernel', 'conv_mfma_kernel<0, 3, 1, 64, 3>'),
    ('dgrad fp32', 'kernel', 'conv_mfma_kernel<0, 3, 1, 120, 0>'),
    ('wgrad1', 'Wt == seg_max x tiles_x', True, 2))
_sw("b5_16x240", 5, 16, 240,
    ('dbias', 'nblk', '2..64'))
# B = 31 at the bench size: 217 strips, 436 blocks per stage level -- 12 short of the 448 the bench configuration makes exactly (no smaller frame gets
# within a frame of the threshold: conv3_kernel / conv4_kernel need 4-row strips at least 21 wide, 84 pixels per strip against 112 here)
_sw("b31_below_conv4", 31, 224, 224,
    ('conv bf16x3', 'conv4 by block count', 'just below'),
    ('dgrad bf16x3', 'conv4 by block count', 'just below'))
_sw("b5_208x8", 5, 208, 8,
    ('wgrad1', 'block range x tiles_x', 'image seam', 1),
    ('wgrad1', 'block range', 'image seam'),
    ('wgrad1', 'rows_per_block x short last block', 'below the ring', True),
    ('wgrad1', 'rows_per_block x short last block', 'the ring', False),
    ('wgrad1', 'rows_per_block', 'the ring'),
    ('wgrad1', 'short last block', True),
    ('wgrad3', 'rows_per_block x short last block', 'the ring', False),
    ('wgrad3', 'rows_per_block', 'the ring'))
_sw("b1_8x256", 1, 8, 256,
    ('conv bf16x3', 'kernel', 'conv_mfma_kernel<1, 3, 1, 120, 1>'),
    ('dgrad bf16x3', 'kernel', 'conv_mfma_kernel<1, 3, 1, 120, 1>'))
_sw("b2_136x248", 2, 136, 248,
    ('conv bf16x3', 'kernel', 'conv_mfma_kernel<1, 3, 1, 64, 4>'),
    ('conv fp32', 'kernel', 'conv_mfma_kernel<0, 3, 1, 64, 4>'),
    ('dgrad bf16x3', 'kernel', 'conv_mfma_kernel<1, 3, 1, 64, 4>'),
    ('wgrad1', 'block range x tiles_x', 'image seam', 2),
    ('wgrad1', 'block range x tiles_x', 'strip seam', 2),
    ('wgrad1', 'block range', 'strip seam'),
    ('wgrad3', 'block range x tiles_x', 'image seam', '3+'),
    ('wgrad3', 'block range x tiles_x', 'image seam', 2),
    ('wgrad3', 'block range x tiles_x', 'strip seam', '3+'),
    ('wgrad3', 'block range x tiles_x', 'strip seam', 2),
    ('wgrad3', 'block range', 'strip seam'),
    ('wgrad3', 'rows_per_block x short last block', 'the ring', True))
_sw("b8_136x8", 8, 136, 8,
    ('wgrad1', 'rows_per_block x short last block', 'the ring', True))
_sw("b8_176x8", 8, 176, 8,
    ('wgrad1', 'rows_per_block x short last block', 'above the ring', True))
_sw("b32_8x248", 32, 8, 248,
    ('wgrad3', 'block range x tiles_x', 'whole column', '3+'))



def grid_shapes(cap=None):
    return [(B, H, W) for B in GRID_B for H in GRID_SIDES for W in GRID_SIDES if cap is None or B * H * W <= cap]


@functools.lru_cache(None)
def grid_classes(convs=True):
    """{class: smallest pixel count B * H * W of a grid shape that reaches it}"""
    out = {}
    for B, H, W in grid_shapes():
        px = B * H * W
        if (B, H, W) in [r[1:] for r in REFUSED_SWEEP]:
            continue
        for c in classes_of(B, H, W, convs=convs):
            if px < out.get(c, 1 << 62):
                out[c] = px
    return out


def small_grid_labels():
    """{precision: sorted kernel labels of the forward / data-gradient convolutions of every grid shape within SIZE_CAP} at 256 CUs: the content of
    tests/golden/train_plan_small_grid_labels.json, which the GPU coverage guard reads (tests/test_train_plan_cases.py keeps the file equal to the planner)."""
    out = {"bf16x3": set(), "fp32": set()}
    for c, px in grid_classes().items():
        if c[1] == "kernel" and px <= SIZE_CAP:
            out[c[0].split()[1]].add(c[2])
    return {k: sorted(v) for k, v in out.items()}


def entry_classes(name, B, H, W, convs=True):
    """The classes a configuration's checks reach.  A FILTERED entry checks only the convolutions whose kernel differs from the bench configuration's: it
    counts for the conv4 decision alone."""
    cls = set(classes_of(B, H, W, convs=convs))
    return {c for c in cls if c[1] == "conv4 by block count" and c[2] == "just below"} if name in FILTERED else cls


def reached(shapes, convs=True):
    out = set()
    for name, B, H, W in shapes:
        out |= entry_classes(name, B, H, W, convs)
    return out


def sweep_shapes():
    return [(n, B, H, W) for n, B, H, W, _ in SWEEP]


def census(convs=True):
    g = grid_classes(convs)
    by_shapes = reached(SHAPES, convs) & set(g)
    by_both = (by_shapes | reached(sweep_shapes(), convs)) & set(g)
    exempt = {c for c in g if c in EXEMPT}
    return dict(grid=len(g), shapes=len(by_shapes), both=len(by_both), exempt=len(exempt), missing=sorted(set(g) - by_both - exempt, key=repr))


# Classes the grid reaches only beyond SIZE_CAP (asserted in tests/test_train_plan_cases.py): class -> one-line reason.  Those that SHAPES' bench
# configuration or the conv4-threshold entry run anyway are not listed.
_BLOCKS128 = "128-cout blocks of the generic bf16 kernel: fewer than one per CU (256) below B = 32 on maps of at least 4 x 112 pixels, where they become 64-cout blocks"
EXEMPT = {(f + " bf16x3", "kernel", "conv_mfma_kernel<1, %d, 1, %d, 0>" % kp): _BLOCKS128 for f in ("conv", "dgrad") for kp in ((1, 32), (1, 64), (3, 16), (3, 32), (3, 64))}
EXEMPT[("dgrad bf16x3", "kernel", "conv3_kernel<1, 2, 2, 1, 7, 4>")] = "WP = 2 on the 1x1 shortcut's 64-row data gradient: 1536 strip tiles, B = 32 at 248 x 256 and up"
