"""The split-bf16 1x1 convolution entries (csrc/conv1x1_x3.hip) on a host without a GPU: the ABI, the planner's description of every A2J
trainer shape, the census of plan classes the small GPU cases of tests/test_gpu_conv1x1_x3.py reach, and the old entries' unchanged answers.
Nothing is launched: pn_conv1x1_x3_plan_info and pn_train_conv_plan_info run on device-less contexts."""
import ctypes as C
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conv1x1_x3_cases as CC  # noqa: E402
import nchw_layer_reference as NR  # noqa: E402

PN_ERR_INVALID = -1
ENTRIES = ("pn_conv1x1_x3_forward", "pn_conv1x1_x3_dgrad", "pn_conv1x1_x3_wgrad", "pn_conv1x1_x3_plan_info")
# plan classes of the trainer's shapes that no small GPU case reaches: {class: reason}; at most a tenth of the classes
EXEMPT = {}
# the stride-1 1x1 rows of tests/test_gpu_train_nchw_layers.py ROWS (lines 440-450 pin them to the fp32 kernels in both precisions)
OLD_1X1_ROWS = [(2, 128, 12, 16, 28), (2, 2048, 2, 3, 512), (2, 1024, 2, 3, 2048), (2, 64, 8, 12, 256)]


def _handle():
    return NR.plan_context(True)


def test_new_entries_are_declared_and_exported():
    from popnet_amd import _lib
    L = _lib.lib()
    for name in ENTRIES:
        assert name in _lib._SIGNATURES and name in _lib.declared_symbols()
        assert getattr(L, name) is not None
    raw = C.CDLL(_lib.LIB_PATH)                                   # exported by the library itself, not only known to the wrapper
    for name in ENTRIES:
        assert C.cast(getattr(raw, name), C.c_void_p).value
    header = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "popnet_hip.h")).read()
    for name in ENTRIES:
        assert "int %s(pn_ctx *ctx" % name in header


def test_plan_describes_all_34_layers_at_the_trainer_shapes_as_split_kernels():
    h = _handle()
    layers = CC.a2j_layers(*CC.TRAIN_HW)
    assert len(layers) == 34 and len({n for n, *_ in layers}) == 34
    assert sum(n.endswith("downsample.0") for n, *_ in layers) == 2 and sum(n.endswith("conv1") for n, *_ in layers) == 16
    kept_on_fp32 = []
    for B in CC.TRAIN_BATCHES:
        for name, Cin, HW, Cout in layers:
            for role in CC.ROLES:
                p = CC.plan(h, role, B, Cin, HW, Cout)
                assert p["BK"] == 32 and len(p["grid"]) == 3 and all(g >= 1 for g in p["grid"]), (name, role, p)
                if p["kernel"] not in CC.SPLIT_KERNELS:
                    kept_on_fp32.append((B, name, role, p["kernel"], p.get("reason")))
                    continue
                assert p["split"] is True
                if role == "wgrad":
                    assert p["grid"] == [-(-Cin // p["BN"]), -(-Cout // p["BM"]), p["slices"]]
                    assert p["per_slice"] == p["per_slice_chunks"] * p["BK"] and p["per_slice_unit"] == "pixels"
                    assert p["chunks"] == B * -(-HW // p["BK"]) and p["chunks_per_image"] == -(-HW // p["BK"])
                    assert (p["slices"] - 1) * p["per_slice_chunks"] < p["chunks"] <= p["slices"] * p["per_slice_chunks"]        # no empty slice
                    assert p["csl"] == NR.reduce_slices(h, B, Cout, HW) >= 1
                    assert p["aligned"] == (HW % 4 == 0) and p["kernel"].endswith("<vec>" if p["aligned"] else "<scalar>")
                else:
                    M, K = (Cin, Cout) if role == "dgrad" else (Cout, Cin)
                    assert (p["M"], p["K"], p["P"]) == (M, K, B * HW) and p["chunks"] == -(-K // 32)
                    assert p["grid"] == [-(-B * HW // p["BN"]), -(-M // p["BM"]), 1]
                    assert p["lds"] <= 64 * 1024
    print("\nCONV1X1 X3 PLAN: 34 layers x %s crops x 3 roles; kept on the fp32 kernels: %s" % (CC.TRAIN_BATCHES, kept_on_fp32 or "none"))
    for row in kept_on_fp32:                 # a shape the planner keeps on fp32 is listed with its reason
        assert isinstance(row[4], str) and row[4], row


def test_small_gpu_cases_reach_every_plan_class_of_the_trainer_shapes():
    h = _handle()
    train, small = CC.classes_of(h, CC.trainer_shapes()), CC.classes_of(h, CC.gpu_shapes())
    missing = sorted(set(train) - set(small) - set(EXEMPT))
    print("\nCONV1X1 X3 CENSUS: classes at the trainer shapes %d / reached by the GPU cases %d (of their own %d) / exempt %d" % (
        len(train), len(set(train) & set(small)), len(small), len(EXEMPT)))
    for cl in sorted(train):
        print("   ", cl, "<-", small.get(cl, ["EXEMPT: " + EXEMPT.get(cl, "?")])[0])
    assert not missing, "\n".join("%r (e.g. %r)" % (cl, train[cl][0]) for cl in missing)
    assert all(isinstance(why, str) and why and "\n" not in why for why in EXEMPT.values())
    assert set(EXEMPT) <= set(train) and 10 * len(EXEMPT) <= len(train)
    # the edges the issue names are among the GPU cases' own classes
    flat = {(cl[0], word) for cl in small for word in cl[2:]}
    for role in ("forward", "dgrad"):
        assert {(role, "K tail"), (role, "ragged channel block"), (role, "ragged pixel tile"), (role, "one chunk"), (role, "chunks")} <= flat
    assert {("wgrad", w) for w in ("ragged Cout block", "ragged Cin block", "ragged chunk at the image end", "one slice", "slices", "ragged last slice",
                                   "aligned rows", "unaligned rows")} <= flat
    # tiny K is not sent back to fp32
    for N, Cin, HW, Cout in CC.gpu_shapes():
        for role in CC.ROLES:
            assert CC.plan(h, role, N, Cin, HW, Cout)["kernel"] in CC.SPLIT_KERNELS


def test_plan_info_refuses_bad_arguments_and_short_buffers():
    from popnet_amd import _lib
    L, h = _lib.lib(), _handle()
    buf = C.create_string_buffer(1024)
    assert L.pn_conv1x1_x3_plan_info(None, 0, 1, 1, 1, 1, buf, 1024) == PN_ERR_INVALID
    for args in ((0, 0, 8, 8, 8), (0, 1, 0, 8, 8), (0, 1, 8, 0, 8), (0, 1, 8, 8, 0), (2, 1, 8, 8, 8), (4, 1, 8, 8, 8), (-1, 1, 8, 8, 8)):
        assert L.pn_conv1x1_x3_plan_info(h, *args, buf, 1024) == PN_ERR_INVALID, args
    assert L.pn_conv1x1_x3_plan_info(h, 0, 1, 8, 8, 8, buf, 16) == PN_ERR_INVALID
    assert L.pn_conv1x1_x3_plan_info(h, 0, 1, 8, 8, 8, None, 1024) == PN_ERR_INVALID
    # the launching entries on a device-less context: refused, nothing to launch on
    assert L.pn_conv1x1_x3_forward(h, None, None, None, None, 1, 1, 1, 1, 0, None) != 0
    assert L.pn_conv1x1_x3_forward(None, None, None, None, None, 1, 1, 1, 1, 0, None) == PN_ERR_INVALID


def test_old_entries_still_plan_every_1x1_call_on_the_fp32_kernels():
    """pn_train_conv_plan_info, in both precisions: the labels tests/test_gpu_train_nchw_layers.py ROWS pins, and every A2J trainer shape."""
    shapes = [(N, Cin, H, W, Cout) for N, Cin, H, W, Cout in OLD_1X1_ROWS]
    side = CC.TRAIN_HW[0]
    for B in CC.TRAIN_BATCHES:
        for _, Cin, HW, Cout in CC.a2j_layers(*CC.TRAIN_HW):
            w = {5184: side // 4, 1296: side // 8, 324: side // 16}[HW]
            shapes.append((B, Cin, HW // w, w, Cout))
    for x3 in (False, True):
        h = NR.plan_context(x3)
        for N, Cin, H, W, Cout in shapes:
            got = tuple(NR.plan(h, which, N, Cin, H, W, Cout, 1, 1, 0)["kernel"] for which in ("forward", "dgrad", "wgrad"))
            assert got == ("tconv_fwd_kernel<1>", "tconv_fwd_kernel<1>", "tconv_wgrad_kernel<1>"), (x3, N, Cin, H, W, Cout, got)
    assert not any(k.startswith("conv1x1") for k in NR.X3_KERNELS)
