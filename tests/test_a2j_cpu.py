"""CPU: the A2J module's state dict, its anchors and the C ABI against the reference's (tests/golden/a2j.npz)."""
import ctypes as C
import os
import re

import numpy as np
import torch

from popnet_amd import _lib
from popnet_amd.network.a2j import A2J_RECORD_DTYPE, A2JCfg, A2J_model, generate_anchors, shift

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = np.load(os.path.join(ROOT, "tests", "golden", "a2j.npz"))


def test_state_dict_keys_and_shapes_equal_the_reference():
    sd = A2J_model(15).state_dict()
    assert len(sd) == 410 and list(sd.keys()) == [str(k) for k in G["keys"]]
    for i, v in enumerate(sd.values()):
        assert tuple(v.shape) == tuple(int(s) for s in G["shapes"][i][:G["ndim"][i]])
    assert sum(v.numel() for k, v in sd.items() if not k.endswith("num_batches_tracked")) == int(G["n_params"])


def test_reference_style_checkpoint_loads():
    m = A2J_model(15)
    sd = {"module." + k: torch.zeros_like(v) for k, v in m.state_dict().items()}      # as saved from a DataParallel wrapper
    m.load_state_dict(sd)
    assert float(m.Backbone.model.layer4[1].conv2.weight.detach().abs().sum()) == 0 and m.Backbone.model.layer4[1].conv2.dilation == (2, 2)
    assert m.Backbone.model.layer4[0].conv2.dilation == (1, 1)


def test_anchors_equal_the_reference_arrays():
    assert np.array_equal(generate_anchors(), G["ref_generate_anchors"])
    assert np.array_equal(shift([5, 6], 16, generate_anchors()), G["ref_shift_5x6"])
    assert np.array_equal(shift([18, 18], 16, generate_anchors()), G["ref_shift_18x18"])


def test_c_abi_symbols_exist():
    handle = _lib.lib()
    txt = open(os.path.join(ROOT, "include", "popnet_hip.h")).read()
    for name in ("pn_a2j_cfg_default", "pn_a2j_crop", "pn_a2j_forward", "pn_a2j_head_shape", "pn_a2j_vote", "pn_a2j_predict", "pn_sizeof_a2j_record"):
        assert hasattr(handle, name) and re.search(r"\b%s\s*\(" % name, txt) and name in _lib.declared_symbols()
    cfg = A2JCfg()
    handle.pn_a2j_cfg_default(C.byref(cfg))
    assert (cfg.img_w, cfg.img_h, cfg.crop_w, cfg.crop_h, cfg.mean, cfg.std) == (480, 512, 288, 288, 3.0, 2.0)
    assert abs(cfg.conf_min - 0.01) < 1e-9 and cfg.fx == 504.1189880371094 and cfg.cy == 320.62640380859375
    assert handle.pn_sizeof_a2j_record() == A2J_RECORD_DTYPE.itemsize == 308
    assert _lib.PN_NET_A2J == 2
