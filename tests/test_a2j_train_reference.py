"""The plain-torch statement of the A2J training step (tests/a2j_train_reference.py) is tied to the reference by the fixture
tests/golden/a2j_train.npz, which tests/golden/make_golden_a2j_train.py writes by running the reference itself.  CPU only.

The fp64 run of our statement must equal the stored fp64 values within a TENTH of each stored `*_tol` (4 x the reference's own fp32-fp64
distance): two fp64 runs of the same mathematics differ by rounding that is orders of magnitude below that, while any difference in the
mathematics -- a wrong layer, a wrong loss term -- is far above it (the injected faults below move the terms by 1e-1 and more)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import a2j_cases as AC
import a2j_train_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
REF = "/root/reference"
G = np.load(os.path.join(GOLDEN, "a2j_train.npz"))
G0 = np.load(os.path.join(GOLDEN, "a2j.npz"))


def golden_state_dict(dtype=torch.float64):
    keys = [str(k) for k in G0["keys"]]
    shapes = [tuple(int(v) for v in s[:n]) for s, n in zip(G0["shapes"], G0["ndim"])]
    sd = AC.state_dict_for_seed(AC.SEED, keys, shapes)
    return {k: (v.to(dtype) if v.is_floating_point() else v.clone()) for k, v in sd.items()}


@pytest.fixture(scope="module")
def step64():
    """one fp64 training step of our statement on the golden case: terms, head gradients, parameter gradients, the state dict after it"""
    from popnet_amd.network.a2j import generate_anchors, shift
    H, W, B = AC.SMALL
    sd = golden_state_dict()
    params = [k for k in sd if sd[k].is_floating_point() and not k.endswith("running_mean") and not k.endswith("running_var")]
    for k in params:
        sd[k].requires_grad_(True)
    x = torch.from_numpy(AC.net_input(AC.SEED + H, B, H, W)).double()
    heads, _ = R.forward_train(sd, x)
    for t in heads:
        t.retain_grad()
    anchors = torch.from_numpy(shift([H // 16, W // 16], 16, generate_anchors()))
    labels = torch.from_numpy(G["labels"])
    c, r = R.a2j_loss(heads, labels, anchors, float(G["spatial_factor"]))
    (c + float(G["reg_loss_factor"]) * r).backward()
    return {"terms": np.array([float(c.detach()), float(r.detach())]), "heads": heads, "anchors": anchors, "labels": labels, "sd": sd, "params": params}


def test_fp64_statement_equals_the_reference_step(step64):
    s = step64
    assert bool((np.abs(s["terms"] - G["terms"]) <= 0.1 * G["terms_tol"]).all()), (s["terms"], G["terms"])
    for name, t in zip(("dcls", "dreg", "ddep"), s["heads"]):
        err = np.abs(t.grad.numpy() - G[name]).max()
        assert err <= 0.1 * float(G[name + "_tol"]), (name, err)
    gkeys = [str(k) for k in G["grad_keys"]]
    assert [k for k in s["params"] if s["sd"][k].grad is not None] == gkeys
    assert [k for k in s["params"] if s["sd"][k].grad is None] == ["Backbone.model.fc.weight", "Backbone.model.fc.bias"]
    norms = np.array([float(s["sd"][k].grad.norm()) for k in gkeys])
    assert bool((np.abs(norms - G["grad_norms"]) <= 0.1 * G["grad_norms_tol"] + 1e-12).all())
    flat = torch.cat([s["sd"][k].grad.reshape(-1) for k in gkeys]).numpy()[::int(G["sample_every"])]
    assert np.abs(flat - G["grad_samples"]).max() <= 0.1 * float(G["grad_samples_tol"])
    for k in G.files:
        if k.startswith("stat_") and not k.endswith("_tol"):
            kind, layer = k.split(".", 1)
            got = s["sd"][layer + (".running_mean" if kind == "stat_mean" else ".running_var")].detach().numpy()
            assert np.abs(got - G[k]).max() <= 0.1 * float(G[k + "_tol"]), k
    assert all(int(v) == 1 for k, v in s["sd"].items() if k.endswith("num_batches_tracked"))


def test_fixture_exercises_every_branch(step64):
    heads, anchors, labels = [t.detach() for t in step64["heads"]], step64["anchors"], step64["labels"]
    w = torch.softmax(heads[0], 1)
    d_a = labels[:, :, :2] - (w.unsqueeze(3) * anchors[None, :, None, :]).sum(1)
    d_r = labels[:, :, :2] - (w.unsqueeze(3) * (anchors[None, :, None, :] + heads[1])).sum(1)
    d_z = labels[:, :, 2] - (w * heads[2]).sum(1)
    for d in (d_a, d_r):
        assert bool((d.abs() <= 1).any() and (d.abs() > 1).any() and (d > 0).any() and (d < 0).any())
    assert bool((d_z > 0).any() and (d_z < 0).any() and (d_z.abs() < 3).any() and (d_z.abs() > 3).any())
    assert os.path.getsize(os.path.join(GOLDEN, "a2j_train.npz")) < 1 << 20


@pytest.mark.parametrize("fault", ["smooth_depth", "swap_xy", "no_spatial_factor"])
def test_loss_rejects_injected_faults(step64, fault):
    heads = [t.detach() for t in step64["heads"]]
    c, r = R.a2j_loss(heads, step64["labels"], step64["anchors"], float(G["spatial_factor"]), fault=fault)
    terms = np.array([float(c), float(r)])
    assert bool((np.abs(terms - G["terms"]) > 1e3 * G["terms_tol"]).any()), (fault, terms, G["terms"])


def test_crop_labels_equal_the_reference_cases():
    from popnet_amd.train_a2j import crop_labels
    sys.path.insert(0, GOLDEN)
    import make_golden_a2j_train as M
    assert [str(n) for n in G["label_case_names"]] == [n for n, _ in M.LABEL_CASES]
    for i, (name, box) in enumerate(M.LABEL_CASES):
        j2, j3 = M.label_case_joints(i, box)
        got = crop_labels(box, j2, j3)
        assert got.dtype == np.float32 and np.array_equal(got, G["label_case_labels"][i]), name
    # past each edge at least once, and one box inside
    boxes = G["label_case_boxes"]
    assert (boxes[:, 0] < 0).any() and (boxes[:, 1] < 0).any() and (boxes[:, 2] > 480).any() and (boxes[:, 3] > 512).any()
    assert ((boxes[:, 0] >= 0) & (boxes[:, 1] >= 0) & (boxes[:, 2] <= 480) & (boxes[:, 3] <= 512)).any()


@pytest.mark.parametrize("wd", [0.0, 1e-4])
def test_adam_formula_equals_torch_optim_adam(wd):
    rng = np.random.default_rng(3)
    p0 = rng.normal(0, 1, 257)
    p = torch.tensor(p0, dtype=torch.float64, requires_grad=True)
    opt = torch.optim.Adam([p], lr=0.00035, weight_decay=wd)
    q, m, v = p0.copy(), np.zeros_like(p0), np.zeros_like(p0)
    for t in (1, 2, 3):
        g = rng.normal(0, 1, 257) * 10.0 ** rng.integers(-6, 2, 257)
        p.grad = torch.tensor(g)
        opt.step()
        q, m, v = R.adam_step(q, g, m, v, t, 0.00035, wd=wd)
        assert np.abs(q - p.detach().numpy()).max() <= 1e-15 * (1 + np.abs(q).max())


@pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "third_party_methods", "A2J_experiments")), reason="needs the reference tree")
def test_a2j_train_golden_regenerates():
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, os.path.join(GOLDEN, "make_golden_a2j_train.py"), "--check"], capture_output=True, text=True, cwd=ROOT, env=env,
                       timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "golden check ok: a2j_train.npz regenerates" in r.stdout
