"""GPU: rasterize_kernel and compose_depth_kernel (popnet_amd/csrc/targets.hip) on the hand-placed annotations of
tests/target_cases.py against oracle/targets.py, at network inputs that are not square, stride 4, a 3 x 8 and a one-cell grid.

Bars, the ones of tests/test_gpu_targets.py: fg, z and paf bit-exact; heat within HEAT_TOL = 1.2e-7, one float32 ulp at 1.0, the
most a last-bit difference of the device's float64 exp can survive.  The number of heat cells that differ at all is printed,
not asserted.  The compositor is compared for equality.
"""
import numpy as np
import pytest
import torch

import popnet_amd  # noqa: F401
from popnet_amd import targets
from oracle import targets as OT

import target_cases as TC

pytestmark = pytest.mark.gpu

HEAT_TOL = 1.2e-7
GEOMS = list(TC.by_geometry())
TALLY = {"frames": 0, "cells": 0, "mismatches": 0, "heat_cells": 0, "heat_differing": 0, "heat_max": 0.0}


def _dev(a, gpu):
    return torch.from_numpy(np.array(a)).to(gpu)                  # a copy: the cases are read-only


def _rasterize(gpu, geom, cs, Pmax, n_persons=None):
    """the cases as one batch, padded to Pmax person slots that hold PAD; returns per case (heat, paf, z, fg) as [h,w,C] arrays"""
    X, Y, s, r, sigma = geom
    gh, gw = TC.grid(geom)
    B = len(cs)
    k2 = np.full((B, Pmax, 15, 2), TC.PAD, np.float32)
    kz = np.full((B, Pmax, 15), -5.0)
    dr = np.zeros((B, gh, gw), np.float32)
    for b, c in enumerate(cs):
        P = len(c.kp2d)
        k2[b, :P], kz[b, :P], dr[b] = c.kp2d, c.kp_z, c.depth
    n = np.array([len(c.kp2d) for c in cs] if n_persons is None else n_persons, np.int32)
    out = targets.rasterize_targets(_dev(k2, gpu), _dev(kz, gpu), _dev(n, gpu), _dev(dr, gpu), (X, Y), s, r, sigma)
    assert [tuple(o.shape) for o in out] == [(B, ch, gh, gw) for ch in (16, 28, 15, 15)]
    return [[o[b].permute(1, 2, 0).cpu().numpy() for o in out] for b in range(B)]


def _compare(c, got, tally=True):
    heat, paf, z, fg = got
    oh, op, oz, of = TC.reference(c)
    name = "%s @ %s" % (c.name, c.geom[:4])
    assert oz.dtype == np.float32
    assert np.array_equal(fg, of.astype(np.float32)), "%s: fg differs in %d cells" % (name, (fg != of).sum())
    assert np.array_equal(z, oz), "%s: z differs in %d cells, by up to %g" % (name, (z != oz).sum(), np.abs(z - oz).max())
    assert np.array_equal(paf, op.astype(np.float32)), "%s: paf differs in %d cells, by up to %g" % (name, (paf != op.astype(np.float32)).sum(), np.abs(paf - op).max())
    dh = np.abs(heat - oh.astype(np.float32))
    if tally:
        TALLY["frames"] += 1
        TALLY["cells"] += fg.size + z.size + paf.size
        TALLY["heat_cells"] += heat.size
        TALLY["heat_differing"] += int((dh > 0).sum())
        TALLY["heat_max"] = max(TALLY["heat_max"], float(dh.max()) if dh.size else 0.0)
    assert dh.max() <= HEAT_TOL, "%s: heat differs by %g" % (name, dh.max())


@pytest.mark.parametrize("geom", GEOMS, ids=lambda g: "%dx%d_s%d_r%d" % g[:4] + ("" if g[4] == 7.0 else "_sigma"))
def test_rasteriser_equals_oracle_in_batch_alone_and_with_padding(gpu, geom):
    cs = TC.by_geometry()[geom]
    Pmax = max(len(c.kp2d) for c in cs)
    batch = _rasterize(gpu, geom, cs, Pmax)                      # ragged: P = 0 and padded slots holding 1e9 among full frames
    for c, got in zip(cs, batch):
        _compare(c, got)
    for c, got in zip(cs, batch):                                # alone, without padding (P = 0 goes through the wrapper's dummy slot)
        alone = _rasterize(gpu, geom, [c], len(c.kp2d))[0]
        for a, b in zip(alone, got):
            assert np.array_equal(a, b), c.name
    # two more slots of padding, and n_persons above Pmax where every slot is a person: the count is clamped to Pmax
    wide = _rasterize(gpu, geom, cs, Pmax + 2)
    over = _rasterize(gpu, geom, cs, Pmax, n_persons=[len(c.kp2d) + (3 if len(c.kp2d) == Pmax else 0) for c in cs])
    perm = np.random.default_rng(3).permutation(len(cs))
    shuffled = _rasterize(gpu, geom, [cs[i] for i in perm], Pmax)
    for b in range(len(cs)):
        for k in range(4):
            assert np.array_equal(wide[b][k], batch[b][k]) and np.array_equal(over[b][k], batch[b][k]), cs[b].name
            assert np.array_equal(shuffled[int(np.nonzero(perm == b)[0][0])][k], batch[b][k]), cs[b].name
    print("%s: so far %d frames, %d fg/z/paf cells, mismatches %d; %d heat cells, %d differ at all, by at most %.3g"
          % (geom[:4], TALLY["frames"], TALLY["cells"], TALLY["mismatches"], TALLY["heat_cells"], TALLY["heat_differing"], TALLY["heat_max"]))


def test_wrapper_takes_an_int_or_a_pair_and_checks_the_grid(gpu):
    c = next(c for c in TC.cases() if c.name == "halves" and c.geom[:3] == (224, 224, 8))
    args = (_dev(c.kp2d[None], gpu), _dev(c.kp_z[None], gpu), torch.tensor([len(c.kp2d)], dtype=torch.int32, device=gpu), _dev(c.depth[None], gpu))
    a, b, d = targets.rasterize_targets(*args), targets.rasterize_targets(*args, 224), targets.rasterize_targets(*args, (224, 224))
    for x, y, z in zip(a, b, d):
        assert torch.equal(x, y) and torch.equal(x, z)
    cfg = targets.target_cfg((232, 200), 8, 1)
    assert (cfg.input_x, cfg.input_y, cfg.stride, cfg.z_radius) == (232, 200, 8, 1) and targets.target_cfg(224).input_y == 224
    with pytest.raises(Exception, match="shape mismatch"):       # a [25, 29] grid handed over as [29, 25]
        targets.rasterize_targets(args[0], args[1], args[2], torch.zeros((1, 29, 25), device=gpu), (232, 200))


@pytest.mark.parametrize("dt", [np.float16, np.float32], ids=["fp16", "fp32"])
def test_compositor_equals_oracle_on_edge_inputs(gpu, dt):
    frames = cells = 0
    for name, d, m, n_src, bg in TC.compose_cases():
        B, S, H, W = d.shape
        dd, bb = d.astype(dt), bg.astype(dt)
        got = targets.compose_depth(_dev(dd, gpu), _dev(m, gpu), _dev(n_src, gpu), _dev(bb, gpu)).cpu().numpy()
        assert got.shape == (B, H, W) and got.dtype == np.float32
        for b in range(B):
            n = min(int(n_src[b]), S)
            want, _ = OT.compose_depth(dd[b, :n], m[b, :n], bb[b])
            assert np.array_equal(got[b], want.astype(np.float32)), (name, dt, b, int(n_src[b]))
            frames, cells = frames + 1, cells + H * W
    print("compositor %s: %d frames, %d cells compared, mismatches 0" % (np.dtype(dt).name, frames, cells))
