"""Every launch of the planes training step (TrainEngine "bf16x3" / "fp32", csrc/trainx.hip) against an fp64 host reference of the same operation.

For each configuration a TrainEngine runs one full step; then the step is replayed op by op (pn_trainer_run_ops): before op k the tensors it
reads are read back (pn_trainer_read_tensor / pn_trainer_read_vector; parameters, gradients, running statistics and loss terms live in the
engine's own torch buffers), op k runs alone, and what it wrote is read back.  tests/train_layer_reference.py computes the exact result of the
operation the code defines on those operands and a per-element allowance; every element-wise output is checked on the first, a middle and the
last frame, every reduction output (per-channel vectors, weight / bias gradients, loss terms) whole, and channels outside a written slice must be
unchanged.  The BatchNorm backward's recomputed activation sign is compared with the stored forward output element by element.
"""
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from helpers import state_dict_from_keys, train_case_inputs  # noqa: E402
import layer_reference as LR  # noqa: E402
import train_layer_reference as TL  # noqa: E402
from popnet_amd import _lib  # noqa: E402

pytestmark = pytest.mark.gpu

SHAPES = TL.SHAPES
CONFIGS = [(name + "_" + prec, prec, B, H, W) for name, B, H, W in SHAPES for prec in ("bf16x3", "fp32")]
BENCH = [c for c in CONFIGS if c[0].startswith("bench_")]
QUIET = ("fork", "join")
CHECKED = {}                 # configuration id -> {(op kind, kernel label)} whose outputs Step.check_all compared (the coverage guard reads it)
PN_ERR_INVALID = -1          # include/popnet_hip.h


def _info(eng, tr, k):
    buf = C.create_string_buffer(1 << 16)
    eng._check(_lib.lib().pn_trainer_op_info(tr, k, buf, len(buf)), "pn_trainer_op_info")
    return json.loads(buf.value.decode())


def op_labels(ops):
    return {(op["kind"], k) for op in ops for k in op["kernels"]}


class Step:
    def __init__(self, golden, gpu, prec, B, H, W, seed=0, tag=None):
        from popnet_amd.train import TrainEngine
        self.tag = tag or "%s_%d_%d_%d" % (prec, B, H, W)
        self.prec, self.fmt, self.B, self.gpu = prec, TL.fmt_of(prec), B, gpu
        self.eng = TrainEngine(state_dict_from_keys(golden.keys["rtpose_light3d"], seed=seed), device=gpu, precision=prec)
        self.batch = [torch.from_numpy(a).to(gpu) for a in train_case_inputs(seed=40 + B + H, B=B, H=H, W=W)]
        self.img, self.heat, self.paf, self.z, self.fg = [b.cpu().double() for b in self.batch]
        self.L = _lib.lib()
        self.eng.forward_backward(*self.batch)
        torch.cuda.synchronize()
        self.tr = self.eng._trainer(B, H, W)
        self.net = _info(self.eng, self.tr, -1)
        self.ops = [_info(self.eng, self.tr, k) for k in range(self.L.pn_trainer_num_ops(self.tr))]
        self.frames = sorted({0, B // 2, B - 1})
        self.flips = 0

    # ---- access ----
    def run(self, first, last):
        p = lambda t: C.c_void_p(t.data_ptr())
        b = self.batch
        self.eng._check(self.L.pn_trainer_run_ops(self.tr, p(b[0]), p(b[1]), p(b[2]), p(b[3]), p(b[4]), p(self.eng.loss_terms), first, last,
                                                  _lib.current_stream_ptr(self.gpu)), "pn_trainer_run_ops")
        torch.cuda.synchronize()

    def _raw(self, tid, which, f0, n):
        H, W, pl = self.net["tensors"][tid]
        out = np.empty((n, pl, H, W), np.float32)
        self.eng._check(self.L.pn_trainer_read_tensor(self.tr, tid, which, f0, n, out.ctypes.data_as(C.c_void_p), out.size, _lib.current_stream_ptr(self.gpu)), "pn_trainer_read_tensor")
        return torch.from_numpy(out).to(torch.float64)

    def read(self, tid, frames=None):
        """Act of tensor tid on the given frames (None: all)."""
        spans = [(0, self.B)] if frames is None else [(f, 1) for f in frames]
        if self.prec == "bf16x3":
            hi = torch.cat([self._raw(tid, 1, f, n) for f, n in spans])
            return LR.Act(hi + torch.cat([self._raw(tid, 2, f, n) for f, n in spans]), hi)
        return LR.Act(torch.cat([self._raw(tid, 0, f, n) for f, n in spans]))

    def write(self, tid, v):
        a = np.ascontiguousarray(v.numpy().astype(np.float32))
        self.eng._check(self.L.pn_trainer_write_tensor(self.tr, tid, 0, self.B, a.ctypes.data_as(C.c_void_p), a.size, _lib.current_stream_ptr(self.gpu)), "pn_trainer_write_tensor")

    def vec(self, name, n):
        out = np.empty(n, np.float32)
        self.eng._check(self.L.pn_trainer_read_vector(self.tr, name.encode(), out.ctypes.data_as(C.c_void_p), n, _lib.current_stream_ptr(self.gpu)), "pn_trainer_read_vector")
        return torch.from_numpy(out).to(torch.float64)

    def head_out(self, name):
        b = int(name.rsplit(".", 1)[1])
        return self.vec(name, self.B * TL.HEAD_C[b] * (self.net["H"] // 8) * (self.net["W"] // 8)).view(self.B, TL.HEAD_C[b], self.net["H"] // 8, self.net["W"] // 8)

    def param(self, name):
        return self.eng.p[name].detach().cpu().double()

    def grad(self, name):
        return self.eng.g[name].detach().cpu().double()

    # ---- one op: returns a closure that, after the op has run, yields (name, report) pairs ----
    def prepare(self, op):
        F_, fmt, kind = self.frames, self.fmt, op["kind"]
        cmp4 = lambda g, r, a, fr=None: LR.compare(g, r, a, frames=fr)
        whole = lambda g, r, a: LR.compare(g.reshape(1, -1, 1, 1), r.reshape(1, -1, 1, 1), a.reshape(1, -1, 1, 1))
        exact = lambda g, r: LR.compare(g, r, torch.zeros_like(r))

        def outside(before, after, c0, n):
            """channels of a tensor outside [c0, c0 + n): unchanged, bit for bit"""
            keep = [c for c in range(before.v.shape[1]) if not c0 <= c < c0 + n]
            if not keep:
                return []
            return [("unchanged", exact(after.v[:, keep], before.v[:, keep]))]

        if kind == "conv":
            pre = []
            for p in op["problems"]:
                x = self.read(p["in"]["t"], F_)
                res = self.read(p["res"]["t"], F_) if p["res"] else None
                bias = self.param(p["layer"] + ".bias") if p["bias"] else None
                r, d = TL.conv_ref(p, self.prec, self.param(p["layer"] + ".weight"), bias, x, res)
                pre.append((p, r, d, self.read(p["out"]["t"], F_) if p["out"] else None))

            def post():
                out = []
                for p, r, d, before in pre:
                    nm = "%s %s" % ("dgrad" if p["dgrad"] else "conv", p["layer"])
                    if p["out"]:
                        after = self.read(p["out"]["t"], F_)
                        c0 = p["out"]["coff"]
                        out.append((nm, cmp4(after.v[:, c0:c0 + p["rows"]], r, LR.allowance(r, d, fmt), F_)))
                        out += [(nm + " " + a, b) for a, b in outside(before, after, c0, p["rows"])]
                    if p["nchw"]:
                        out.append((nm + " (nchw)", cmp4(self.head_out(p["nchw"])[F_], r, LR.allowance(r, d, "fp32"), F_)))
                return out
            return post

        if kind == "bn_fwd":
            pre = []
            for p in op["problems"]:
                x = self.read(p["x"]["t"])
                bn = p["bn"]
                st = TL.bn_stats_ref(x.v, self.param(bn + ".weight"), self.param(bn + ".bias"), self.eng.stats[bn + ".running_mean"].cpu().double(),
                                     self.eng.stats[bn + ".running_var"].cpu().double(), TL.chain(p))
                pre.append((p, LR.Act(x.v[F_]), self.read(p["res"]["t"], F_) if p["res"] else None, st))

            def post():
                out = []
                for p, x, res, st in pre:
                    bn, Cn = p["bn"], p["C"]
                    got = {k: self.vec("%s.%s" % (bn, k), Cn) for k in ("mean", "invstd", "scale", "shift")}
                    got["running_mean"], got["running_var"] = self.eng.stats[bn + ".running_mean"].cpu().double(), self.eng.stats[bn + ".running_var"].cpu().double()
                    out += [("bn_fwd %s %s" % (bn, k), whole(got[k], *st[k])) for k in st]
                    r, d = TL.bn_apply_ref(x, got["scale"], got["shift"], res, p["act"])
                    out.append(("bn_fwd %s y" % bn, cmp4(self.read(p["y"]["t"], F_).v, r, LR.allowance(r, d, fmt), F_)))
                return out
            return post

        if kind == "bn_bwd":
            pre = []
            for p in op["problems"]:
                x, dy = self.read(p["x"]["t"]).v, self.read(p["dy"]["t"]).v
                mask = self.read(p["y"]["t"]).v > 0 if p["act"] else None
                bn = p["bn"]
                mean, istd = self.vec(bn + ".mean", p["C"]), self.vec(bn + ".invstd", p["C"])
                pre.append((p, x, dy, mask, mean, istd,
                            TL.bn_bwd_sums_ref(x, dy, mask, mean, istd, self.param(bn + ".weight"), p["act"], TL.chain(p))))

            def post():
                out = []
                for p, xa, dya, maska, mean, istd, sums in pre:
                    bn, Cn = p["bn"], p["C"]
                    x, dy, mask = xa[F_], dya[F_], maska[F_] if p["act"] else None
                    got = {"dbeta": self.grad(bn + ".bias"), "dgamma": self.grad(bn + ".weight")}
                    got.update({k: self.vec("%s.%s" % (bn, k), Cn) for k in ("k1", "k2", "k3")})
                    out += [("bn_bwd %s %s" % (bn, k), whole(got[k], *sums[k])) for k in sums]
                    if not p["dx"]:
                        continue
                    r, d, g, dg = TL.bn_bwd_apply_ref(x, dy, mask, mean, istd, got["k1"], got["k2"], got["k3"], p["act"])
                    gdx = self.read(p["dx"]["t"], F_).v
                    out.append(("bn_bwd %s dx" % bn, cmp4(gdx, r, LR.allowance(r, d, fmt), F_)))
                    if p["act"]:                 # every element of every frame: dx is read whole once more
                        self.flips += TL.mask_disagreements(self.read(p["dx"]["t"]).v, xa, dya, maska, mean, istd, got["k1"], got["k2"], got["k3"], p["act"], fmt)
                    if p["dres"]:
                        out.append(("bn_bwd %s dres" % bn, cmp4(self.read(p["dres"]["t"], F_).v, g, LR.allowance(g, dg, fmt), F_)))
                return out
            return post

        if kind == "dbias":
            r, a = TL.dbias_ref(self.read(op["dy"]["t"]).v, op["cout"], TL.chain(op))
            return lambda: [("dbias " + op["layer"], whole(self.grad(op["layer"] + ".bias"), r, a))]

        if kind == "add":
            Cn = op["out"]["c"]
            r, d = TL.add_ref([self.read(i["t"], F_).v[:, i["coff"]:i["coff"] + Cn] for i in op["ins"]])
            before = self.read(op["out"]["t"], F_)

            def post():
                after = self.read(op["out"]["t"], F_)
                return [("add", cmp4(after.v[:, :Cn], r, LR.allowance(r, d, fmt), F_))] + outside(before, after, 0, Cn)
            return post

        if kind == "pool_fwd":
            Cn, c0 = op["x"]["c"], op["y"]["coff"]
            r, d = LR.avgpool_ref(self.read(op["x"]["t"], F_))
            before = self.read(op["y"]["t"], F_)

            def post():
                after = self.read(op["y"]["t"], F_)
                return [("pool_fwd", cmp4(after.v[:, c0:c0 + Cn], r, LR.allowance(r, d, fmt), F_))] + outside(before, after, c0, Cn)
            return post

        if kind == "pool_bwd":
            H, W, _ = self.net["tensors"][op["dx"]["t"]]
            r, d = TL.pool_bwd_ref(self.read(op["dy"]["t"], F_).v, H, W)
            return lambda: [("pool_bwd", cmp4(self.read(op["dx"]["t"], F_).v, r, LR.allowance(r, d, fmt), F_))]

        if kind == "heads":
            pre = []
            targets = (self.paf, self.heat, self.z)
            for b, h in enumerate(op["heads"]):
                de = self.read(h["dextra"]["t"]).v[:, h["dextra"]["coff"]:h["dextra"]["coff"] + h["C"]] if h["dextra"] else None
                pre.append((h, TL.heads_ref(self.head_out(h["out"]), targets[b], self.fg if h["fg"] else None, de, h["kind"])))

            def post():
                out = []
                for h, (r, d, loss, la) in pre:
                    dv = self.read(h["dv"]["t"]).v
                    out.append(("heads %s dv" % h["out"], cmp4(dv[:, :h["C"]], r, LR.allowance(r, d, fmt))))
                    out.append(("heads %s dv pad" % h["out"], exact(dv[:, h["C"]:], torch.zeros_like(dv[:, h["C"]:]))))
                    out.append(("heads %s loss" % h["out"], whole(self.eng.loss_terms[h["loss"]].cpu().double().view(1), loss.view(1), la.view(1))))
                return out
            return post

        if kind == "wgrad":
            r, a = TL.wgrad_ref(op, self.prec, self.read(op["x"]["t"]), self.read(op["dy"]["t"]))
            name = op["layer"] + ".weight"
            before = self.eng.flat_g.clone()

            def post():
                off, n = self.eng._offsets[name]
                after = self.eng.flat_g
                same = bool(torch.equal(before[:off], after[:off])) and bool(torch.equal(before[off + n:], after[off + n:]))
                return [("wgrad " + op["layer"], whole(self.grad(name), r, a)), ("wgrad %s elsewhere" % op["layer"], {"worst": 0.0 if same else float("inf"), "n_bad": 0 if same else 1, "where": []})]
            return post

        if kind == "stem_fwd":
            r, d = TL.stem_fwd_ref(self.img[F_], self.param("model0.conv1.weight"))
            return lambda: [("stem_fwd", cmp4(self.read(op["out"]["t"], F_).v, r, LR.allowance(r, d, fmt), F_))]

        if kind == "stem_wgrad":
            assert op["bn"] == "model0.bn1"
            a0 = next(p["y"]["t"] for o in self.ops if o["kind"] == "bn_fwd" for p in o["problems"] if p["bn"] == op["bn"])
            v = lambda k: self.vec("%s.%s" % (op["bn"], k), 64)
            r, a = TL.stem_wgrad_ref(self.img, self.read(op["x"]["t"]).v, self.read(op["dy"]["t"]).v, self.read(a0).v > 0, v("mean"), v("invstd"), v("k1"), v("k2"), v("k3"), self.prec)
            return lambda: [("stem_wgrad", whole(self.grad("model0.conv1.weight"), r, a))]

        assert kind == "pack", kind
        return lambda: []

    def check_all(self, which=None):
        """Replays the step op by op; records in CHECKED the (op kind, kernel label) pairs that produced a compared result.  which: a predicate over ops --
        only those are compared (the others still run, in order, so every compared op reads the operands the step gives it); None: all."""
        results = []
        for k, op in enumerate(self.ops):
            post = None if op["kind"] in QUIET or (which is not None and not which(op)) else self.prepare(op)
            self.run(k, k + 1)
            if post:
                reports = post()
                results += [(k, op["kind"], op["kernels"], name, rep) for name, rep in reports]
                if reports:
                    CHECKED.setdefault(self.tag, set()).update((op["kind"], kern) for kern in op["kernels"])
        return results


EXACT = ("unchanged", "dv pad", "elsewhere", " k1", " dres")          # outputs that are copies, zeros or one exactly rounded product: worst == 0 is legitimate


def _report(tag, results):
    by_kind = {}
    for k, kind, _, _, rep in results:
        by_kind[kind] = max(by_kind.get(kind, 0.0), rep["worst"])
    print("\nTRAIN LAYERS %s: %d checks; worst |gpu - r| / allowance per op kind: %s" % (tag, len(results), ", ".join("%s %.3f" % kv for kv in sorted(by_kind.items()))))
    bad = ["op %d %s %s %s: worst %.3g, %d elements over, at (frame, channel, row, col, ratio) %s" % (k, kind, kern, name, rep["worst"], rep["n_bad"], rep["where"])
           for k, kind, kern, name, rep in results if rep["n_bad"]]
    return bad


@pytest.mark.parametrize("cfg", CONFIGS, ids=[c[0] for c in CONFIGS])
def test_every_op_of_the_training_step_within_fp64_allowance(gpu, golden, cfg):
    tag, prec, B, H, W = cfg
    t0 = time.time()
    st = Step(golden, gpu, prec, B, H, W, tag=tag)
    results = st.check_all()
    bad = _report(tag, results)
    print("TRAIN LAYERS %s: BatchNorm-backward mask disagreements with the stored forward output: %d; %.0f s" % (tag, st.flips, time.time() - t0))
    launching = [k for k, op in enumerate(st.ops) if op["kind"] not in QUIET + ("pack",)]
    assert {r[0] for r in results} == set(launching)
    assert not bad, "\n".join(bad)
    assert st.flips == 0
    vacuous = [(r[0], r[3]) for r in results if r[4]["worst"] == 0 and not any(e in r[3] for e in EXACT)]
    assert not vacuous, vacuous


def _to_mine(ref, cat, plane):
    """reference channel order -> this engine's plane channels (the stage-2 input map; pad channels zero)"""
    out = torch.zeros((ref.shape[0], plane) + tuple(ref.shape[2:]), dtype=torch.float64)
    if cat:
        for i, m in enumerate(TL.CAT_MAP):
            if m >= 0:
                out[:, i] = ref[:, m]
    else:
        out[:, :ref.shape[1]] = ref
    return out


def impulse_spots(op, B, Ht, Wd, extended=False):
    """(image, row, column) of the dy impulses for weight-gradient op `op` on a B x Ht x Wd map: a corner, the last pixel of the last image, both sides of a
    column-strip seam and of a rows_per_block boundary.  extended (the shape sweep): both sides of EVERY column-strip seam, of the first and the last
    rows_per_block boundary, of every image seam that lies inside one block (the first and the last such), and the first and last row of the last block."""
    rpb, tiles_x, wt = op["rows_per_block"], op["tiles_x"], op["Wt"]
    rows_total = B * tiles_x * Ht
    spots = {(0, 0, 0), (B - 1, Ht - 1, Wd - 1)}

    def at(row, last_col=False):             # flattened (image, column strip, row) index -> (image, row, first | last column of the strip)
        strip, y = divmod(row, Ht)
        b, tx = divmod(strip, tiles_x)
        if 0 <= row < rows_total:
            spots.add((b, y, min(Wd, (tx + 1) * wt) - 1 if last_col else tx * wt))
    if tiles_x > 1:
        spots |= {(B - 1, Ht // 2, wt - 1), (B - 1, Ht // 2, wt)}
    for row in (rpb - 1, rpb):
        at(row)
    if extended:
        for t in range(1, tiles_x):
            spots |= {(0, Ht - 1, t * wt - 1), (0, Ht - 1, t * wt), (B - 1, 0, t * wt - 1), (B - 1, 0, t * wt)}
        last0 = (rows_total - 1) // rpb * rpb
        for row in (last0 - 1, last0, rows_total - 1):
            at(row)
            at(row, last_col=True)
        seams = [b * tiles_x * Ht for b in range(1, B) if (b * tiles_x * Ht) % rpb != 0]         # image seams that fall inside a block
        for r in seams[:1] + seams[-1:]:
            for row in (r - 1, r):
                at(row)
                at(row, last_col=True)
    return sorted(spots)


def impulse_ops(st, extended=False):
    """[(op index, op)] of the weight gradients that get impulses: the 3x3 one with the widest map; extended: one of every (kernel size, map, plan) the step has."""
    wg = [(k, op) for k, op in enumerate(st.ops) if op["kind"] == "wgrad" and not op["cat"]]
    if not extended:
        return [max((ko for ko in wg if ko[1]["ks"] == 3), key=lambda ko: st.net["tensors"][ko[1]["x"]["t"]][1])]
    seen = {}
    for k, op in wg:
        seen.setdefault((op["ks"], tuple(st.net["tensors"][op["x"]["t"]][:2]), op["rows_per_block"], op["Sr"]), (k, op))
    return list(seen.values())


def integer_probes(st, tag, extended=False, which=None):
    """The body of the integer-probe test for a built Step: returns (convolution problems, weight gradients, impulses, differences).  which: a predicate
    over ops -- only those are probed, and no impulses are run."""
    import torch.nn.functional as F
    B = st.B
    layers = sorted({p["layer"] for op in st.ops if op["kind"] == "conv" for p in op["problems"]})
    for i, name in enumerate(layers):
        st.eng.p[name + ".weight"].copy_(TL.integer_operand(tuple(st.eng.p[name + ".weight"].shape), 1000 + i).float())
        if name + ".bias" in st.eng.p:
            st.eng.p[name + ".bias"].copy_(TL.integer_operand(tuple(st.eng.p[name + ".bias"].shape), 2000 + i).float())
    torch.cuda.synchronize()
    conv_max, wgrad_max = TL.integer_limits(B, st.net["H"], st.net["W"])
    kpack = next(k for k, op in enumerate(st.ops) if op["kind"] == "pack")
    st.run(kpack, kpack + 1)
    F_ = st.frames
    planted = {}

    def plant(tid, valid, seed):
        """integers in channels [0, valid) of tensor tid (all frames), zeros above; returns them"""
        Ht, Wt, plane = st.net["tensors"][tid]
        v = torch.zeros((B, plane, Ht, Wt), dtype=torch.float64)
        v[:, :valid] = TL.integer_operand((B, valid, Ht, Wt), seed)
        st.write(tid, v)
        planted[tid] = v
        return v
    nconv = nwg = nimp = 0
    bad = []
    for k, op in enumerate(st.ops):
        if which is not None and not which(op):
            continue
        if op["kind"] == "conv":
            probs = [p for p in op["problems"] if p["act"] == 0]
            if not probs:
                continue
            assert len(probs) == len(op["problems"])
            planted.clear()
            for p in probs:
                valid_in = p["cout"] if p["dgrad"] else (187 if p["cat"] else p["cin"])
                if p["in"]["t"] not in planted:
                    plant(p["in"]["t"], valid_in, 10 * k)
                if p["res"] and p["res"]["t"] not in planted:
                    plant(p["res"]["t"], p["rows"], 10 * k + 1)
            st.run(k, k + 1)
            for p in probs:
                w = st.param(p["layer"] + ".weight")
                x = planted[p["in"]["t"]][F_]
                if p["dgrad"]:
                    Ht, Wt, _ = st.net["tensors"][p["in"]["t"]]
                    ref = torch.nn.grad.conv2d_input((len(F_), p["cin"], Ht, Wt), w, x[:, :p["cout"]], padding=p["ks"] // 2)
                    ref = _to_mine(ref, p["cat"], p["rows"])
                else:
                    xr = x[:, [TL.CAT_MAP.index(c) for c in range(p["cin"])]] if p["cat"] else x[:, :p["cin"]]
                    ref = F.conv2d(xr, w, st.param(p["layer"] + ".bias") if p["bias"] else None, padding=p["ks"] // 2)
                if p["res"]:
                    ref = ref + planted[p["res"]["t"]][F_][:, :p["rows"]]
                assert float(ref.abs().max()) <= conv_max
                got = st.read(p["out"]["t"], F_).v[:, p["out"]["coff"]:p["out"]["coff"] + p["rows"]]
                nconv += 1
                if not torch.equal(got, ref):
                    d = (got - ref).abs()
                    bad.append("op %d %s %s %s: %d elements differ, first at (frame index, channel, row, col) %s" % (
                        k, op["kernels"], "dgrad" if p["dgrad"] else "conv", p["layer"], int((d > 0).sum()), tuple(int(i) for i in torch.nonzero(d)[0])))
        elif op["kind"] == "wgrad":
            cin_valid = 187 if op["cat"] else op["cin"]
            x = plant(op["x"]["t"], cin_valid, 10 * k + 2)
            dy = plant(op["dy"]["t"], op["cout"], 10 * k + 3)
            st.run(k, k + 1)
            xr = x[:, [TL.CAT_MAP.index(c) for c in range(op["cin"])]] if op["cat"] else x[:, :op["cin"]]
            ref = TL._cw(dy[:, :op["cout"]], xr, op["ks"])
            assert float(ref.abs().max()) <= wgrad_max
            got = st.grad(op["layer"] + ".weight")
            nwg += 1
            if not torch.equal(got, ref):
                d = (got - ref).abs()
                bad.append("op %d %s wgrad %s: %d elements differ, first at (co, ci, ky, kx) %s" % (k, op["kernels"], op["layer"], int((d > 0).sum()), tuple(int(i) for i in torch.nonzero(d)[0])))
    chosen = [] if which is not None else impulse_ops(st, extended)
    for k, op in chosen:
        Ht, Wt_, plane = st.net["tensors"][op["dy"]["t"]]
        pad = op["ks"] // 2
        x = plant(op["x"]["t"], op["cin"], 77)
        xp = F.pad(x[:, :op["cin"]], (pad, pad, pad, pad))
        for n, (b, y, xc) in enumerate(impulse_spots(op, B, Ht, Wt_, extended)):
            dy = torch.zeros((B, plane, Ht, Wt_), dtype=torch.float64)
            co = (7 * n + 3) % op["cout"]
            dy[b, co, y, xc] = 1.0
            st.write(op["dy"]["t"], dy)
            st.run(k, k + 1)
            ref = torch.zeros((op["cout"], op["cin"], op["ks"], op["ks"]), dtype=torch.float64)
            ref[co] = xp[b, :, y:y + op["ks"], xc:xc + op["ks"]]
            nimp += 1
            if not torch.equal(st.grad(op["layer"] + ".weight"), ref):
                bad.append("impulse at (image %d, row %d, col %d) of %s: dW is not the shifted x patch" % (b, y, xc, op["layer"]))
    return nconv, nwg, nimp, bad


@pytest.mark.parametrize("cfg", CONFIGS, ids=[c[0] for c in CONFIGS])
def test_integer_probes_of_every_convolution_and_weight_gradient_are_bit_exact(gpu, golden, cfg):
    """Single ops on planted integer operands in [-3, 3] (weights written into the flat parameter buffer, then the pack op): every hi / lo split is exact and
    every fp32 partial sum is an integer below 2^24 (test_train_layer_reference.py checks the limits at these shapes), so whatever the summation order, forward,
    data gradient (with and without residual) and weight gradient must equal F.conv2d / conv2d_input / the weight-gradient sum in float64 BIT FOR BIT: a single
    missing pixel, strip seam, tile edge or slice shows.  Every convolution problem without an activation (first, middle and last frame) and every
    weight-gradient op (whole); then impulses: one non-zero dy element at a corner, at the last pixel of the last image, on both sides of a column-strip
    seam and of a rows_per_block boundary -- dW must be the shifted x patch.  (The body is integer_probes: tests/test_gpu_train_layer_shapes.py runs it too.)"""
    tag, prec, B, H, W = cfg
    t0 = time.time()
    st = Step(golden, gpu, prec, B, H, W)
    conv_max, wgrad_max = TL.integer_limits(B, H, W)
    assert conv_max < 2 ** 16 and wgrad_max < 2 ** 24
    nconv, nwg, nimp, bad = integer_probes(st, tag)
    print("\nINTEGER PROBES %s: %d convolution problems, %d weight gradients, %d impulses; %d differ; %.0f s" % (tag, nconv, nwg, nimp, len(bad), time.time() - t0))
    assert nconv >= 38 and nwg == sum(op["kind"] == "wgrad" for op in st.ops)
    assert not bad, "\n".join(bad)


def test_a_changed_parameter_reaches_the_next_convolution_through_the_pack_op(gpu, golden):
    """pack: change one weight between two partial runs; after the pack op the convolution that reads it must compute with the new value, and
    without the pack op it must not have seen it."""
    st = Step(golden, gpu, "bf16x3", 2, 48, 64)
    kpack = next(k for k, op in enumerate(st.ops) if op["kind"] == "pack")
    kconv = next(k for k, op in enumerate(st.ops) if op["kind"] == "conv")
    p = st.ops[kconv]["problems"][0]
    st.run(0, kconv)
    w = st.eng.p[p["layer"] + ".weight"]
    w[3, 5, 1, 2] += 0.5
    torch.cuda.synchronize()
    x = st.read(p["in"]["t"])
    r, d = TL.conv_ref(p, st.prec, st.param(p["layer"] + ".weight"), None, x)
    st.run(kconv, kconv + 1)
    stale = LR.compare(st.read(p["out"]["t"]).v, r, LR.allowance(r, d, st.fmt))
    assert stale["n_bad"] > 0                                     # the pack still holds the old weight
    st.run(kpack, kpack + 1)
    st.run(kconv, kconv + 1)
    fresh = LR.compare(st.read(p["out"]["t"]).v, r, LR.allowance(r, d, st.fmt))
    assert fresh["n_bad"] == 0 and 0 < fresh["worst"] <= 1, fresh


def test_coverage_guard_every_bench_op_kernel_is_checked(gpu, golden):
    """Every (op kind, kernel label) pair a bench-shape trainer plans (the pack op apart: it is checked through the convolutions) must be among the pairs
    for which test_every_op_of_the_training_step_within_fp64_allowance compared a result (CHECKED, filled by Step.check_all; a bench configuration that has
    not been checked in this process is checked here).  A planner change that routes a level to another instantiation fails until that one is checked."""
    from popnet_amd.train import TrainEngine

    def labels(cfg):
        _, prec, B, H, W = cfg
        eng = TrainEngine(state_dict_from_keys(golden.keys["rtpose_light3d"], seed=0), device=gpu, precision=prec)
        tr = eng._trainer(B, H, W)
        return op_labels(_info(eng, tr, k) for k in range(_lib.lib().pn_trainer_num_ops(tr)))
    for tag, prec, B, H, W in BENCH:
        if tag not in CHECKED:
            Step(golden, gpu, prec, B, H, W, tag=tag).check_all()
    bench = {kl for c in BENCH for kl in labels(c) if kl[0] != "pack"}
    checked = set().union(*CHECKED.values())
    print("\nbench (op kind, kernel):", sorted(bench))
    assert ("conv", "conv4_kernel") in bench and any(k == "wgrad" for k, _ in bench)
    assert bench <= checked, sorted(bench - checked)
    with_conv4 = [c[0] for c in CONFIGS if ("conv", "conv4_kernel") in labels(c)]
    assert with_conv4 and len(with_conv4) < len(CONFIGS), with_conv4      # one shape where the stage levels take conv4 and one where they do not


def test_diagnostic_entries_reject_bad_arguments(gpu, golden):
    st = Step(golden, gpu, "fp32", 2, 48, 64)
    L, s = st.L, _lib.current_stream_ptr(gpu)
    one = np.empty(st.net["tensors"][0][0] * st.net["tensors"][0][1] * st.net["tensors"][0][2], np.float32)
    ptr = one.ctypes.data_as(C.c_void_p)
    assert L.pn_trainer_read_tensor(st.tr, len(st.net["tensors"]), 0, 0, 1, ptr, one.size, s) == PN_ERR_INVALID
    assert L.pn_trainer_read_tensor(st.tr, -1, 0, 0, 1, ptr, one.size, s) == PN_ERR_INVALID
    assert L.pn_trainer_read_tensor(st.tr, 0, 0, st.B, 1, ptr, one.size, s) == PN_ERR_INVALID
    assert L.pn_trainer_read_tensor(st.tr, 0, 0, 0, 1, ptr, one.size + 1, s) == PN_ERR_INVALID
    assert L.pn_trainer_read_tensor(st.tr, 0, 1, 0, 1, ptr, one.size, s) == PN_ERR_INVALID          # no hi plane in an fp32 trainer
    assert L.pn_trainer_write_tensor(st.tr, 0, 1, st.B, ptr, one.size, s) == PN_ERR_INVALID
    assert L.pn_trainer_read_vector(st.tr, b"model0.bn1.nope", ptr, 64, s) == PN_ERR_INVALID
    assert L.pn_trainer_read_vector(st.tr, b"model0.bn1.mean", ptr, 63, s) == PN_ERR_INVALID
    assert L.pn_trainer_read_vector(st.tr, b"head_out.2.0", ptr, 64, s) == PN_ERR_INVALID
    p = lambda t: C.c_void_p(t.data_ptr())
    run = lambda first, last: L.pn_trainer_run_ops(st.tr, *(p(b) for b in st.batch), p(st.eng.loss_terms), first, last, s)
    assert run(3, 2) == PN_ERR_INVALID and run(-1, 2) == PN_ERR_INVALID and run(0, len(st.ops) + 1) == PN_ERR_INVALID
    assert run(2, 2) == 0                                          # an empty range is valid and launches nothing
    buf = C.create_string_buffer(8)
    assert L.pn_trainer_op_info(st.tr, 0, buf, len(buf)) == PN_ERR_INVALID
    assert L.pn_trainer_op_info(st.tr, len(st.ops), buf, len(buf)) == PN_ERR_INVALID
