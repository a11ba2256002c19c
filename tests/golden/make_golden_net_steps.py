"""Recipe of tests/golden/net_steps.json.gz: the compiled step list of every inference net the GPU suites compile.

Each net is compiled through the C ABI alone -- pn_net_create, pn_net_set_tensor from a CPU state dict, pn_net_finalize -- and right after
finalize, before any forward, pn_net_step_info is dumped for k = -1 .. n - 1.  The nets:

  every entry of test_gpu_layers.CONFIGS with its environment (the two reference-default topologies included),
  every case of test_gpu_layer_shapes.CASES, POPNET_MAX_BATCH honoured as network/_hipnet.py::_compile honours it,
  the A2J nets tests/test_gpu_a2j.py compiles: the rows of tests/a2j_plan_cases.py, each at its max_batch.

The recorded file was written on an MI355X (--device 0) by the last commit whose pn_net_finalize needed a device; a context without a device
(--device -1, the default) must reproduce it: the step list is decided on the host (tests/test_net_steps.py).  The A2J rows added with
tests/a2j_plan_cases.py were written without a device, the older entries reproduced byte for byte beside them; tests/test_gpu_a2j.py compares the
kernel labels of the deployed plans as a device compiles them with the device-less list.  A convolution's "cin_map" is
stored as [length, sha256 of its decimal text], which keeps the file small.  The lists of nets are those of the GPU test modules themselves, imported
here (they import without a GPU), so this recipe and tests/test_net_steps.py follow them and depend on their importing.

  python tests/golden/make_golden_net_steps.py [--device N] [--out FILE]
"""
import ctypes as C
import gzip
import hashlib
import json
import os
import re
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
ROOT = os.path.dirname(TESTS)
for _p in (ROOT, TESTS):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import a2j_cases as AC  # noqa: E402
import a2j_plan_cases as APC  # noqa: E402
import plan_cases as PC  # noqa: E402
import test_gpu_layers as GL  # noqa: E402
import test_gpu_layer_shapes as GS  # noqa: E402
from popnet_amd import _lib  # noqa: E402

OUT = os.path.join(HERE, "net_steps.json.gz")
# tests/test_gpu_a2j.py compiles the rows of tests/a2j_plan_cases.py and nothing else: (H, W, B run, max_batch compiled, precision) of each row -- the
# fixture shapes, the wider pitch classes, the plans the engines deploy (288 x 288 at max_batch 32 / 16 / 2) and the census's additions.  Not covered:
# YoloA2JEngine at crop 96, whose instance keys tests/test_a2j_plan_cases.py shows to be among the compared ones.
A2J_SHAPES = [(H, W, B, mb, prec) for _, prec, H, W, B, mb, _ in APC.CASES]
PREC = {"fp32": _lib.PN_PREC_F32, "bf16": _lib.PN_PREC_BF16, "bf16x3": _lib.PN_PREC_BF16X3}
_CIN_MAP = re.compile(r'"cin_map": \[([^\]]*)\]')


def nets():
    """[(id, network, precision, max_batch, H, W, reference default topology, environment)]"""
    out = []
    for id_, kind, prec, B, H, W, default, env in GL.CONFIGS + [c[0] for c in GS.CASES]:
        env = dict(env)
        mb = max(B, int(env.pop("POPNET_MAX_BATCH", "0")))
        out.append((id_, kind, prec, mb, H, W, default, env))
    for H, W, B, mb, prec in A2J_SHAPES:
        out.append((APC.case_id(prec, H, W, B, mb), "a2j", prec, mb, H, W, False, {}))
    assert len({n[0] for n in out}) == len(out)
    return out


BENCH_IDS = [c[0] for c in GL.BENCH]
GPU_IDS = BENCH_IDS + ["rt_224_b5_bf16_conv4", "a2j_80x96_b3_bf16", "a2j_80x96_b3_fp32"]      # what the GPU test of tests/test_net_steps.py compiles


class _Keys:
    keys = json.load(open(os.path.join(HERE, "state_dict_keys.json")))


_SD = {}


def state_dict(kind, default):
    """(net kind, num_parts, a, input_dim), {name: float32 array}: what HipNetModule._compile hands to pn_net_set_tensor."""
    key = (kind, default)
    if key not in _SD:
        if kind == "a2j":
            g = np.load(os.path.join(HERE, "a2j.npz"))
            shapes = [tuple(int(v) for v in s[:n]) for s, n in zip(g["shapes"], g["ndim"])]
            sd = AC.state_dict_for_seed(int(g["seed"]), [str(k) for k in g["keys"]], shapes)
            args = (_lib.PN_NET_A2J, 15, 16, 1)
        else:
            m = GL._model(_Keys, kind, default)
            sd, args = m.state_dict(), m._net_args()
        _SD[key] = (args, {k: np.ascontiguousarray(v.detach().to("cpu", torch.float32).numpy()) for k, v in sd.items()
                           if not k.endswith("num_batches_tracked") and not k.startswith("model0.layer3.")})
    return _SD[key]


def last_error(ctx):
    buf = C.create_string_buffer(1024)
    _lib.lib().pn_last_error(ctx, buf, len(buf))
    return buf.value.decode()


def compile_net(ctx, net):
    """-> pn_net handle, finalized under the net's environment.  The caller destroys it."""
    _, kind, prec, mb, H, W, default, env = net
    L = _lib.lib()
    args, sd = state_dict(kind, default)
    h = L.pn_net_create(ctx, *args)
    assert h, last_error(ctx)
    for name, arr in sd.items():
        rc = L.pn_net_set_tensor(h, name.encode(), arr.ctypes.data_as(C.c_void_p), (C.c_int64 * arr.ndim)(*arr.shape), arr.ndim)
        assert rc == 0, (name, rc, last_error(ctx))
    with PC.environment(env):
        rc = L.pn_net_finalize(h, PREC[prec], mb, H, W)
    if rc != 0:
        msg = last_error(ctx)
        L.pn_net_destroy(h)
        raise AssertionError("pn_net_finalize(%s) = %d: %s" % (net[0], rc, msg))
    return h


def short_cin_map(text):
    return _CIN_MAP.sub(lambda m: '"cin_map": [%d, "%s"]' % (len(m.group(1).split(",")) if m.group(1) else 0, hashlib.sha256(m.group(1).encode()).hexdigest()), text)


def step_texts(ctx, h):
    """pn_net_step_info of k = -1 .. n - 1, as text, cin_map shortened."""
    L = _lib.lib()
    buf = C.create_string_buffer(1 << 16)
    n = L.pn_net_num_steps(h)
    assert n > 0, last_error(ctx)
    out = []
    for k in range(-1, n):
        rc = L.pn_net_step_info(h, k, buf, len(buf))
        assert rc == 0, (k, rc, last_error(ctx))
        out.append(short_cin_map(buf.value.decode()))
    return out


def a2j_steps(ctx, prec, max_batch, H, W):
    """The steps of one A2J net as pn_net_step_info gives them (parsed, cin_map kept): what tests/a2j_plan_cases.py's instance keys are read from."""
    L = _lib.lib()
    h = compile_net(ctx, ("a2j", "a2j", prec, max_batch, H, W, False, {}))
    try:
        buf = C.create_string_buffer(1 << 16)
        out = []
        for k in range(L.pn_net_num_steps(h)):
            rc = L.pn_net_step_info(h, k, buf, len(buf))
            assert rc == 0, (k, rc, last_error(ctx))
            out.append(json.loads(buf.value.decode()))
        return out
    finally:
        L.pn_net_destroy(h)


def net_steps(ctx, net):
    h = compile_net(ctx, net)
    try:
        return step_texts(ctx, h)
    finally:
        _lib.lib().pn_net_destroy(h)


def load(path=OUT):
    with gzip.open(path, "rt") as f:
        return json.load(f)


def main(argv):
    device = int(argv[argv.index("--device") + 1]) if "--device" in argv else -1
    out = argv[argv.index("--out") + 1] if "--out" in argv else OUT
    ctx = _lib.lib().pn_create(device)
    rec = {}
    for net in nets():
        rec[net[0]] = net_steps(ctx, net)
        print(net[0], len(rec[net[0]]) - 1, "steps", flush=True)
    with open(out, "wb") as raw, gzip.GzipFile(filename="", mode="wb", fileobj=raw, mtime=0) as f:
        f.write(json.dumps(rec, indent=0, sort_keys=True).encode())
    print("wrote %s: %d nets, %d bytes" % (out, len(rec), os.path.getsize(out)))


if __name__ == "__main__":
    main(sys.argv[1:])
