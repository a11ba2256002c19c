"""bench.py's plain line and --dump-outputs: a plain run times the headline region only; the dump holds what the last timed step
returned (its pn_pose_wire records), one float32 / float64 file per field."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def test_dump_outputs_writes_one_float_file_per_record_field(tmp_path):
    """Run in a child: importing bench sets the HIP queue count of the importing process."""
    code = ("import sys, numpy as np; sys.path.insert(0, %r); import bench; from popnet_amd import _lib\n"
            "rec = np.zeros(4, _lib.POSE_WIRE_DTYPE); rec['n_persons'] = [0, 1, 2, 16]; rec['status'][2] = 1\n"
            "rec['person_joint'][1, 0] = np.arange(15) - 1; rec['vals'][3] = np.random.default_rng(0).normal(size=(16, 15, 6))\n"
            "np.save(%r, rec); bench.dump_outputs(%r, {'records': rec})" % (ROOT, str(tmp_path / "rec.npy"), str(tmp_path / "out")))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    from popnet_amd import _lib
    rec = np.load(tmp_path / "rec.npy")
    files = sorted(os.listdir(tmp_path / "out"))
    assert files == sorted("records_%s.npy" % f for f in _lib.POSE_WIRE_DTYPE.names)
    for f in _lib.POSE_WIRE_DTYPE.names:
        a = np.load(tmp_path / "out" / ("records_%s.npy" % f))
        assert a.dtype in (np.float32, np.float64) and a.shape == rec[f].shape
        assert np.array_equal(a, rec[f]) and (a.dtype == np.float64 or rec[f].dtype == np.float32)


@pytest.mark.gpu
def test_plain_bench_line_and_dumped_records_equal_an_engine_run(gpu, tmp_path):
    import torch
    from popnet_amd import _lib, synth
    from popnet_amd.pipeline import PoseEngine
    out_dir = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "7", "--warmup", "2", "--reps", "1",
                        "--pool", "2", "--dump-outputs", str(out_dir)], capture_output=True, text=True, cwd=ROOT, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    out = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert out["steps"] == 7 and out["value"] > 1000 and out["unit"] == "frames/s" and out["higher_is_better"] is True and out["dtype"] == "bf16"
    assert abs(out["value"] - 32 * 1e3 / out["ms_per_step"]) <= 1e-3 * out["value"]
    for moved in ("roofline", "postproc", "h2d_inclusive", "frame_stats", "cpu_baseline", "precision_modes", "parity_mode", "yolo", "train_step"):
        assert moved not in out, moved
    # the dump: the records of the last timed step, equal to what one engine returns for the same input batch
    eng = PoseEngine(precision="bf16", device=gpu, max_batch=32)
    depth = torch.from_numpy(synth.synth_depth(32, 640, 480, seed=out["dump_outputs"]["input_seed"])).to(gpu)
    wire_dev = torch.zeros((32, _lib.POSE_WIRE_DTYPE.itemsize), device=gpu, dtype=torch.uint8)
    eng.predict(depth, None, wire_dev)
    want = wire_dev.cpu().numpy().view(_lib.POSE_WIRE_DTYPE).reshape(-1)
    for f in _lib.POSE_WIRE_DTYPE.names:
        got = np.load(out_dir / ("records_%s.npy" % f))
        assert got.dtype in (np.float32, np.float64)
        assert np.array_equal(got, want[f]), f
    assert (want["status"] == 0).all()
