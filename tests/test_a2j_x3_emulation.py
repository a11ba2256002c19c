"""The recorded cost of the bf16x3 format on the A2J net (tests/a2j_x3_emulation.py::DEVIATION) is what the emulation gives -- without a GPU.

The small shape (80 x 96, 3 crops) is recomputed here, a few seconds of float64 convolutions; the large one (288 x 288, 2 crops, about 200 GFLOP of
float64) is recorded by the helper's own command line.  Both stay far below the 5e-4 in z above which the mode would not be worth its cost, and
below the north star's 1e-3.
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import a2j_x3_emulation as EMU  # noqa: E402


def test_the_small_shape_reproduces_the_recorded_deviation():
    px, z = EMU.deviation("s")
    print("\nA2J bf16x3 EMULATION 80x96: %.6g px, %.6g (z); recorded %s" % (px, z, EMU.DEVIATION["s"]))
    rpx, rz = EMU.DEVIATION["s"]
    # float64 sums whose order the BLAS and its thread count choose: they agree to about 1e-13, which can move a value across a rounding boundary of
    # the lo plane once in a while (one flip is 2^-17 of one activation among millions) -- 1 % of the constant is far more than that and far less
    # than a missing rounding or product would change it by
    assert abs(px - rpx) <= 1e-2 * rpx and abs(z - rz) <= 1e-2 * rz, (px, z)
    assert px > 0 and z > 0          # the format is not float64


def test_the_format_alone_is_far_inside_the_tolerance():
    for size in ("s", "l"):
        px, z = EMU.DEVIATION[size]
        assert 0 < z < 5e-4 and 0 < px < 1e-3, (size, px, z)


def test_split_planes_carry_sixteen_bits():
    import torch
    v = torch.linspace(-3, 3, 4097, dtype=torch.float64) * 1.2345
    hi, lo = EMU.split(v)
    assert bool((hi == EMU.rne_bf16(hi + lo)).all())
    assert float(((hi + lo) - EMU.f32(v)).abs().max()) <= 2.0 ** -17 * 4
    assert float(((hi + lo) - EMU.f32(v)).abs().max()) > 0
