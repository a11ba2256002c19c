"""fp64 reference of the A2J anchor vote (post_process.forward, anchor.py:57-82) with its allowance, shared by tests/test_gpu_a2j.py and
tests/test_gpu_a2j_crop_edges.py."""
import numpy as np

U = 2.0 ** -24


def vote_reference(cls, reg, dep, anchors):
    """fp64 r = N / Z per (crop, joint) and the allowance 2 (n + rho + 2) 2^-24 sum e_i |v_i| / Z: any fp32 summation order of n terms
    in numerator and denominator, plus expf and the rounding of its argument (rho = 3 + max |c_i - max c|)."""
    c = cls.astype(np.float64)
    d = c - c.max(1, keepdims=True)
    e = np.exp(d)
    Z = e.sum(1)
    v = np.concatenate([anchors[None, :, None, :].astype(np.float64) + reg.astype(np.float64), dep.astype(np.float64)[..., None]], -1)      # [B, K, P, 3]
    r = (e[..., None] * v).sum(1) / Z[..., None]
    n = c.shape[1]
    rho = 3 + np.abs(d).max(1)
    allow = 2 * (n + rho + 2)[..., None] * U * (e[..., None] * np.abs(v)).sum(1) / Z[..., None]
    return r, allow
