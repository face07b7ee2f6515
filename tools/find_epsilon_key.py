#!/usr/bin/env python3
"""Find an RNG key for tests/ref_sweep.py's geometric case at which the
`- FLT_EPSILON` of the view selection (src/ACMMP.cu:1036) decides a draw.

The rule matters only when a uniform lies within FLT_EPSILON above a step of a
pixel's CDF, about once in 10^7 draws, so no scene reaches it by chance. The
geometric case's init draws nothing: the CDFs of its first half-sweep do not
depend on the key, and the key can be searched with the CDFs held fixed.
For every key the 15 view draws of every black pixel are computed (Philox in
numpy, checked against the oracle's) and the views picked with and without the
epsilon are compared. Prints the first key that differs; put it into
make_case("geom") as seed_lo when the case's inputs have changed and
test_every_changed_rule_is_noticed[no_epsilon] fails. CPU only, seconds.

    python tools/find_epsilon_key.py [first_key] [last_key]
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")):
    sys.path.insert(0, p)

import oracle  # noqa: E402
import ref_sweep as rs  # noqa: E402

F = np.float32


def philox4(k0, k1, c0, c1, c2, c3):
    """Philox4x32-10 on arrays of counters: (..., 4) output words."""
    m = np.uint64(0xFFFFFFFF)
    c0, c1, c2, c3 = (np.asarray(c, np.uint64) for c in (c0, c1, c2, c3))
    k0, k1 = np.uint64(k0), np.uint64(k1)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = ((p1 >> np.uint64(32)) ^ c1 ^ k0) & m, p1 & m, ((p0 >> np.uint64(32)) ^ c3 ^ k1) & m, p0 & m
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & m, (k1 + np.uint64(0xBB67AE85)) & m
    return np.stack([c0, c1, c2, c3], -1)


def main():
    lo = int(sys.argv[1]) if len(sys.argv) > 1 else 1
    hi = int(sys.argv[2]) if len(sys.argv) > 2 else 100000
    assert philox4(1, 2, [3], [4], [5], [6])[0].tolist() == oracle.philox4(1, 2, 3, 4, 5, 6)
    prob = rs.make_case("geom")
    r = rs.SweepRestated(prob, rs.OracleBackend(prob))
    r.init()
    r.half_sweep(0, 0)
    tr = r.traces[0]
    cdf, pix = tr.extra["cdf"], tr.ys * r.W + tr.xs
    P = len(pix)
    scale = F(2.3283064365386963e-10)
    for key in range(lo, hi):
        # draw d of (pixel, phase 1, stream): word d mod 4 of block d div 4
        words = np.stack([philox4(key, prob.prm.seed_hi, pix, np.full(P, b), np.full(P, 1),
                                  np.full(P, prob.prm.rng_stream)) for b in range(4)], 1).reshape(P, 16)[:, :15]
        u = words.astype(F) * scale + scale / F(2)
        with np.errstate(invalid="ignore"):
            a = cdf[:, None, :] > (u - rs.FLT_EPSILON)[:, :, None]
            b = cdf[:, None, :] > u[:, :, None]
        fa = np.where(a.any(-1), a.argmax(-1), -1)
        fb = np.where(b.any(-1), b.argmax(-1), -1)
        if (fa != fb).any():
            i, k = np.argwhere(fa != fb)[0]
            print(f"seed_lo {key}: pixel (x {tr.xs[i]}, y {tr.ys[i]}), draw {k}, uniform {u[i, k]!r}, "
                  f"CDF {cdf[i].tolist()}: view {fa[i, k]} with the epsilon, {fb[i, k]} without")
            return 0
    print("no key in range")
    return 1


if __name__ == "__main__":
    sys.exit(main())
