"""
The reference's fp32 digamma helper (`const DIGAMMA_c`, src/utils.jl:21-53, compiled by oracle/_ref/Makefile) at a fixed set of
points, recorded in tests/golden/ref_digamma_f32.npz, so that the tests that pin the oracle's and the device's digamma to it run
where neither the reference tree nor oracle/_ref/libref_digamma.so is present.  Where the library is present, the tests use it and
check it against the recording as well.

    python tests/ref_digamma_golden.py        # rewrites the fixture from oracle/_ref/libref_digamma.so
"""
import hashlib
import os
import sys

import numpy as np

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_digamma_f32.npz")


def points():
    """every float32 argument the tests evaluate the helper at (the 100 000 draws of test_oracle_special are the first of these 200 000)"""
    rng = np.random.default_rng(0)
    return np.concatenate([np.exp(rng.uniform(np.log(1e-3), np.log(1e6), 200000)), np.linspace(1.40, 1.52, 5000), np.linspace(1.40, 1.52, 2000),
                           [1e-3, 1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 6.9999995, 7.0, 8.0, 100.0, 1e6]]).astype(np.float32)


def _digest(x):
    return hashlib.sha256(np.ascontiguousarray(x, dtype=np.float32).tobytes()).hexdigest()


def recorded(x):
    """the recorded helper values at the float32 points x, each of which must be one of points()"""
    g = np.load(GOLD)
    xs = points()
    assert _digest(xs) == str(g["points_sha256"]), "points() no longer generates the recorded arguments"
    order = np.argsort(xs, kind="stable")
    sx, sp = xs[order], g["psi"][order]
    x = np.asarray(x, dtype=np.float32)
    i = np.minimum(np.searchsorted(sx, x), sx.size - 1)
    assert np.array_equal(sx[i], x), "an argument the fixture does not record"
    return sp[i]


def ref_digamma_f32(oracle, x):
    """the helper at x: the compiled library when there is one (checked bit for bit against the recording), else the recording"""
    rec = recorded(x)
    if oracle.build_ref() is not None:
        live = oracle.ref_digamma_f32(x)
        assert np.array_equal(live, rec), "oracle/_ref/libref_digamma.so disagrees with tests/golden/ref_digamma_f32.npz"
        return live
    return rec


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from oracle import oracle as oc
    if oc.build_ref() is None:
        raise SystemExit("needs oracle/_ref/libref_digamma.so (oracle/_ref/Makefile)")
    xs = points()
    np.savez_compressed(GOLD, psi=oc.ref_digamma_f32(xs).astype(np.float32), points_sha256=np.array(_digest(xs)))
    print(f"wrote {GOLD}: {xs.size} points, {os.path.getsize(GOLD)} bytes")
