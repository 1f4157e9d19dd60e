"""Regenerates tests/golden/enkf.npz from the LIVE reference (filterpy.kalman.EnsembleKalmanFilter of the checkout named by
FILTERPY_REFERENCE), with the reference's multivariate_normal wrapped by a recorder: per case and per call the recorded draw,
the (mean, cov) it was asked with (size is the case's N), the call's own arguments and every attribute after the call.

    FILTERPY_REFERENCE=/path/to/filterpy python tests/golden/make_enkf_golden.py [--spread-only]

It also prints the spread table behind the 1e-10 bar of the EnKF tests (docs/MEASUREMENTS.md, "EnKF"): the worst error over
x, P, K, S and the ensemble after 20 steps of tests/enkf_port.py in its three forms of the second moments, against the live
reference replaying the same draws."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import enkf_port as ep  # noqa: E402

REF = os.environ.get("FILTERPY_REFERENCE", "/root/reference")
sys.path.insert(0, REF)
import filterpy.kalman.ensemble_kalman_filter as ref_mod  # noqa: E402
from filterpy.common import Q_discrete_white_noise  # noqa: E402
sys.path.remove(REF)

real_mvn = ref_mod.multivariate_normal
record = []


def recorder(mean, cov, size):
    d = real_mvn(mean, cov, size)
    record.append((np.array(mean, dtype=float), np.array(cov, dtype=float), int(size), d.copy()))
    return d


ref_mod.multivariate_normal = recorder


def rel_err(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b))) / max(1.0, float(np.max(np.abs(b)))))


def random_model(n, m, rs, offset=0.0):
    A = rs.randn(n, n)
    F = np.eye(n) + 0.05 * rs.randn(n, n) / np.sqrt(n)
    H = rs.randn(m, n) / np.sqrt(n)
    x0 = offset * (1.0 + rs.rand(n)) * np.where(rs.rand(n) < 0.5, -1.0, 1.0) + rs.randn(n)
    return dict(F=F, H=H, x0=x0, P0=np.eye(n), Q=0.01 * (A @ A.T / n + np.eye(n)), R=0.5 * np.eye(m))


def reference_models():
    """the two models of the reference's test_enkf.py (singular Q_discrete_white_noise blocks included)"""
    F2, H2 = np.array([[1., 1.], [0., 1.]]), np.array([[1., 0.]])
    one = dict(F=F2, H=H2, x0=np.array([0., 1.]), P0=np.eye(2) * 100., Q=Q_discrete_white_noise(2, 1., .001), R=np.eye(1) * 100.)
    F6 = np.array([[1., 1., .5, 0., 0., 0.], [0., 1., 1., 0., 0., 0.], [0., 0., 1., 0., 0., 0.],
                   [0., 0., 0., 1., 1., .5], [0., 0., 0., 0., 1., 1.], [0., 0., 0., 0., 0., 1.]])
    H6 = np.zeros((2, 6))
    H6[0, 0] = H6[1, 3] = 1.0
    Q6 = np.eye(6)
    Q6[0:3, 0:3] = Q6[3:6, 3:6] = Q_discrete_white_noise(3, 1., .001)
    two = dict(F=F6, H=H6, x0=np.array([50., 0., 0., 0., 0., 0.]), P0=np.eye(6) * 100., Q=Q6, R=np.eye(2) * 0.01)
    return one, two


def make_filter(md, N):
    F, H = md["F"], md["H"]
    f = ref_mod.EnsembleKalmanFilter(x=md["x0"].copy(), P=md["P0"].copy(), dim_z=H.shape[0], dt=1., N=N,
                                     hx=lambda s: np.dot(H, s), fx=lambda s, dt: np.dot(F, s))
    f.Q, f.R = md["Q"].copy(), md["R"].copy()
    return f


# after the constructor's initialize: every op, a matrix and a scalar R, two updates in a row, a second initialize
OPS = [ep.PREDICT, ep.UPDATE, ep.PREDICT, ep.UPDATE_RMAT, ep.UPDATE_RSCALAR, ep.UPDATE_NONE, ep.INIT, ep.PREDICT, ep.UPDATE]


def run_case(out, ci, md, N, rs):
    n, m = md["F"].shape[0], md["H"].shape[0]
    p = f"c{ci}_"
    for k in ("F", "H", "x0", "P0", "Q", "R"):
        out[p + k] = md[k]
    out[p + "n"], out[p + "m"], out[p + "N"] = n, m, N
    record.clear()
    f = make_filter(md, N)
    ops = [ep.INIT] + OPS
    out[p + "ops"] = np.array(ops)
    for k, op in enumerate(ops):
        q = f"{p}k{k}_"
        if k > 0:
            record.clear()
            z = md["H"] @ f.x + rs.randn(m)
            if op == ep.INIT:
                f.initialize(md["x0"] + 0.5, md["P0"] * 2.0)
            elif op == ep.PREDICT:
                f.predict()
            elif op == ep.UPDATE_NONE:
                f.update(None)
            else:
                Rarg = None
                if op == ep.UPDATE_RMAT:
                    B = rs.randn(m, m)
                    Rarg = out[q + "Rarg"] = 0.3 * (B @ B.T / m + np.eye(m))
                elif op == ep.UPDATE_RSCALAR:
                    Rarg = 0.7
                    out[q + "Rarg"] = np.array(0.7)
                out[q + "z"] = z
                f.update(z, Rarg)
        assert len(record) == (0 if op == ep.UPDATE_NONE else 1), (ci, k, len(record))
        if record:
            mean, cov, size, d = record[0]
            assert size == N
            out[q + "draw"], out[q + "mean"], out[q + "cov"] = d, mean, cov
        for a in ep.ATTRS:
            out[q + a] = np.array(getattr(f, a), dtype=float)
        out[q + "z_is_none"] = np.array(f.z.dtype == object)


def spread():
    """the worst error of the port's three forms against the live reference, 20 steps, 8 seeds per setting"""
    print("offset  (n, m, N)        two-pass    shifted     uncentred")
    for offset in (0.0, 1e3, 1e4):
        for n, m, N in ((4, 2, 200), (2, 1, 8), (6, 3, 1025), (9, 4, 70)):
            worst = dict(twopass=0.0, shifted=0.0, uncentred=0.0)
            for seed in range(8):
                rs = np.random.RandomState(1000 + seed)
                md = random_model(n, m, rs, offset)
                np.random.seed(seed)
                record.clear()
                f = make_filter(md, N)
                draws, zs, refs = [record[0][3]], [], []
                for _ in range(20):
                    f.predict()
                    z = md["H"] @ f.x + rs.randn(m)
                    f.update(z)
                    zs.append(z)
                    refs.append([np.array(getattr(f, a), dtype=float) for a in ("x", "P", "K", "S", "sigmas")])
                draws += [r[3] for r in record[1:]]
                for mode in worst:
                    sig, x, P = draws[0].copy(), md["x0"].copy(), md["P0"].copy()
                    for t in range(20):
                        # the two-pass form with its summation reversed: the reference's own rounding scatter
                        e1, e2 = draws[1 + 2 * t], draws[2 + 2 * t]
                        if mode == "twopass":
                            sig, x, P = ep.predict(sig[::-1], e1[::-1], md["F"])
                            sig, x, P, K, S, SI = ep.update(sig, x, P, zs[t], md["R"], e2[::-1], md["H"])
                            sig = sig[::-1]
                        else:
                            sig, x, P = ep.predict(sig, e1, md["F"], mode, md["F"] @ x)
                            sig, x, P, K, S, SI = ep.update(sig, x, P, zs[t], md["R"], e2, md["H"], mode=mode)
                        for mine, want in zip((x, P, K, S, sig), refs[t]):
                            worst[mode] = max(worst[mode], rel_err(mine, want))
            print(f"{offset:<7g} ({n}, {m}, {N:<5d})  {worst['twopass']:10.1e}  {worst['shifted']:10.1e}  {worst['uncentred']:10.1e}")


def main():
    if "--spread-only" not in sys.argv:
        out = {}
        rs = np.random.RandomState(20261017)
        np.random.seed(424242)
        one, two = reference_models()
        cases = [(one, 8), (two, 30), (random_model(4, 2, rs, 1e3), 200), (random_model(3, 3, rs), 2), (random_model(1, 1, rs), 5),
                 (random_model(9, 4, rs), 70), (random_model(16, 8, rs), 40)]
        for ci, (md, N) in enumerate(cases):
            run_case(out, ci, md, N, rs)
        out["n_cases"] = len(cases)
        path = os.path.join(HERE, "enkf.npz")
        np.savez_compressed(path, **out)
        print(f"{path}: {os.path.getsize(path)} bytes, {len(cases)} cases")
    spread()


if __name__ == "__main__":
    main()
