"""Regenerates tests/golden/enkf_bank.npz from the LIVE reference (filterpy.kalman.EnsembleKalmanFilter of the checkout named by
FILTERPY_REFERENCE): per bank, n_tracks reference filters built and stepped IN LOCKSTEP -- `for f in filters: f.predict()` --
under ONE numpy.random.seed, with the reference's multivariate_normal wrapped by a recorder.  That loop is what
EnsembleKalmanFilterBank replaces, and the order in which it consumes the global stream is the bank's draw-order contract.
Per op: which tracks drew, the draws, the (mean, cov) they were asked with, the op's arguments and every attribute of every
filter after the call.

    FILTERPY_REFERENCE=/path/to/filterpy python tests/golden/make_enkf_bank_golden.py

Two banks: 3 tracks at (4, 2) with N = 20 and one model for all; 3 tracks at (6, 3) with N = 70 and F, H, Q, R per track."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import enkf_port as ep  # noqa: E402

REF = os.environ["FILTERPY_REFERENCE"]
sys.path.insert(0, REF)
import filterpy.kalman.ensemble_kalman_filter as ref_mod  # noqa: E402
sys.path.remove(REF)

real_mvn = ref_mod.multivariate_normal
record = []


def recorder(mean, cov, size):
    d = real_mvn(mean, cov, size)
    record.append((np.array(mean, dtype=float), np.array(cov, dtype=float), int(size), d.copy()))
    return d


ref_mod.multivariate_normal = recorder

# the ops of enkf_port plus one: an update in which one track has no measurement (the loop calls its update(None))
UPDATE_MISSING = 6
OPS = [ep.INIT, ep.PREDICT, ep.UPDATE, UPDATE_MISSING, ep.PREDICT, ep.UPDATE_RMAT, ep.UPDATE_NONE]
ATTRS = ep.ATTRS


def random_model(n, m, rs, offset):
    A = rs.randn(n, n)
    return dict(F=np.eye(n) + 0.05 * rs.randn(n, n) / np.sqrt(n), H=rs.randn(m, n) / np.sqrt(n),
                x0=offset * (1.0 + rs.rand(n)) + rs.randn(n), P0=np.eye(n) * (1.0 + rs.rand()),
                Q=0.01 * (A @ A.T / n + np.eye(n)), R=(0.3 + rs.rand()) * np.eye(m))


def make_filter(md, N):
    F, H = md["F"], md["H"]
    f = ref_mod.EnsembleKalmanFilter(x=md["x0"].copy(), P=md["P0"].copy(), dim_z=H.shape[0], dt=1., N=N,
                                     hx=lambda s: np.dot(H, s), fx=lambda s, dt: np.dot(F, s))
    f.Q, f.R = md["Q"].copy(), md["R"].copy()
    return f


def run_bank(out, ci, mds, N, shared, seed, rs):
    B, n, m = len(mds), mds[0]["F"].shape[0], mds[0]["H"].shape[0]
    p = f"b{ci}_"
    for k in ("F", "H", "x0", "P0", "Q", "R"):
        out[p + k] = np.stack([md[k] for md in mds])
    out[p + "n"], out[p + "m"], out[p + "N"], out[p + "B"] = n, m, N, B
    out[p + "shared"], out[p + "seed"], out[p + "ops"] = shared, seed, np.array(OPS)
    np.random.seed(seed)
    filters = []
    for k, op in enumerate(OPS):
        q = f"{p}k{k}_"
        drew = np.zeros(B, dtype=bool)
        d = n if op in (ep.INIT, ep.PREDICT) else m
        draws, means, covs = np.zeros((B, N, d)), np.zeros((B, d)), np.zeros((B, d, d))
        z = np.stack([md["H"] @ (f.x if filters else md["x0"]) for md, f in zip(mds, filters or [None] * B)]) + rs.randn(B, m)
        has_z = np.ones(B, dtype=bool)
        Rarg = None
        if op == UPDATE_MISSING:
            has_z[1] = False
        elif op == ep.UPDATE_NONE:
            has_z[:] = False
        elif op == ep.UPDATE_RMAT:
            A = rs.randn(m, m)
            Rarg = out[q + "Rarg"] = 0.3 * (A @ A.T / m + np.eye(m))
        for b in range(B):
            record.clear()
            if op == ep.INIT:
                filters.append(make_filter(mds[b], N))
            elif op == ep.PREDICT:
                filters[b].predict()
            else:
                filters[b].update(z[b] if has_z[b] else None, Rarg)
            assert len(record) in (0, 1)
            if record:
                means[b], covs[b], size, draws[b] = record[0]
                assert size == N
                drew[b] = True
        assert np.array_equal(drew, has_z if op not in (ep.INIT, ep.PREDICT) else np.ones(B, dtype=bool))
        out[q + "drew"], out[q + "draw"], out[q + "mean"], out[q + "cov"] = drew, draws, means, covs
        if op not in (ep.INIT, ep.PREDICT):
            out[q + "z"], out[q + "has_z"] = z, has_z
        for a in ATTRS:
            out[q + a] = np.stack([np.array(getattr(f, a), dtype=float) for f in filters])
        out[q + "z_is_none"] = np.array([f.z.dtype == object for f in filters])


def main():
    out = {}
    rs = np.random.RandomState(20261020)
    one = random_model(4, 2, rs, 50.0)
    shared = [dict(one, x0=one["x0"] + 3.0 * b) for b in range(3)]
    run_bank(out, 0, shared, 20, True, 1234, rs)
    run_bank(out, 1, [random_model(6, 3, rs, 20.0 * b) for b in range(3)], 70, False, 4321, rs)
    out["n_cases"] = 2
    path = os.path.join(HERE, "enkf_bank.npz")
    np.savez_compressed(path, **out)
    print(f"{path}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
