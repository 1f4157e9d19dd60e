"""What the Kalman filter, IMM and unscented-filter dispatchers (csrc/kf_dispatch.cpp, csrc/imm_dispatch.cpp,
csrc/ukf_dispatch.cpp) do with a call, one line per call on stdout -- to be run once per library (FK_LIB=<path to a
libfilterhip.so>, default: the tree's) and the outputs compared.  A second argument, kf or ukf, runs that half alone.

  families   no device: every call carries fake pointers, passes the checks and ends in a launch that fails; the line is the
             return code and fk_last_error(), which names the kernel family.  Every (dim_x, dim_z), both layouts, the four
             model modes, the output sets, call shapes and flags, each routing switch unset and set; the IMM banks of 2..16.
             The unscented filter's eleven entry points and the two Kalman filter variants (ukf): every (dim_x, dim_z), both
             layouts, with and without the pair-weight flag, k = 2n+1 and 2n, shared and per-track mode, with and without the
             optional outputs; their switches are read once per process, so every value gets an interpreter of its own.
             Refuses to run where a device is present (the calls would launch on the fake pointers).
  kernels    on a device, under `rocprofv3 --kernel-trace --stats -- python tools/dispatch_probe.py kernels`: one tiny valid
             call (N = 64, T = 2, real buffers) per class of each instantiation table; the trace's ordered kernel names show
             the instantiation chosen inside a family.  The line is the call and its return code.  ukf: P = I, Merwe weights
             (alpha 1, beta 2, kappa 0), at N = 64 and at N = 63 -- the odd count takes the smoother without the LDS-DMA fetch
             and the forward kernel without the paired stores --, every dim_x, for each of the eleven.
"""
import ctypes
import itertools
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from filterpy_amd import _abi                                                          # noqa: E402

if os.environ.get("FK_LIB"):      # another build of the library (A/B of two builds); tools only
    _abi.LIB_PATH = os.path.abspath(os.environ["FK_LIB"])

SWITCHES = (None, "FK_NO_FAST=1", "FK_NO_ML=1", "FK_NO_MLG=1", "FK_ML9=m", "FK_ML9=g", "FK_RTS_LANES=4", "FK_RTS_LANES=8",
            "FK_NO_FAST_EX=1", "FK_NO_MLG_EX=1")
ONE = 8                            # a non-NULL address that is never dereferenced


def kf_desc(n, m, N, T, layout=0, mode=0, nu=0, update_first=0, flags=0):
    return _abi.fk_kf_desc(n=n, m=m, nu=nu, model_mode=mode, N=N, T=T, layout=layout, update_first=update_first, alpha_sq=1.0,
                           flags=flags)


def call(lib, name, desc, args):
    rc = getattr(lib, name)(ctypes.byref(desc), *args)
    return "%d %s" % (rc, lib.fk_last_error().decode() if rc else "")


def batch_args(p, outs="all", mask=False, control=False, extras=None):
    """F Q H R B u z mask x P means covs means_p covs_p [extras] status stream; p: name -> address."""
    o = {"all": (1, 1, 1, 1), "none": (0, 0, 0, 0), "two": (1, 1, 0, 0)}[outs]
    a = [p["F"], p["Q"], p["H"], p["R"], p["B"] if control else None, p["u"] if control else None, p["z"],
         p["mask"] if mask else None, p["x"], p["P"]]
    a += [p[k] if on else None for k, on in zip(("means", "covs", "means_p", "covs_p"), o)]
    if extras is not None:
        a.append(ctypes.byref(extras) if extras else None)
    return a + [p["status"], None]


class Fake(dict):
    def __missing__(self, key):
        return ONE


UKF_SWITCHES = (None, "FK_UKF_MLG=0", "FK_UKF_MLG_MIN_NX=7", "FK_UKF_MLG_MIN_NX=8", "FK_UKF_MLG_MIN_NX=9", "FK_UKF_MLG_RTS_MIN_NX=8",
                "FK_UKF_MLG_RTS_MIN_NX=9", "FK_UKF_MLG_RTS_MIN_NX=10", "FK_UKF_PADDED=1", "FK_UKF_PAIRED=0", "FK_UT_COOP=0", "FK_UKF_DMA=0",
                "FK_STEADY_ROLLED=1", "FK_STEADY_AOS_WAVES=3", "FK_UKF_SOA_PAIRS=0", "FK_UKF_CHUNKS=2,2", "FK_UKF_RTS_CHUNKS=2,2",
                "FK_UKF_MLG_LANES=4", "FK_UKF_MLG_LANES=8", "FK_UKF_MLG_RTS_LANES=4", "FK_UKF_MLG_RTS_LANES=8", "FK_UKF_PERSIST=1")


def ukf_desc(n, m, N, T, layout=0, flags=0):
    return _abi.fk_ukf_desc(n=n, m=m, N=N, T=T, layout=layout, flags=flags, scale=float(n))


def plain(lib, name, args):
    rc = getattr(lib, name)(*args)
    return "%d %s" % (rc, lib.fk_last_error().decode() if rc else "")


def ukf_families(tag):
    """The calls of one interpreter (its switches are in the environment already)."""
    lib, N, T = _abi.lib(), 600, 5
    for n, layout in itertools.product(range(1, 17), (0, 1)):
        for flags, gains in itertools.product((0, 1), (ONE, None)):
            print(tag, "ukf rts %d layout %d flags %d gains %s" % (n, layout, flags, gains),
                  call(lib, "fk_ukf_linear_rts_f64", ukf_desc(n, 1, N, T, layout, flags), [ONE] * 8 + [gains, gains, None]))
        print(tag, "sigma %d layout %d" % (n, layout), plain(lib, "fk_ut_sigma_points_f64", [n, N, layout, 1.0, ONE, ONE, ONE, ONE, None]))
        for k, noise in itertools.product((2 * n + 1, 2 * n), (ONE, None)):
            print(tag, "transform %d k %d layout %d noise %s" % (n, k, layout, noise),
                  plain(lib, "fk_ut_transform_f64", [n, k, N, layout, ONE, ONE, ONE, noise, ONE, ONE, None]))
        for opt in (ONE, None):
            print(tag, "rts_correct %d layout %d optional %s" % (n, layout, opt),
                  plain(lib, "fk_ukf_rts_correct_f64", [n, N, layout, ONE, opt, ONE, ONE, ONE, ONE, ONE, opt, opt, None]))
        for m in range(1, 9):
            at = "(%d,%d) layout %d" % (n, m, layout)
            for flags in (0, 1):
                print(tag, "supported", at, flags, lib.fk_ukf_linear_supported(n, m, flags, 0), lib.fk_ukf_linear_supported(n, m, flags, 1))
                for outs in (ONE, None):
                    print(tag, "ukf batch", at, "flags %d outs %s" % (flags, outs),
                          call(lib, "fk_ukf_linear_batch_f64", ukf_desc(n, m, N, T, layout, flags), [ONE] * 7 + [outs, ONE, ONE, outs, outs, outs, None]))
            for k, opt in itertools.product((2 * n + 1, 2 * n), (ONE, None)):
                print(tag, "cross", at, "k %d x,z %s" % (k, opt),
                      plain(lib, "fk_ut_cross_variance_f64", [n, m, k, N, layout, opt, opt, ONE, ONE, ONE, ONE, None]))
                print(tag, "map", at, k, plain(lib, "fk_ut_linear_map_f64", [n, m, k, N, layout, ONE, ONE, ONE, None]),
                      plain(lib, "fk_ut_linear_map_f64", [m, n, k, N, layout, ONE, ONE, ONE, None]))
            for opt in (ONE, None):
                print(tag, "correct", at, "optional %s" % opt,
                      plain(lib, "fk_ukf_correct_f64", [n, m, N, layout, ONE, opt, ONE, ONE, ONE, ONE, opt, opt, None]))
            for mode, opt in itertools.product((0, 1), (ONE, None)):
                d = kf_desc(n, m, N, T, layout, mode, nu=2 if opt else 0)
                print(tag, "steady", at, "mode %d optional %s" % (mode, opt),
                      call(lib, "fk_kf_steadystate_f64", d, [ONE, ONE, ONE, opt, opt, ONE, opt, ONE, opt, opt, opt, None]),    # both halves
                      call(lib, "fk_kf_steadystate_f64", d, [ONE, None, None, opt, opt, None, None, ONE, None, opt, None, None]),   # predict
                      call(lib, "fk_kf_steadystate_f64", d, [None, ONE, ONE, None, None, ONE, opt, ONE, opt, None, opt, None]))     # update
                print(tag, "correlated", at, "mode %d optional %s" % (mode, opt),
                      call(lib, "fk_kf_update_correlated_f64", d, [ONE] * 4 + [opt, ONE, ONE] + [opt] * 5 + [None]))


def families(which=None):
    import subprocess
    import torch
    if torch.cuda.is_available():
        sys.exit("dispatch_probe.py families: a device is present; the fake pointers would be launched on")
    if which in (None, "kf"):
        kf_families()
    for switch in UKF_SWITCHES if which in (None, "ukf") else ():
        env = {k: v for k, v in os.environ.items() if k not in {s.split("=")[0] for s in UKF_SWITCHES[1:]}}
        env.update([switch.split("=")] if switch else [])
        sys.stdout.flush()
        subprocess.run([sys.executable, os.path.abspath(__file__), "ukf-one", str(switch)], env=env, check=True)


def kf_families():
    lib, p, N, T = _abi.lib(), Fake(), 300, 3
    ex = _abi.fk_kf_extras(*([ONE] * 6))
    for switch in SWITCHES:
        for v in SWITCHES[1:]:
            os.environ.pop(v.split("=")[0], None)
        if switch:
            os.environ.update([switch.split("=")])
        for n, m, layout, mode in itertools.product(range(1, 17), range(1, 9), (0, 1), (0, 1, 2, 3)):
            tag = "%s (%d,%d) layout %d mode %d" % (switch, n, m, layout, mode)
            for outs, (nu, uf) in itertools.product(("all", "none", "two"), ((0, 0), (2, 0), (0, 1))):
                d = kf_desc(n, m, N, T, layout, mode, nu, uf)
                print(tag, "batch", outs, nu, uf, call(lib, "fk_kf_batch_filter_f64", d, batch_args(p, outs, control=nu > 0)))
            d = kf_desc(n, m, N, T, layout, mode)
            print(tag, "batch mask", call(lib, "fk_kf_batch_filter_f64", d, batch_args(p, mask=True)))
            for mask in (False, True):
                print(tag, "ex", mask, call(lib, "fk_kf_batch_filter_ex_f64", d, batch_args(p, mask=mask, extras=ex)))
            # the flags: R's diagonal in the Joseph form, one interleaved covariance history, a caller-supplied inverse
            pi = Fake(covs=1 << 20, covs_p=(1 << 20) + 8 * (n * n if layout == 0 else n * n * N))
            print(tag, "rj_diag", call(lib, "fk_kf_batch_filter_f64", kf_desc(n, m, N, T, layout, mode, flags=1), batch_args(p)))
            print(tag, "interleaved", call(lib, "fk_kf_batch_filter_f64", kf_desc(n, m, N, T, layout, mode, flags=2), batch_args(pi)))
            for flags in (4, 8):
                print(tag, "update", flags, call(lib, "fk_kf_update_f64", kf_desc(n, m, N, T, layout, mode, flags=flags), [ONE] * 11 + [None]))
            for flags in (16, 32) if m == 1 else ():
                print(tag, "rts", flags, call(lib, "fk_kf_rts_f64", kf_desc(n, m, N, T, layout, mode, flags=flags), [ONE] * 8 + [0, ONE, None]))
            print(tag, "predict", call(lib, "fk_kf_predict_f64", d, [ONE, ONE, None, None, ONE, ONE, ONE, None]))
            print(tag, "update", call(lib, "fk_kf_update_f64", d, [ONE] * 4 + [ONE] * 7 + [None]))
            if m <= 2:                      # the smoother does not read dim_z
                for gains in (ONE, None):
                    print(tag, "rts", gains, call(lib, "fk_kf_rts_f64", d, [ONE] * 6 + [gains, gains, m - 1, ONE, None]))
        for (n, m), models, layout in itertools.product(((2, 1), (4, 2), (5, 3), (6, 3), (7, 3), (6, 4), (9, 4), (10, 4), (9, 5), (12, 4),
                                                         (13, 4), (16, 8)), range(2, 17), (0, 1)):
            for phase, mmae, extended in ((0, 0, False), (0, 0, True), (0, 1, False), (1, 0, False), (2, 0, False)):
                d = _abi.fk_imm_desc(n=n, m=m, n_models=models, layout=layout, N=N, T=T, phase=phase, flags=mmae)
                outs = [ONE] * 3 + [None if mmae else ONE] * 2 + [ONE]
                tag = "%s imm (%d,%d) x %d layout %d phase %d mmae %d" % (switch, n, m, models, layout, phase, mmae)
                if not extended:
                    print(tag, "plain", call(lib, "fk_imm_batch_f64", d, [ONE] * 9 + outs + [ONE, None]))
                more = [ONE, ONE, 2, ONE, ONE] if extended else [None, None, 0, None, None]
                print(tag, "ex", extended, call(lib, "fk_imm_batch_ex_f64", d, [ONE] * 6 + more + [ONE] * 3 + outs + [ONE, None]))


def merwe(n):
    """alpha 1, beta 2, kappa 0: lambda = 0, so Wm[0] = 0, Wc[0] = 2, every other weight 1 / 2n; scale = n + lambda."""
    w = [1.0 / (2 * n)] * (2 * n + 1)
    return [0.0] + w[1:], [2.0] + w[1:]


def ukf_kernels():
    import torch
    dev = torch.device("cuda:0")
    lib, T = _abi.lib(), 2
    big = 1 << 16             # doubles per buffer; the widest array of a call, 64 x 33 x 16 sigma points, is 33792
    buf = {k: torch.zeros(big, dtype=torch.float64, device=dev) for k in
           ("F", "Q", "H", "R", "Wm", "Wc", "z", "x", "P", "means", "covs", "Xs", "Ps", "xs", "ps", "Kg", "sig", "sh", "xo", "Po", "Pxz", "zp",
            "S", "K", "y", "SI", "M", "Pb", "xb", "B", "u", "means_p")}
    buf["mask"] = torch.ones(big, dtype=torch.uint8, device=dev)
    buf["status"] = torch.zeros(big, dtype=torch.int32, device=dev)
    p = {k: v.data_ptr() for k, v in buf.items()}

    def records(name, mat, count, layout, steps=1):
        r = mat.double().expand(count, *mat.shape).reshape(count, -1)
        r = (r if layout == 0 else r.t()).contiguous().reshape(-1).repeat(steps)
        buf[name][:r.numel()] = r.to(dev)

    def report(what, line):
        torch.cuda.synchronize()
        print(what, line, flush=True)

    for layout, N, n in itertools.product((0, 1), (64, 63), range(1, 17)):
        m = min(n, 2)
        at = "%d layout %d N %d" % (n, layout, N)
        for name, mat in (("F", torch.eye(n)), ("Q", 0.1 * torch.eye(n)), ("H", torch.eye(m, n)), ("R", torch.eye(m)), ("M", torch.eye(m, n))):
            buf[name][:mat.numel()] = mat.double().reshape(-1).to(dev)
        for name, w in zip(("Wm", "Wc"), merwe(n)):
            buf[name][:2 * n + 1] = torch.tensor(w, dtype=torch.float64)
        eye = {"x": (torch.zeros(n), 1), "P": (torch.eye(n), 1), "Xs": (torch.zeros(n), T), "Ps": (torch.eye(n), T), "Pb": (torch.eye(n), 1),
               "S": (torch.eye(m), 1), "K": (torch.zeros(n, m), 1)}
        for name, (mat, steps) in eye.items():
            records(name, mat, N, layout, steps)
        # the forward call also at the classes' own shapes (the exact instantiations) and on eight lanes (dim_x >= 13, dim_z >= 5)
        for mz, flags in itertools.product(sorted({m} | {z for x, z in ((6, 3), (8, 4), (9, 3), (9, 4), (13, 5), (16, 8)) if x == n}), (0, 1)):
            if lib.fk_ukf_linear_supported(n, mz, flags, 0):
                buf["H"][:mz * n] = torch.eye(mz, n, dtype=torch.float64).reshape(-1).to(dev)
                buf["R"][:mz * mz] = torch.eye(mz, dtype=torch.float64).reshape(-1).to(dev)
                records("x", torch.zeros(n), N, layout)
                records("P", torch.eye(n), N, layout)
                report("ukf batch (%d,%d) layout %d N %d flags %d" % (n, mz, layout, N, flags),
                       call(lib, "fk_ukf_linear_batch_f64", ukf_desc(n, mz, N, T, layout, flags),
                            [p[k] for k in ("F", "H", "Q", "R", "Wm", "Wc", "z", "mask", "x", "P", "means", "covs", "status")] + [None]))
        buf["H"][:m * n] = torch.eye(m, n, dtype=torch.float64).reshape(-1).to(dev)
        buf["R"][:m * m] = torch.eye(m, dtype=torch.float64).reshape(-1).to(dev)
        for flags in (0, 1):
            if lib.fk_ukf_linear_supported(n, m, flags, 1):
                report("ukf rts %s flags %d" % (at, flags),
                       call(lib, "fk_ukf_linear_rts_f64", ukf_desc(n, m, N, T, layout, flags),
                            [p[k] for k in ("F", "Q", "Wm", "Wc", "Xs", "Ps", "xs", "ps", "Kg", "status")] + [None]))
        records("P", torch.eye(n), N, layout)
        report("sigma " + at, plain(lib, "fk_ut_sigma_points_f64", [n, N, layout, float(n), p["x"], p["P"], p["sig"], p["status"], None]))
        for k in (2 * n + 1, 2 * n):
            report("transform %s k %d" % (at, k),
                   plain(lib, "fk_ut_transform_f64", [n, k, N, layout, p["sig"], p["Wm"], p["Wc"], p["Q"], p["xo"], p["Po"], None]))
        report("map " + at, plain(lib, "fk_ut_linear_map_f64", [n, m, 2 * n + 1, N, layout, p["H"], p["sig"], p["sh"], None]))
        report("cross " + at, plain(lib, "fk_ut_cross_variance_f64", [n, m, 2 * n + 1, N, layout, p["xo"], p["zp"], p["sig"], p["sh"], p["Wc"], p["Pxz"], None]))
        report("correct " + at, plain(lib, "fk_ukf_correct_f64", [n, m, N, layout, p["Pxz"], p["zp"], p["S"], p["z"], p["x"], p["P"], p["Kg"], p["status"], None]))
        report("rts_correct " + at, plain(lib, "fk_ukf_rts_correct_f64", [n, N, layout, p["Po"], p["xb"], p["Pb"], p["xo"], p["Pb"], p["x"], p["P"], p["Kg"],
                                                                          p["status"], None]))
        for mm, mode in itertools.product(sorted({m, min(n, 8)} | {z for x, z in ((2, 1), (6, 3), (9, 3), (9, 4), (10, 4), (9, 5), (16, 8)) if x == n}), (0, 1)):
            d = kf_desc(n, mm, N, T, layout, mode)
            records("K", torch.zeros(n, mm), N if mode else 1, layout if mode else 0)
            buf["H"][:mm * n] = torch.eye(mm, n, dtype=torch.float64).reshape(-1).to(dev)
            buf["R"][:mm * mm] = torch.eye(mm, dtype=torch.float64).reshape(-1).to(dev)
            report("steady (%d,%d) layout %d N %d mode %d" % (n, mm, layout, N, mode),
                   call(lib, "fk_kf_steadystate_f64", d, [p[k] for k in ("F", "H", "K", "B", "u", "z", "mask", "x", "means", "means_p", "y")] + [None]))
            records("P", torch.eye(n), N, layout)
            report("correlated (%d,%d) layout %d N %d mode %d" % (n, mm, layout, N, mode),
                   call(lib, "fk_kf_update_correlated_f64", d, [p[k] for k in ("H", "R", "K", "z", "mask", "x", "P", "y", "Kg", "S", "SI", "status")] + [None]))
        buf["H"][:m * n] = torch.eye(m, n, dtype=torch.float64).reshape(-1).to(dev)


def kernels(which=None):
    if which in (None, "kf"):
        kf_kernels()
    if which in (None, "ukf"):
        ukf_kernels()


def kf_kernels():
    import torch
    dev = torch.device("cuda:0")
    lib, N, T = _abi.lib(), 64, 2
    big = 1 << 20             # doubles per buffer; the widest array of a call, N x 16 filters x 16 x 16, is 2^18
    buf = {k: torch.zeros(big, dtype=torch.float64, device=dev) for k in
           ("F", "Q", "H", "R", "B", "u", "z", "x", "P", "means", "covs", "means_p", "covs_p", "y", "K", "S", "SI", "ll", "maha",
            "Xs", "Ps", "xs", "Ps_out", "Kg", "Pp", "M", "mu", "x_out", "P_out", "mu_out", "xp_out", "Pp_out", "L", "ll0")}
    buf["mask"] = torch.ones(big, dtype=torch.uint8, device=dev)
    buf["status"] = torch.zeros(big, dtype=torch.int32, device=dev)
    p = {k: v.data_ptr() for k, v in buf.items()}
    ex = _abi.fk_kf_extras(p["y"], p["K"], p["S"], p["SI"], p["ll"], p["maha"])

    def records(name, mat, count, layout):
        """`count` copies of mat as a record array in the layout."""
        r = mat.to(dev).double().expand(count, *mat.shape)
        r = r.reshape(count, -1) if layout == 0 else r.reshape(count, -1).t()
        buf[name][:r.numel()] = r.contiguous().reshape(-1)

    def model(n, m, copies=1):
        buf["F"][:copies * n * n] = torch.eye(n).repeat(copies, 1, 1).reshape(-1)
        buf["Q"][:copies * n * n] = 0.1 * torch.eye(n).repeat(copies, 1, 1).reshape(-1)
        buf["H"][:copies * m * n] = torch.eye(m, n).repeat(copies, 1, 1).reshape(-1)
        buf["R"][:copies * m * m] = torch.eye(m).repeat(copies, 1, 1).reshape(-1)

    def report(what, line):
        torch.cuda.synchronize()
        print(what, line, flush=True)

    stream = None
    for layout in (0, 1):
        # every (dim_x, dim_z): the kf_fast, kf_ml, kf_mlg shapes and the general kernel's classes; plain and with histories
        for n, m in itertools.product(range(1, 17), range(1, 9)):
            model(n, m)
            for extras in (None, ex):
                records("x", torch.zeros(n), N, layout)
                records("P", torch.eye(n), N, layout)
                name = "fk_kf_batch_filter_ex_f64" if extras else "fk_kf_batch_filter_f64"
                report("batch (%d,%d) layout %d extras %d" % (n, m, layout, extras is not None),
                       call(lib, name, kf_desc(n, m, N, T, layout), batch_args(p, extras=extras)))
        # every dim_x of the smoothers
        for n in range(1, 17):
            model(n, 1)
            buf["Ps"].zero_()                                                  # (Xs: zeros)
            for t in range(T):
                r = torch.eye(n).expand(N, n, n).reshape(N, -1)
                r = r if layout == 0 else r.t()
                buf["Ps"][t * N * n * n:(t + 1) * N * n * n] = r.contiguous().reshape(-1).to(dev)
            args = [p["F"], p["Q"], p["Xs"], p["Ps"], p["xs"], p["Ps_out"], p["Kg"], p["Pp"], 0, p["status"], stream]
            report("rts %d layout %d" % (n, layout), call(lib, "fk_kf_rts_f64", kf_desc(n, 1, N, T, layout), args))
        # IMM: every class x bank-size step x plain / extended, and the small banks' compiled output sets
        for (n, m), models, extended in itertools.product(((2, 1), (4, 2), (6, 3), (9, 4), (12, 4), (16, 8)), (2, 3, 4, 8, 16), (False, True)):
            model(n, m, models)
            buf["M"][:models * models] = torch.full((models, models), 1.0 / models).reshape(-1)
            buf["mu"][:N * models] = 1.0 / models
            buf["xs"].zero_()
            records("Ps", torch.eye(n), N * models, layout)
            d = _abi.fk_imm_desc(n=n, m=m, n_models=models, layout=layout, N=N, T=T, phase=0, flags=0)
            for outs in ((1, 1, 1, 1, 1, 1), (1, 1, 1, 0, 0, 0), (0, 0, 0, 0, 0, 0)):
                o = [p[k] if on else None for k, on in zip(("x_out", "P_out", "mu_out", "xp_out", "Pp_out", "L"), outs)]
                more = [p["mask"], p["ll0"], 2, p["B"], p["u"]] if extended else [None, None, 0, None, None]
                args = [p["F"], p["Q"], p["H"], p["R"], p["M"], p["z"]] + more + [p["xs"], p["Ps"], p["mu"]] + o + [p["status"], stream]
                report("imm (%d,%d) x %d layout %d extended %d outs %s" % (n, m, models, layout, extended, outs),
                       call(lib, "fk_imm_batch_ex_f64", d, args))


if __name__ == "__main__":
    {"families": families, "kernels": kernels, "ukf-one": ukf_families}[sys.argv[1]](*sys.argv[2:3])
