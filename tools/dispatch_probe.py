"""What the Kalman filter and IMM dispatchers (csrc/kf_dispatch.cpp, csrc/imm_dispatch.cpp) do with a call, one line per call
on stdout -- to be run once per library (FK_LIB=<path to a libfilterhip.so>, default: the tree's) and the outputs compared.

  families   no device: every call carries fake pointers, passes the checks and ends in a launch that fails; the line is the
             return code and fk_last_error(), which names the kernel family.  Every (dim_x, dim_z), both layouts, the four
             model modes, the output sets, call shapes and flags, each routing switch unset and set; the IMM banks of 2..16.
             Refuses to run where a device is present (the calls would launch on the fake pointers).
  kernels    on a device, under `rocprofv3 --kernel-trace --stats -- python tools/dispatch_probe.py kernels`: one tiny valid
             call (N = 64, T = 2, real buffers) per class of each instantiation table; the trace's ordered kernel names show
             the instantiation chosen inside a family.  The line is the call and its return code.
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


def families():
    import torch
    if torch.cuda.is_available():
        sys.exit("dispatch_probe.py families: a device is present; the fake pointers would be launched on")
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


def kernels():
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
    {"families": families, "kernels": kernels}[sys.argv[1]]()
