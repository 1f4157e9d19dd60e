// fk_dispatch.hpp -- what the C-ABI entry points of the shared-model banks have in common on the host (srkf_dispatch.cpp,
// info_dispatch.cpp, fls_dispatch.cpp): the refusals every family makes before it touches a pointer, the table of exact-shape
// kernels with its environment override, and the limit that 32-bit record offsets put on a bank.  Every message is part of
// the ABI's behaviour (tests/test_host_refusals.py pins them).
#pragma once

#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>

#include "../../include/filterhip.h"
#include "fk_device.hpp"

namespace fk {

inline int fail(int code, const char *msg)
{
    set_last_error(msg);
    return code;
}

// One fast kernel: exact (nx, nz), and for the fixed-lag smoother lags up to lmax (0 where the family has no third dimension).
template <class Args>
struct FastEntry {
    int nx, nz, lmax;
    int (*fn)(const Args &, int, hipStream_t);
};

// The table's entry for (n, m, lf), or nullptr: the general kernel.  A nonzero value of the environment variable `general`
// (FK_SRKF_GENERAL, ...) forces the general kernel (A/B and tests).  Nothing else enters the choice: chained calls run the
// kernel one call would.
template <class Args, size_t K>
const FastEntry<Args> *pick_fast(const FastEntry<Args> (&table)[K], const char *general, int n, int m, int lf = 0)
{
    const char *ev = getenv(general);
    if (ev && atoi(ev) != 0) return nullptr;
    for (const FastEntry<Args> &e : table)
        if (e.nx == n && e.nz == m && lf <= e.lmax) return &e;
    return nullptr;
}

// What a family takes of fk_kf_desc beyond the dimensions, and how its messages are spelled.
struct Family {
    const char *name;
    bool update_first;      // desc->update_first may be set (the predict / update filters; they take no flag)
    int32_t flags;          // otherwise: the FK_KF_FLAG_* bits the family accepts
    bool k0;                // the entry point takes a first step k0 >= 0 and names it next to N and T
};

// Everything about desc that does not need a pointer.  steps: the entry point reads desc->T (the single steps treat it as 1).
inline int check_desc(const fk_kf_desc *d, const Family &f, bool steps, int64_t k0 = 0)
{
    char msg[128];
    if (!d) return fail(FK_ERR_BAD_ARG, "desc is NULL");
    if (d->n < 1 || d->m < 1 || d->nu < 0) return fail(FK_ERR_BAD_ARG, "dim_x, dim_z must be >= 1, dim_u >= 0");
    if (d->N < 0 || (steps && d->T < 0) || k0 < 0)
        return fail(FK_ERR_BAD_ARG, f.k0 ? "N, T and k0 must be >= 0" : "N and T must be >= 0");
    if (d->layout != FK_LAYOUT_AOS && d->layout != FK_LAYOUT_SOA) return fail(FK_ERR_BAD_ARG, "bad layout");
    if (d->n > 16 || d->m > 8) return fail(FK_ERR_UNSUPPORTED, "dim_x/dim_z outside the compiled range (dim_x <= 16, dim_z <= 8)");
    if (d->model_mode != FK_MODEL_SHARED) {
        snprintf(msg, sizeof(msg), "%s: FK_MODEL_SHARED only", f.name);
        return fail(FK_ERR_UNSUPPORTED, msg);
    }
    if (f.update_first) {
        if (d->alpha_sq != 1.0 || d->flags != 0) {
            snprintf(msg, sizeof(msg), "%s: alpha_sq 1 and flags 0 only", f.name);
            return fail(FK_ERR_UNSUPPORTED, msg);
        }
        return FK_OK;
    }
    if (d->update_first != 0 || d->alpha_sq != 1.0) {
        snprintf(msg, sizeof(msg), "%s: update_first 0 and alpha_sq 1 only", f.name);
        return fail(FK_ERR_UNSUPPORTED, msg);
    }
    if (d->flags & ~f.flags) {
        snprintf(msg, sizeof(msg), "%s: flags 0 or FK_KF_FLAG_R_JOSEPH_DIAG only", f.name);
        return fail(FK_ERR_UNSUPPORTED, msg);
    }
    return FK_OK;
}

inline int check_control(const fk_kf_desc *d, const double *B, const double *u)
{
    if (d->nu > 0 && (!B || !u)) return fail(FK_ERR_BAD_ARG, "dim_u > 0 needs B and u");
    return FK_OK;
}

// One step's record block is addressed with 32-bit byte offsets (fk_device.hpp).  E: the family's widest record in doubles
// (the control record counts too).
inline int check_record_block(const fk_kf_desc *d, long E)
{
    if (d->nu > E) E = d->nu;
    if ((double)d->N * (double)E * 8.0 >= 4294967264.0) return fail(FK_ERR_UNSUPPORTED, "N * dim^2 * 8 bytes must stay below 4 GiB (split the bank)");
    return FK_OK;
}

// The launch of a predict / update filter (Args: N, n, m, nu): the fast kernel serves exact (n, m), the general kernel the
// rest; the widest record is n x n or an m x m by-product.
template <class Args, size_t K>
int launch_filter(const fk_kf_desc *d, Args &a, void *stream, const FastEntry<Args> (&table)[K], const char *general_env,
                  int (*general)(const Args &, int, hipStream_t))
{
    const long mx = d->n > d->m ? d->n : d->m;
    const int rc = check_record_block(d, mx * mx);
    if (rc != FK_OK) return rc;
    a.N = d->N;
    a.n = d->n; a.m = d->m; a.nu = d->nu;
    const FastEntry<Args> *e = pick_fast(table, general_env, d->n, d->m);
    return e ? e->fn(a, d->layout, (hipStream_t)stream) : general(a, d->layout, (hipStream_t)stream);
}

}  // namespace fk
