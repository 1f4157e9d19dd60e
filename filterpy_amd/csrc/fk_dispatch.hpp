// fk_dispatch.hpp -- the host scaffold of every *_dispatch.cpp: what the C-ABI entry points have in common before a kernel
// is chosen.  For all of them: fail, the B / u rule, the limit that 32-bit record offsets put on a bank, and the convention by
// which a launcher hands a call on (NOT_SERVED) with the lookup over an instantiation table.  For the shared-model banks
// (srkf_dispatch.cpp, info_dispatch.cpp, fls_dispatch.cpp) also the descriptor refusals by family and the table of exact-shape
// kernels with its environment override; the Kalman filter with its variants, the IMM estimator and the unscented filter
// (kf_dispatch.cpp, imm_dispatch.cpp, ukf_dispatch.cpp) keep their own rules and messages and take fail, find_entry and the
// record-block guard.  Every message is part of the ABI's behaviour (tests/test_host_refusals.py pins them).
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

// A launcher answers FK_OK or an error once it has launched, and NOT_SERVED -- before it touches anything -- where the call is
// not one its kernels carry (a model mode, an output set, a by-product): the dispatcher then tries its next candidate.
constexpr int NOT_SERVED = 1;

// The entry of an instantiation table ({nx, nz, ..., fn}; a table over dim_x alone holds nz = 0) made for exactly (nx, nz), or
// nullptr.
template <class Entry, size_t K>
const Entry *find_entry(const Entry (&table)[K], int nx, int nz = 0)
{
    for (const Entry &e : table)
        if (e.nx == nx && e.nz == nz) return &e;
    return nullptr;
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

// One step's record block is addressed with 32-bit byte offsets (fk_device.hpp): `records` records of E doubles each must stay
// below `limit` bytes.  Limit and words are the caller's: the Kalman filter and IMM entry points spell theirs differently.
constexpr double FK_4GIB = 4294967296.0;
inline int check_record_block(double records, double E, double limit, const char *msg)
{
    if (records * E * 8.0 >= limit) return fail(FK_ERR_UNSUPPORTED, msg);
    return FK_OK;
}

// ... for the shared-model banks.  E: the family's widest record in doubles (the control record counts too).
inline int check_record_block(const fk_kf_desc *d, long E)
{
    if (d->nu > E) E = d->nu;
    return check_record_block((double)d->N, (double)E, FK_4GIB - 32.0, "N * dim^2 * 8 bytes must stay below 4 GiB (split the bank)");
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
