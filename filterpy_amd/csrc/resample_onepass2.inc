// resample_onepass2.inc -- round 6's form of the one-pass kernel (included by resample_onepass.hip, inside namespace fk).
//
// Same protocol, same hand-off words, same exact arithmetic as resample_onepass_kernel (the chunks of one call are resolved by
// a mix of the two code paths: op_chunk_slow and round 3's kernel both call op_resolve_chunk, ONE text in resample_onepass.hip)
// -- what changed is how many instructions and barriers the COMMON chunk costs.  Round 5's phase clocks: 20 k clocks per chunk at five workgroups per CU, the SIMDs 0.56
// busy issuing ~450 VALU instructions per wave and chunk, six workgroup barriers (two of them __syncthreads_or = three
// s_barriers each).  The common chunk -- its binade guessed right, no tie, not the first and not the last of its vector -- now
// takes:
//   * ONE fused pass over the weights where the binade is known before they land (PREDICTED: the running sum is extrapolated
//     from the inclusive prefix a chunk ~1.2 rounds back published; the word is requested together with the weights): chunk
//     sum, sign bits, increments and their in-thread prefix in 6 instructions per weight, one barrier;
//     otherwise round 3's order (sum -> barrier -> guess from k S -> increments -> barrier) on the same trimmed arithmetic;
//   * increments as  floor(fma(w, 2^-g, 1/2))  (one instruction less than ldexp + add; the same single rounding);
//   * slot boundaries as  cvt_i32(e1 - eps) == cvt_i32(e1 + eps)  with  e1 = fma(E_j, N ulp, K_thread) = N cs_j - u + 1:
//     6 instructions per weight instead of ~10 (truncation of a positive number is floor; both conversions agree exactly when
//     the estimate is farther than eps from an integer, and then n_j = floor(e) + 1 is the conversion itself); the exact tests
//     of fk_resample_math.hpp take the rest, per lane;
//   * no exchange of the neighbours' last boundary through LDS: a thread forms the boundary in front of its first weight
//     itself (the same exact value cs = (C0 + excl) ulp its neighbour's last weight ends on) -- one barrier less;
//   * plain s_barriers: the negative-weight verdict travels in the per-wave word that carries the partial sums.
// Everything the fast path does not take goes to op_chunk_slow, out of line.
//
// Error budget of the boundary estimate (slots; Np < 2^31): K0 = fma(C0, N ulp, 1 - u), K_thread = fma(excl, N ulp, K0),
// e1 = fma(E_j, N ulp, K_thread): three roundings of at most 2^-22 each, plus the 2^-21 of the two roundings inside pos_i
// (fk_resample_math.hpp) = 1.25 * 2^-20 < eps = 2^-18.

// op_chunk_slow is a real call.  Inlined, its ~90 registers and two loops share the allocation of the persistent loop: 212 spill
// instructions all over the fast path; as a call at the end of the iteration -- nothing of the fast path is live across it -- the
// fast path has none (the callee saves what it uses, when it runs).  The exact slot boundary (`decide` below) is inline: one to
// three pos_ge tests, no loop -- as calls in the middle of the fast path they cost it 26 registers and a spill.
#ifndef FK_OP2_SLOW_INLINED
#define FK_OP2_SLOW_INLINED 1      // 0: A/B build with op_chunk_slow as a real call (one copy per register budget)
#endif
#if FK_OP2_SLOW_INLINED
#define OP2_SLOW_INLINE __forceinline__
#else
#define OP2_SLOW_INLINE __attribute__((noinline))
#endif
// (BUDGET: the caller's WAVES -- one copy of the function per register budget: a callee shared by the 5- / 6- / 7-workgroup
//  kernels is compiled for the tightest of them, 72 registers and 150 spill instructions, and every slow chunk of every kernel
//  pays for it: 3.21 ms whatever FK_OP_WAVES said, against 3.05 with the slow path inlined at five)
template <bool STRATIFIED, int BUDGET>
__device__ OP2_SLOW_INLINE void op_chunk_slow(OpShared &sh, const double *a_w, const double *a_u, int32_t *a_idx, int32_t *a_status,
                                                        OpCtl *a_ctl, OpDesc *a_desc, int *a_bad, const double a_delta, const long a_Np,
                                                        const long a_nch, const int f, const int k, const double S_in, const int any_bad_in, const int lb_mode);
#define OP_SLOW_CALL(S_, bad_) op_chunk_slow<false, WAVES>(sh, a.w, a.u, a.idx, a.status, a.ctl, a.desc, a.bad, a.delta, a.Np, a.nch, f, k, S_, bad_, lb_mode)

// lookback_spec for ONE candidate binade (what the fast path publishes and looks for): the predecessors' increment sums at g
// down to the nearest published exact carry-out, which must lie in binade g and agree with its `raw` double.  which = 0: hit
// (returns the exact carry-in), -1: miss.  Wave 0 only.  Reads two words per predecessor (round 3's: three).
// wait_other: a predecessor nearer than the nearest carry-out that published at ANOTHER binade is waited for like one that has
// published nothing yet (and the launcher raises max_polls) -- it becomes a carry-out sooner or later (it lies across a crossing, or guessed wrong),
// and what this chunk would do after a miss (op_chunk_slow) is wait for exactly that carry, chunk by chunk.  With few long
// vectors the whole first wave of chunks sits behind the crossings of the binades below them: a miss there put every one of
// them on the chunk-by-chunk chain (profiles/r06/onepass: 2133 of the 3907 chunks of a 1 x 8e6 call).
__device__ double lookback_spec1(const OpDesc *d, int k, int g, double I0, int lane, int &which, const unsigned max_polls,
                                 const bool wait_other)
{
    which = -1;
    double acc = 0.0;
    const int g9 = g & 511;
    unsigned polls = 0;
    for (int j = k - 1; j >= 0; j -= 64) {
        const int jj = j - lane;
        u64 e1, e2, rw, term;
        for (;;) {
            e1 = jj >= 0 ? ld_agent(&d[jj].exact) : (u64)3;               // before the vector: a carry-out nobody can use
            rw = jj >= 0 ? ld_agent(&d[jj].raw) : (u64)0;
            term = __ballot((e1 & ST_MASK) >= 2);
            const u64 below = term ? (term & (0 - term)) - 1 : ~(u64)0;   // lanes nearer than the nearest carry-out
            const auto waiting = [&](const u64 w) { return (w & ST_MASK) == 0 || (wait_other && (w & ST_MASK) == 1 && exact_eu9(w) != g9); };
            if ((__ballot(waiting(e1)) & below) == 0) break;
            // (a predecessor on round 3's two-candidate path may have published at g in `exact2` only: look there before waiting)
            e2 = jj >= 0 ? ld_agent(&d[jj].exact2) : (u64)0;
            if (((e1 & ST_MASK) == 0 || ((e1 & ST_MASK) == 1 && exact_eu9(e1) != g9)) && (e2 & ST_MASK) == 1 && exact_eu9(e2) == g9) e1 = e2;
            if ((__ballot(waiting(e1)) & below) == 0) break;
            if (++polls > max_polls) return 0.0;                          // somebody is not speculating: do not wait here
            __builtin_amdgcn_s_sleep(FK_OP_SLEEP);
        }
        const int L = term ? __builtin_ctzll(term) : 64;
        const bool mine = lane < L;
        const bool at_g = (e1 & ST_MASK) == 1 && exact_eu9(e1) == g9;
        if (__ballot(mine && !at_g) != 0) return 0.0;
        acc += lane_bcast(wave_incl_sum(mine ? exact_C(e1) : 0.0), 63);   // integers: exact below 2^53 (checked at the end)
        if (!term) continue;
        const u64 tw = lane_bcast_u64(e1, L), tr = lane_bcast_u64(rw, L);
        if ((tw & ST_MASK) != 2 || j - L < 0) return 0.0;
        const double c = bits_to_double(tr);
        if (!(c > OP_SANE_LO && c < OP_SANE_HI)) return 0.0;
        const int ec = ulp_exp(c);
        const double Ct = scale2(c, -ec);
        if (Ct != exact_C(tw) || (ec & 511) != exact_eu9(tw)) return 0.0;
        if (ec == g && acc < 0x1p53 && Ct + acc + I0 < 0x1p53) {
            which = 0;
            return scale2(Ct + acc, g);
        }
        return 0.0;
    }
    return 0.0;
}

#ifndef FK_OP2_WAVES
#define FK_OP2_WAVES 5
#endif
#ifndef FK_OP2_PREDICT
#define FK_OP2_PREDICT 1       // 0: never predict the binade (A/B build)
#endif

// systematic only (the stratified boundaries read u[floor(e)] per weight: they stay on round 3's kernel)
//
// WAVES: workgroups per CU the register allocation aims at.  The fast path needs 70 VGPRs and the slow path is a call whose callee
// the compiler holds to the caller's budget (it spills inside, when it runs): 5 -> 96 registers, 6 -> 80, 7 -> 72, all without a
// spill in this kernel's own code; seven workgroups are 7 x 22.5 KB = 157 KB of the CU's 160 KB of LDS.
template <int WAVES>
__global__ void __launch_bounds__(OP_THREADS, WAVES)
resample_onepass2_kernel(const OpArgs a, const int pred_back, const int spec_polls, const int lb_mode)
{
    __shared__ OpShared sh;
    const long Np = a.Np, nch = a.nch;
    OP_CLOCK_START();
    int *win = sh.win();
    init_window(win, (int)threadIdx.x);
    const double Nd = (double)Np;
    double w8[OP_ITEMS];
    const long c = blockIdx.x;
    {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int f = (int)(c % a.Fn);
    const int k = (int)(c / a.Fn);
    OP_CLOCK(0);
    OP_STAMP(0);
    const double *wf = a.w + (long)f * Np;
    int32_t *of = a.idx + (long)f * Np;
    const double u_sys = a.u[f];
    OpDesc *d = a.desc + (long)f * nch;
    const long base = (long)k * OP_TILE;
    const int len = (int)((Np - base) < OP_TILE ? (Np - base) : OP_TILE);

    // ---- the prediction word and the weights are requested together ----
    // ONE wave reads the word (requested in front of its weights: the counter retires in order) and hands it to the others
    // through LDS: the word can change between two reads -- a chunk sum becomes an inclusive prefix, a chunk on op_chunk_slow
    // publishes again -- and four waves that read it themselves could disagree about the path they take through the barriers.
    const int kb = k - pred_back;
    const bool may_predict = FK_OP2_PREDICT && pred_back > 0 && kb >= 1 && len == OP_TILE && k < nch - 1;   // uniform
    u64 pword = 0;
    if (may_predict && wave == 0) pword = ld_agent(&d[kb].approx);
    {
        const double *src = wf + base + tid * OP_ITEMS;
        if (len == OP_TILE && (((uintptr_t)(wf + base)) & 15) == 0) {                          // uniform
            FK_UNROLL for (int q = 0; q < OP_ITEMS; q += 2) {
                const f64x2 t = *reinterpret_cast<const f64x2 *>(src + q);
                w8[q] = t.x;
                w8[q + 1] = t.y;
            }
        } else if (len == OP_TILE) {
            FK_UNROLL for (int q = 0; q < OP_ITEMS; ++q) w8[q] = src[q];
        } else {
            FK_UNROLL for (int q = 0; q < OP_ITEMS; ++q) {
                const int j = tid * OP_ITEMS + q;
                const double t = wf[base + (j < len ? j : 0)];
                w8[q] = j < len ? t : 0.0;
            }
        }
    }
    if (tid == 0) sh.bc_i[2] = 0;                                          // (the boundary check's verdict: see `decide` below)
    // the guess from the prediction word: the inclusive prefix after chunk kb, scaled to this chunk's range.  A guess only: a
    // wrong one is a miss like any other.  The extrapolation over pred_back chunks is good to a few parts in 10^4 of the
    // running sum once k is a few times pred_back; [lo, hi] gets 2^-8 of slack on either side and must lie inside ONE binade.
    int g = 0;
    bool predicted = false;
    if (may_predict) {                                                     // uniform
        if (wave == 0) {
            int gw = 0, pw = 0;
            if ((pword & ST_MASK) == 2) {
                const double Ab = unpack_approx(pword);
                const double r = Ab / (double)(kb + 1);                    // mean chunk sum so far
                const double lo = r * (double)k * (1.0 - 0x1p-8), hi = r * ((double)k + 1.0) * (1.0 + 0x1p-8);
                if (lo > OP_SANE_LO && hi < OP_SANE_HI && ulp_exp(lo) == ulp_exp(hi)) {
                    pw = 1;
                    gw = ulp_exp(lo);
                }
            }
            if (lane == 0) {
                sh.bc_i[0] = pw;
                sh.bc_i[1] = gw;
            }
        }
        __syncthreads();                                                                      // (0)
        predicted = sh.bc_i[0] != 0;
        g = sh.bc_i[1];
    }
    predicted = __builtin_amdgcn_readfirstlane((int)predicted) != 0;
    g = __builtin_amdgcn_readfirstlane(g);
    OP_COUNT(12, predicted ? 1 : 0);                                      // (tools/op_phase.py: chunks whose binade was predicted)
    double E[OP_ITEMS];
    double S = 0.0, excl = 0.0, I0 = 0.0;
    bool bad = false, valid = false;
    if (predicted) {
        // ---- ONE pass: chunk sum, sign bits, increments at g ----
        const double sg = scale2(1.0, -g);
        double s = 0.0, run = 0.0;
        int neg = 0;
        bool tie = false;
        FK_UNROLL for (int q = 0; q < OP_ITEMS; ++q) {
            s += w8[q];
            neg |= __double2hiint(w8[q]);
            const double x = __builtin_fma(w8[q], sg, 0.5);
            const double i = floor(x);
            tie = tie || (i == x);
            run += i;
            E[q] = run;
        }
        const double winc = wave_incl_sum(run);
        const double ws = lane_bcast(wave_incl_sum(s), 63);
        const int flags = (__ballot(neg < 0) != 0 ? 1 : 0) | (__ballot(tie) != 0 ? 2 : 0);
        if (lane == 63) sh.wsum[wave] = winc;
        if (lane == 0) {
            sh.seg.wtot[wave] = ws;
            sh.wmax[wave] = flags;
        }
        __syncthreads();                                                                      // (1)
        excl = winc - run;
        int fl = 0;
        FK_UNROLL for (int wv = 0; wv < OP_THREADS / 64; ++wv) {
            if (wv < wave) excl += sh.wsum[wv];
            I0 += sh.wsum[wv];
            fl |= sh.wmax[wv];
        }
        S = (sh.seg.wtot[0] + sh.seg.wtot[1]) + (sh.seg.wtot[2] + sh.seg.wtot[3]);
        bad = (fl & 1) || !(S < 0x1p1000);
        valid = !bad && !(fl & 2) && I0 < 0x1p52 && I0 > 0.0;
        OP_CLOCK(1);
    } else {
        // ---- round 3's order: the chunk sum first, the guess from k S ----
        double s = 0.0;
        int neg = 0;
        FK_UNROLL for (int q = 0; q < OP_ITEMS; ++q) {
            s += w8[q];
            neg |= __double2hiint(w8[q]);
        }
        const double ws = lane_bcast(wave_incl_sum(s), 63);
        const int fneg = __ballot(neg < 0) != 0 ? 1 : 0;
        if (lane == 0) {
            sh.seg.wtot[wave] = ws;
            sh.wmax[wave] = fneg;
        }
        __syncthreads();                                                                      // (A)
        S = (sh.seg.wtot[0] + sh.seg.wtot[1]) + (sh.seg.wtot[2] + sh.seg.wtot[3]);
        bad = ((sh.wmax[0] | sh.wmax[1] | sh.wmax[2] | sh.wmax[3]) & 1) || !(S < 0x1p1000);
        OP_CLOCK(1);
        bool guess = false;
        if (k > 0 && k < nch - 1 && !bad && S > 0.0 && len == OP_TILE) {   // uniform
            const double glo = (double)k * S * FK_OP_GUESS_LO, ghi = ((double)k + 1.0) * S * 1.04;
            // one candidate only: where the interval straddles a binade the chunk takes round 3's path (two candidates)
            guess = glo > OP_SANE_LO && ghi < OP_SANE_HI && ulp_exp(glo) == ulp_exp(ghi);
            g = ulp_exp(glo);
        }
        guess = __builtin_amdgcn_readfirstlane((int)guess) != 0;
        g = __builtin_amdgcn_readfirstlane(g);
        if (guess) {                                                       // uniform
            const double sg = scale2(1.0, -g);
            double run = 0.0;
            bool tie = false;
            FK_UNROLL for (int q = 0; q < OP_ITEMS; ++q) {
                const double x = __builtin_fma(w8[q], sg, 0.5);
                const double i = floor(x);
                tie = tie || (i == x);
                run += i;
                E[q] = run;
            }
            const double winc = wave_incl_sum(run);
            const int ftie = __ballot(tie) != 0 ? 2 : 0;
            if (lane == 63) sh.wsum[wave] = winc;                          // (other slots than barrier (A)'s: no second barrier
            if (lane == 0) sh.nlast[wave] = ftie;                          //  between that exchange and this one)
            __syncthreads();                                                                  // (S1)
            excl = winc - run;
            int fl = 0;
            FK_UNROLL for (int wv = 0; wv < OP_THREADS / 64; ++wv) {
                if (wv < wave) excl += sh.wsum[wv];
                I0 += sh.wsum[wv];
                fl |= sh.nlast[wv];
            }
            valid = !(fl & 2) && I0 < 0x1p52 && I0 > 0.0;
        }
    }
    valid = __builtin_amdgcn_readfirstlane((int)valid) != 0;
    OP_STAMP(1);
    OP_NOTE(12, (predicted ? 1 : 0) | (valid ? 2 : 0) | ((unsigned long long)(unsigned)g << 8));
    // (ONE call site for everything the fast path declines: the start or the end of a vector, a tie, a straddled binade, garbage,
    //  zeros -- `valid` is false --, a missed guess, the end of the positions)
    bool go_slow = !valid;
    double c_in = 0.0, ulp = 0.0, C0 = 0.0, Nu = 0.0, K0 = 0.0, e_hi = 0.0;
    if (valid) {                                                           // uniform
    // ---- publish the conditional increment sum, look back once ----
    // (rotating the looking-back wave over the SIMDs with the chunk number was measured: 3.200 / 3.201 ms, nothing)
    if (wave == 0) {
        if (lane == 0) {
            st_agent(&d[k].approx, pack_approx(S, 1));
            st_agent(&d[k].exact, pack_exact(1, g, I0));
        }
        int which = -1;
        const double cin0 = lookback_spec1(d, k, g, I0, lane, which, (unsigned)spec_polls, (lb_mode & 1) != 0);
        if (which == 0) {
            const double Cout = scale2(cin0, -g) + I0;                     // < 2^53: lookback_spec1 checked it
            const double c_out = scale2(Cout, g);
            if (lane == 0) {
                publish_carry(&d[k], c_out);
                st_agent(&d[k].approx, pack_approx(c_out, 2));             // the inclusive prefix (exact here): stage 1 and the predictions
            }
        }
        if (lane == 0) {
            sh.bc_d[1] = cin0;
            sh.bc_i[3] = which == 0 ? 1 : 0;
        }
    }
    __syncthreads();                                                                          // (2)
    const int verdict = __builtin_amdgcn_readfirstlane(sh.bc_i[3]);
    OP_CLOCK(2);
    OP_STAMP(3);
    OP_NOTE(13, verdict);
    c_in = sh.bc_d[1];
    // the chunk's first and last slot boundary, by every thread (uniform values: K0 and the whole increment sum) -- nothing more
    // for wave 0 to do while the others wait.  A chunk whose estimates come within four slots of Np goes to round 3's code
    // (its boundaries clamp at Np); its carry is published, nobody waits for it.
    ulp = scale2(1.0, g), C0 = scale2(c_in, -g), Nu = scale2(Nd, g);
    K0 = __builtin_fma(C0, Nu, 1.0 - u_sys);
    e_hi = __builtin_fma(I0, Nu, K0);
    go_slow = verdict != 1 || !(e_hi + 4.0 < Nd);                          // uniform: a miss, or the end of the positions
    }
    bool violated = false;
    if (!go_slow) {                                                        // uniform: the fast path
    // ---- slot boundaries: nb[q] = n(cs_j), np = the boundary in front of the thread's first weight, u_lo / u_hi the chunk's ----
    // An estimate within eps of an integer M leaves two candidates, M - 1 and M ... in slot numbers lo and lo + 1: n(c) =
    // min{ i : pos_i >= c } is lo if pos_lo >= c, else lo + 1 -- ONE exact comparison (pos_ge, fk_resample_math.hpp), no loop.
    // That the answer lies between them is the error analysis of the estimate (header of this file); it is CHECKED, not
    // trusted: pos_(lo-1) < c and, where pos_lo < c, pos_(lo+1) >= c -- a violation (never observed) sends the whole chunk
    // to op_chunk_slow before anything is stored.
    const double halfNd = 0.5 * Nd;
    int viol = 0;
    auto decide = [&](const double cs, const int lo) -> int {
        const bool t0 = pos_ge(u_sys + (double)lo, cs, Nd, halfNd);
        const bool below = lo == 0 || !pos_ge(u_sys + (double)(lo - 1), cs, Nd, halfNd);
        const bool above = t0 || pos_ge(u_sys + (double)(lo + 1), cs, Nd, halfNd);
        viol |= (below && above) ? 0 : 1;
        return t0 ? lo : lo + 1;
    };
    int u_lo = (int)(K0 - N_BOUNDARY_EPS), u_hi = (int)(e_hi - N_BOUNDARY_EPS);
    if (u_lo != (int)(K0 + N_BOUNDARY_EPS)) u_lo = decide(c_in, u_lo);                          // uniform, rare
    if (u_hi != (int)(e_hi + N_BOUNDARY_EPS)) u_hi = decide((C0 + I0) * ulp, u_hi);              // uniform, rare
    u_lo = __builtin_amdgcn_readfirstlane(u_lo);
    u_hi = __builtin_amdgcn_readfirstlane(u_hi);
    OP_COUNT(9, 1);
    int nb[OP_ITEMS], np;
    {
        const double Kt = __builtin_fma(excl, Nu, K0);
        unsigned unsure = 0;
        {
            const int lo = (int)(Kt - N_BOUNDARY_EPS), hi = (int)(Kt + N_BOUNDARY_EPS);
            unsure = lo != hi ? 1u << OP_ITEMS : 0u;
            np = lo;
        }
        FK_UNROLL for (int q = 0; q < OP_ITEMS; ++q) {
            const double e1 = __builtin_fma(E[q], Nu, Kt);
            const int lo = (int)(e1 - N_BOUNDARY_EPS), hi = (int)(e1 + N_BOUNDARY_EPS);
            unsure |= lo != hi ? 1u << q : 0u;
            nb[q] = lo;
        }
        if (unsure) {                                                      // about one lane in 10^4
            const double Cb = C0 + excl;                                   // exact
            if (unsure >> OP_ITEMS) np = decide(Cb * ulp, np);
            _Pragma("nounroll") for (int q = 0; q < OP_ITEMS; ++q) {
                if (!(unsure & (1u << q))) continue;
                double Eq = E[0];
                int lo = nb[0];
                FK_UNROLL for (int r = 1; r < OP_ITEMS; ++r) {
                    Eq = (q == r) ? E[r] : Eq;
                    lo = (q == r) ? nb[r] : lo;
                }
                const int n = decide((Cb + Eq) * ulp, lo);
                FK_UNROLL for (int r = 0; r < OP_ITEMS; ++r) nb[r] = (q == r) ? n : nb[r];
            }
        }
        if (tid == 0) np = u_lo;                                           // (what the chunk before ended on: the same exact value)
#ifdef FK_OP_CLOCKS
        FK_UNROLL for (int q = 0; q < OP_ITEMS; ++q) {
            if (g_dbg_cs) {
                g_dbg_cs[(long)f * Np + base + tid * OP_ITEMS + q] = (C0 + (excl + E[q])) * ulp;
                g_dbg_n[(long)f * Np + base + tid * OP_ITEMS + q] = nb[q];
            }
        }
#endif
    }
    if (viol) sh.bc_i[2] = 1;                                              // (read behind barrier (3); cleared by thread 0 at the top)
    OP_CLOCK(5);
    // ---- emission: heads into the window, inclusive max-scan, coalesced 16-byte stores ----
    const int mis = (int)(((uintptr_t)of >> 2) & 3);
    int seed = -1;
    const int jbase = (int)base + tid * OP_ITEMS;
    for (int wb = u_lo - ((mis + u_lo) & 3); u_hi > u_lo && wb < u_hi; wb += OP_WIN) {        // uniform
        {
            int p = np;
            FK_UNROLL for (int q = 0; q < OP_ITEMS; ++q) {
                const unsigned h = (unsigned)(p - wb);                     // a head below wb wraps to a huge number
                if (nb[q] > p && h < (unsigned)OP_WIN) win[h] = jbase + q;
                p = nb[q];
            }
        }
        __syncthreads();                                                                      // (3)
        violated = sh.bc_i[2] != 0;
        if (violated) break;                                               // uniform: a boundary outside its bracket (see `decide`)
        const int lim = u_hi - wb;                                         // slots [max(first, 0), lim) are ours
        const int first = u_lo - wb;
        int32_t *ow = of + wb;                                             // uniform; 16-byte aligned
        const int s0 = 12 * tid;
        int x[12];
        FK_UNROLL for (int gq = 0; gq < 3; ++gq) {
            const i32x4 t = *reinterpret_cast<const i32x4 *>(&win[s0 + 4 * gq]);
            x[4 * gq + 0] = t.x;
            x[4 * gq + 1] = t.y;
            x[4 * gq + 2] = t.z;
            x[4 * gq + 3] = t.w;
        }
        init_window(win, tid);                                             // (its own twelve slots: free for the next window / nobody else reads them)
        FK_UNROLL for (int e = 1; e < 12; ++e) x[e] = x[e] > x[e - 1] ? x[e] : x[e - 1];
        const int wincl = wave_incl_max(x[11]);
        if (lane == 63) sh.nlast[8 + wave] = wincl;      // (not wmax: a wave that runs ahead into the next chunk writes its flags there)
        __syncthreads();                                                                      // (4)
        const int up = __shfl_up(wincl, 1, 64);
        int pre = (lane == 0 || up < seed) ? seed : up;                   // everything before this thread, this wave
        FK_UNROLL for (int wv = 0; wv < OP_THREADS / 64; ++wv) {
            const int t = sh.nlast[8 + wv];
            if (wv < wave) pre = pre > t ? pre : t;
            seed = seed > t ? seed : t;                                    // every thread: running max after this window
        }
        FK_UNROLL for (int e = 0; e < 12; ++e) x[e] = x[e] > pre ? x[e] : pre;
        if (s0 < lim) {
            FK_UNROLL for (int gq = 0; gq < 3; ++gq) {
                const int sg4 = s0 + 4 * gq;
                if (sg4 >= first && sg4 + 3 < lim) *reinterpret_cast<i32x4 *>(&ow[sg4]) = i32x4{x[4 * gq], x[4 * gq + 1], x[4 * gq + 2], x[4 * gq + 3]};
                else {
                    FK_UNROLL for (int e = 0; e < 4; ++e)
                        if (sg4 + e >= first && sg4 + e < lim) ow[sg4 + e] = x[4 * gq + e];
                }
            }
        }
    }
    OP_CLOCK(7);
    OP_STAMP(4);
    }   // fast path
    if (go_slow || violated) {                                             // uniform: ONE call site for everything the fast path declines
        OP_COUNT(13, (go_slow && !valid) ? 1 : 0);                         // (tools/op_phase.py: why -- no valid guess, ...
        OP_COUNT(14, (go_slow && valid && sh.bc_i[3] != 1) ? 1 : 0);       //  ... the look-back missed, ...
        OP_COUNT(15, (go_slow && valid && sh.bc_i[3] == 1) ? 1 : 0);       //  ... the end of the positions)
        if (violated) __syncthreads();                                     // (a boundary outside its bracket: never observed)
        OP_SLOW_CALL(S, bad ? 1 : 0);
        OP_COUNT(8, 1);
    }
    OP_COUNT(11, 1);
    // (the last chunk of a vector never takes this path: op_chunk_slow fills the positions behind cumsum[-1])
    }
    OP_CLOCK_FLUSH();
}
