// kf_ml_predict.inc -- the predict half of one kf_ml_kernel step (included by kf_ml.hip at the two places a step can
// run it: before the update half, or -- update_first -- after it; only one of them exists in any instantiation).
// Plain text inclusion on purpose: a lambda or an unrolled two-trip loop around the halves changed the code hipcc
// generates for the tuned plain-call kernels (a lambda: +850 instructions, arrays through scratch).
        // ---------------------------------------------------------------- predict --
        // Row i of F serves x' [i] = F[i][:] x AND column i of T = P F' in the same pass, and it is requested from LDS one
        // iteration ahead (two row buffers): a stage's ds_reads and the s_waitcnt right behind them exposed the whole LDS
        // latency once per row -- ~60 times per step, which is what kept the VALU at 0.5-0.65 busy with two waves per SIMD
        // (round 4; same operations in the same order, bit-identical results).
        {
            // The posterior covariance of step t-1 is still in P: its 27 stores are spread over the nine
            // iterations below (and the prior's over the PHT stage), so that a wave's store traffic is
            // issued evenly through its arithmetic instead of in two bursts per step that every wave of
            // the chip fires at the same moment.
            // (update_first: the posterior just computed in this very step)
            const MlView vPost(a.covs + (UF ? t : (t > 0 ? t - 1 : 0)) * N * NX * NX, off_rows, estride, pair_rows);
            double T[R][NX];                 // T = P F' : T[r][i] = sum_k P[r][k] F[i][k]
            double Fr[2][NX];
            FK_UNROLL for (int k = 0; k < NX; ++k) Fr[0][k] = sF[k];
            FK_UNROLL for (int i = 0; i < NX; ++i) {
                if (i + 1 < NX) {
                    FK_UNROLL for (int k = 0; k < NX; ++k) Fr[(i + 1) & 1][k] = sF[(i + 1) * NX + k];
                }
                const double (&Fi)[NX] = Fr[i & 1];
                FK_UNROLL for (int r = 0; r < R; ++r) {
                    double acc = P[r][0] * Fi[0];
                    FK_UNROLL for (int k = 1; k < NX; ++k) acc = fma(P[r][k], Fi[k], acc);
                    T[r][i] = acc;
                }
                if (OUTS && !AOS && !SLAB) {
                    // (at t == 0 this writes the initial P into covs[0], overwritten by step 0's own result later)
                    if constexpr (PAIRS) {
                        // the lane's 27 elements as 13 pairs + 1: iterations 0,2,4,6 send 3 pairs, 8 sends 1 pair + the last
                        if (i % 2 == 0 && i < NX - 1) {
                            FK_UNROLL for (int e = 0; e < 2 * R; e += 2) {
                                const int f0 = i * R + e, f1 = f0 + 1;
                                vPost.store_pair(f0, P[f0 / NX][f0 % NX], P[f1 / NX][f1 % NX]);
                            }
                        } else if (i == NX - 1) {
                            vPost.store_pair(i * R, P[R - 1][NX - 3], P[R - 1][NX - 2]);
                            vPost.store(R * NX - 1, P[R - 1][NX - 1]);
                        }
                    } else {
                        FK_UNROLL for (int e = 0; e < R; ++e) vPost.store((i / R) * NX + (i % R) * R + e, P[i / R][(i % R) * R + e]);
                    }
                }
                FK_STAGE();
            }
            // P' = F T : row i (own) = sum_k F[i][k] T[k][:]  (this lane's column k of F one iteration ahead, like the rows above)
            // Round 6: x' = F x rides on the same coefficients -- this lane's R rows of it (the same products in the same order as
            // the nine rows every lane used to form: 27 fused multiply-adds instead of 81), gathered from their owners afterwards.
            double fk[2][R], Qr[R][NX], xo[R];
            FK_UNROLL for (int r = 0; r < R; ++r) fk[0][r] = myF[r * NX];
            FK_UNROLL for (int k = 0; k < NX; ++k) {
                if (k + 1 < NX) {
                    FK_UNROLL for (int r = 0; r < R; ++r) fk[(k + 1) & 1][r] = myF[r * NX + k + 1];
                }
                if (k == NX - 1) {             // Q's rows for the closing fma: requested early too, into the registers T's spent rows leave
                    FK_UNROLL for (int r = 0; r + 1 < R; ++r)
                        FK_UNROLL for (int j = 0; j < NX; ++j) Qr[r][j] = myQ[r * NX + j];
                }
                double Tk[NX];
                FK_OWNER_ROW(R, tri, Tk, T, k);
                if (k == NX - 1) {
                    FK_UNROLL for (int j = 0; j < NX; ++j) Qr[R - 1][j] = myQ[(R - 1) * NX + j];
                }
                FK_UNROLL for (int r = 0; r < R; ++r) {
                    const double f = fk[k & 1][r];
                    xo[r] = (k == 0) ? f * x[0] : fma(f, x[k], xo[r]);
                    FK_UNROLL for (int j = 0; j < NX; ++j) P[r][j] = (k == 0) ? f * Tk[j] : fma(f, Tk[j], P[r][j]);
                }
                FK_STAGE();
            }
            FK_UNROLL for (int i = 0; i < NX; ++i) {
                const double v = xo[i % R];
                x[i] = owner_value<R, 3>(tri, i, v);
            }
            if constexpr (VAR) {
                // x = (F x) + (B u): the product first, like dot(F, x) + dot(B, u)  (kalman_filter.py:472-475);
                // no control input: B and u are zeros, x + 0 = x
                FK_UNROLL for (int i = 0; i < NX; ++i) {
                    double bu = sB[i * NUC] * u[0];
                    FK_UNROLL for (int k = 1; k < NUC; ++k) bu = fma(sB[i * NUC + k], ((unsigned)k < nu ? u[k] : 0.0), bu);
                    x[i] += bu;
                }
            }
            if (OUTS && !AOS && !SLAB) {
                const MlView vx(a.means_p + t * N * NX, t8, estride, pair_x);
                store_x<NX, PAIRS ? 1 : 0>(vx, x);      // replicated: the quad writes the same bytes
            }
            FK_UNROLL for (int r = 0; r < R; ++r)
                FK_UNROLL for (int j = 0; j < NX; ++j) P[r][j] = fma(a.alpha_sq, P[r][j], Qr[r][j]);
        }
        if constexpr (OUTS && AOS)
            ml_store_aos<R, NX>(x, P, a.means_p + (t * N + w0) * NX, a.covs_p + (t * N + w0) * NX * NX, tile, lane, Lc, valid);
        if constexpr (OUTS && SLAB)
            ml_store_soa_slab<R, NX>(x, P, a.means_p + t * N * NX + w0, a.covs_p + t * N * NX * NX + w0, (unsigned)N * 8u, tile, lane, Lc, valid);
        FK_STAGE();
