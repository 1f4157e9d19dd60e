// kf_mlg_predict.inc -- the predict half of one kf_mlg_kernel step (included by kf_mlg.hip at the two places a step can
// run it: before the update half, or -- update_first -- after it; only one of them exists in any instantiation; see
// kf_ml_predict.inc for why this is a textual inclusion).
        // ---------------------------------------------------------------- predict --
        // Row i of F serves x'[i] = F[i][:] x AND column i of T = P F' in one pass and is requested from LDS one iteration
        // ahead (two row buffers), this lane's column k of F likewise, Q's rows during the last iteration: one wave per
        // SIMD has nothing to cover a ds_read -> s_waitcnt pair with (round 4; same sums in the same order).
        {
            double T[R][NX];                 // T = P F' : T[r][i] = sum_k P[r][k] F[i][k]
            double xn[NX];
            double Fr[2][NX];
            FK_UNROLL for (int k = 0; k < NX; ++k) Fr[0][k] = sF[k];
            FK_UNROLL for (int i = 0; i < NX; ++i) {
                if (i + 1 < NX) {
                    FK_UNROLL for (int k = 0; k < NX; ++k) Fr[(i + 1) & 1][k] = sF[(i + 1) * NX + k];
                }
                const double (&Fi)[NX] = Fr[i & 1];
                {
                    double acc = Fi[0] * x[0];
                    FK_UNROLL for (int k = 1; k < NX; ++k) acc = fma(Fi[k], x[k], acc);
                    xn[i] = acc;
                }
                FK_UNROLL for (int r = 0; r < R; ++r) {
                    double acc = P[r][0] * Fi[0];
                    FK_UNROLL for (int k = 1; k < NX; ++k) acc = fma(P[r][k], Fi[k], acc);
                    T[r][i] = acc;
                }
                FK_STAGE();
            }
            FK_UNROLL for (int i = 0; i < NX; ++i) x[i] = xn[i];
            if constexpr (VAR) {
                // x = (F x) + (B u): the product first, like dot(F, x) + dot(B, u)  (kalman_filter.py:472-475);
                // no control input: B and u are zeros, x + 0 = x
                FK_UNROLL for (int i = 0; i < NX; ++i) {
                    double bu = sB[i * NUC] * u[0];
                    FK_UNROLL for (int k = 1; k < NUC; ++k) bu = fma(sB[i * NUC + k], ((unsigned)k < nu ? u[k] : 0.0), bu);
                    x[i] += bu;
                }
            }
            if constexpr (!AOS) {
                const MlView vx(a.means_p + t * N * NX, t8, estride);
                FK_UNROLL for (int k = 0; k < NX; ++k) vx.store(k, x[k]);      // replicated: the quad writes the same bytes
            }
            FK_STAGE();
            // P' = F T : row i (own) = sum_k F[i][k] T[k][:]
            double fk[2][R], Qr[R][NX];
            FK_UNROLL for (int r = 0; r < R; ++r) fk[0][r] = sF[row[r] * NX];
            FK_UNROLL for (int k = 0; k < NX; ++k) {
                if (k + 1 < NX) {
                    FK_UNROLL for (int r = 0; r < R; ++r) fk[(k + 1) & 1][r] = sF[row[r] * NX + k + 1];
                }
                double Tk[NX];
                FK_OWNER_ROW(R, quad, Tk, T, k);
                if (k == NX - 1) {             // (T's rows are spent once their last broadcast is out)
                    FK_UNROLL for (int r = 0; r < R; ++r)
                        FK_UNROLL for (int j = 0; j < NX; ++j) Qr[r][j] = sQ[row[r] * NX + j];
                }
                FK_UNROLL for (int r = 0; r < R; ++r) {
                    const double f = fk[k & 1][r];
                    FK_UNROLL for (int j = 0; j < NX; ++j) P[r][j] = (k == 0) ? f * Tk[j] : fma(f, Tk[j], P[r][j]);
                }
                FK_STAGE();
            }
            FK_UNROLL for (int r = 0; r < R; ++r)
                FK_UNROLL for (int j = 0; j < NX; ++j) P[r][j] = fma(a.alpha_sq, P[r][j], Qr[r][j]);
        }
        if constexpr (AOS) {
            mlg_store_aos<R, NX>(x, P, row, a.means_p + (t * N + w0) * NX, a.covs_p + (t * N + w0) * NX * NX, tile, lane, valid);
        } else {
            if constexpr (SOA_SLAB) {
                ml_store_rows_soa_slab<R, NX, 16>(P, row, a.covs_p + t * N * NX * NX, N, w0, tile, lane, lane >> 2, valid);
            } else {
                FK_UNROLL for (int r = 0; r < R; ++r) {
                    const MlView vP(a.covs_p + t * N * NX * NX, off_row[r], estride);
                    FK_UNROLL for (int c = 0; c < NX; ++c) vP.store(c, P[r][c]);
                }
            }
        }
        FK_STAGE();
