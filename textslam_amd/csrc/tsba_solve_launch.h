// Host side of the reduced-camera-system solve of one LM trial: which kernels it enqueues, and in which order.  Part of tsba.hip's translation
// unit (needs Ctx, LAUNCHK, grid_resident, solve_lds_bytes).  launch_solve: the direct solvers, one launcher each.  launch_ms_solve /
// launch_sv_solve: the solve phases on the factor the last launch_solve left.  launch_solve_full: + conjugate gradients where the map has
// blocks outside the band, with the preconditioner that pcg_choose picks.
// Its device buffers only grow, to exactly the bytes needed (reserve, tsba.hip).

// ---- the direct solvers.  Multi-workgroup blocked Cholesky (tsba_chol.h) of the system in `W` (band bound bw rows below a pose block; bw = N: dense)
static void launch_dense_chol(Ctx *c, Work &W, int bw) {
    const int N = W.N;                                             // worst case: every keyframe free
    LAUNCHK(k_chol_rhs, dim3((N + 255)/256), dim3(256), 0, c->stream, W);
    const int lds_diag = (int)(solve_diag_lds_doubles()*sizeof(double));
    const int lds_panel = (CH_NB + 64)*(CH_NB + 1)*(int)sizeof(double);
    const int lds_upd = 2*64*(CH_NB + 1)*(int)sizeof(double);
    for (int j0 = 0; j0 < N; j0 += CH_NB) {
        LAUNCHK(k_solve_t<true>, dim3(1), dim3(SOLVE_THREADS), lds_diag, c->stream, W, j0);
        // the host only knows the worst case n = N; a shorter last block (nb < NB) still has the rhs row below it
        const int wr = std::max(0, std::min(bw, N - (j0 + 6)));        // band rows below the block, + 1 for the rhs row
        LAUNCHK(k_chol_panel, dim3(wr/64 + 1), dim3(CH_T), lds_panel, c->stream, W, j0, bw);
        const int nt = (wr + 1 + 63)/64;
        if (wr > 0) LAUNCHK(k_chol_update, dim3(nt*(nt + 1)/2), dim3(CH_T), lds_upd, c->stream, W, j0, bw);
    }
    LAUNCHK(k_chol_backsub, dim3(1), dim3(1024), chol_subst_lds_bytes(), c->stream, W, bw);
}
// small windows: one workgroup, S in LDS.  solve_variant 1: the two-panel-wave schedule of tsba_solve.h (A/B runs)
static void launch_lds_solve(Ctx *c, int lds) {
    Work &W = c->W; const int v = c->dbg.solve_variant; const size_t la = solve_la_lds_doubles(W.N)*sizeof(double);
    if ((v == 1 || v == 2) && la <= 160*1024 - 64) LAUNCHK(k_solve_la, dim3(1), dim3(SOLVE_THREADS), (int)la, c->stream, W, v == 2 ? 0 : 1);
    else if (v == 4) LAUNCHK((k_solve_t<false, false>), dim3(1), dim3(SOLVE_THREADS), lds, c->stream, W, 0);      // (the diagonal blocks through the LDS scratch: A/B and bit-identity runs)
    else LAUNCHK(k_solve_t<false>, dim3(1), dim3(SOLVE_THREADS), lds, c->stream, W, 0);
}
// streaming band solve of the system in `W` (tsba_band.h): one workgroup streams down the band of bw rows, factor rows to Lcol; then the back substitution
static void launch_band_stream(Ctx *c, Work &W, int bw, double *Lcol) {
    const int lds = (int)(band_lds_doubles(bw, band_chunk_blocks(bw))*sizeof(double)), nu = (bw + 63)/64;      // nu: tasks per lane of the back substitution
    LAUNCHK(k_band_solve, dim3(1), dim3(SOLVE_THREADS), lds, c->stream, W, bw, band_chunk_blocks(bw), Lcol);
    if (nu <= 1) LAUNCHK(k_band_backsub<1>, dim3(1), dim3(BAND_BS_T), lds, c->stream, W, bw, (const double *)Lcol);
    else if (nu == 2) LAUNCHK(k_band_backsub<2>, dim3(1), dim3(BAND_BS_T), lds, c->stream, W, bw, (const double *)Lcol);
    else LAUNCHK(k_band_backsub<3>, dim3(1), dim3(BAND_BS_T), lds, c->stream, W, bw, (const double *)Lcol);
}

// ---- buffers of the solve phases of the partitioned band solver (tsba_bandms.h: T right-hand sides; tsba_bandsv.h: one), on the factor of the last launch_solve of this level
static bool ms_available(const Ctx *c) { return c->band_stream && c->band_parts > 1 && c->sep_cr && !c->W.ring && c->dbg.sep_solver != 3; }
static int ms_reserve(Ctx *c, int T) {           // buffers for T columns (kept until a larger request or another problem size)
    const size_t n6 = (size_t)c->W.N, labels = (size_t)cr_mmax(0, c->band_parts, 0) + 1, sdim = (size_t)std::max(6, c->cur_bw_rows);
    const size_t per = 4*n6 + 6*labels*sdim;
    if (int rc = reserve(c, c->ms_alloc, "multi-right-hand-side buffers", per*(size_t)T*sizeof(double))) return rc;
    double *q = c->ms_alloc.as<double>(); MsBuf &M = c->ms; M.T = T;
    M.R = q; q += n6*T; M.Wm = q; q += n6*T; M.V = q; q += n6*T; M.X = q; q += n6*T;
    M.G = q; q += labels*sdim*T; M.Z = q; q += labels*sdim*T; M.Xs = q; q += labels*sdim*T; M.Cg = q; q += 2*labels*sdim*T; M.G2 = q;
    c->ms_T = T; return TSBA_OK;
}
static int sv_reserve(Ctx *c) {
    const size_t n6 = ((size_t)c->W.N + 1) & ~(size_t)1, labels = (size_t)cr_mmax(0, c->band_parts, 0) + 1, sdim = (size_t)std::max(6, c->cur_bw_rows);
    if (int rc = reserve(c, c->sv_alloc, "solve-phase buffers", (4*n6 + 7*labels*sdim + 3*labels*sdim*sdim)*sizeof(double))) return rc;
    double *q = c->sv_alloc.as<double>(); MsBuf &M = c->sv; M.T = 1;
    M.Li = q; q += labels*sdim*sdim; M.Pp = q; q += 2*labels*sdim*sdim;
    M.R = q; q += n6; M.Wm = q; q += n6; M.V = q; q += n6; M.X = q; q += n6;
    M.G = q; q += labels*sdim; M.Z = q; q += labels*sdim; M.Xs = q; q += labels*sdim; M.Cg = q; q += 2*labels*sdim; M.G2 = q; q += labels*sdim; M.Lid = q;
    return TSBA_OK;
}
// the separators' inverse factors (k_sv_linv), once per factorisation: both solve phases and the one-launch back substitution of the separator system use them
static void launch_sv_prepare(Ctx *c, double *xreset) {
    const int bwp = std::max(6, c->cur_bw_rows), P = c->band_parts, mmax = cr_mmax(0, P, 0);
    if (mmax > 0) LAUNCHK(k_sv_linv, dim3(mmax), dim3(SV_LT), sv_linv_lds_doubles(bwp)*sizeof(double), c->stream, c->W, bwp, P, (const double *)c->CRfac, (const double *)c->Ssep, c->sv, xreset);
    c->sv_prepared = true;
}

// ---- partitioned band solver: interiors in parallel + separator system (tsba_bandp.h).  bwp: rows of a separator, P: interiors.  Border products + separator assembly:
static void launch_bandp_assemble(Ctx *c, int bwp, int P) {
    Work &W = c->W, &Ws = c->Wsep;
    if (c->sep_cr && (W.ring || (c->dbg.sep_solver != 3 && c->dbg.sep_solver != 4))) {     // block pool: both in one launch (4: the three launches, for A/B runs)
        LAUNCHK(k_bandp_sepf, dim3(W.ring ? P + 1 : P - 1), dim3(BSF_T), (int)(bandp_sepf_lds_doubles()*sizeof(double)), c->stream, W, bwp, P, (const double *)c->Tbuf, (const double *)c->Lb, c->Ssep, Ws.g, Ws.nfree);
        return; }
    hipMemsetAsync(c->Bpart, 0, sizeof(double)*(size_t)P*BANDP_NS*((size_t)bwp*bwp + bwp), c->stream);        // (slices of short interiors stay empty)
    LAUNCHK(k_bandp_border, dim3(P, BANDP_NS), dim3(256), (int)((2*(size_t)BANDP_JC*bwp*6 + 6*BANDP_JC)*sizeof(double)), c->stream, W, bwp, P, (const double *)c->Lb, c->Bpart);
    LAUNCHK(k_bandp_sep, dim3(P - 1), dim3(256), 0, c->stream, W, bwp, P, (const double *)c->Tbuf, (const double *)c->Bpart, c->Ssep, Ws.ldS, Ws.g, Ws.nfree, (int)c->sep_cr);
}
// separator system by block cyclic reduction, one launch per level (tsba_bandcre.h): chains, rings and rings with a tail
static void launch_sep_cre(Ctx *c, int bwp, int P) {
    Work &W = c->W, &Ws = c->Wsep; const int mmax = cr_mmax(W.ring, P, W.ring_g);
    int mlev = mmax;                  // levels h < mlev.  Ring: the loop's separators need h <= G/2 (the root and the ghost are merged at the root, no level for them),
    if (W.ring) { mlev = W.ring_g;    // a tail's separator RING_OFF - j the level of the lowest set bit of j (j < the number of tail interiors)
        for (int hh = 1; hh < P - W.ring_g; hh <<= 1) mlev = std::max(mlev, 2*hh); }
    const int lab0 = W.ring && P > W.ring_g ? RING_OFF - (P - W.ring_g) + 1 : 0;          // lowest separator label (a ring with a tail counts down from RING_OFF)
    const int le = (int)(cre_elim_lds_doubles(bwp)*sizeof(double)), lbk = (int)(cre_back_lds_doubles(bwp)*sizeof(double));
    c->cre_epoch++;                                   // (this factorisation's ordinal: what the K workgroups of a pivot tell each other they have loaded for, k_cre_elim)
    int htop = 1, kb;
    for (int h = 1; h < mlev; htop = h, h <<= 1) {
        const int npiv = cr_level_pivots(mmax, h, lab0, &kb); if (npiv <= 0) continue;
        const int K = std::max(1, std::min(TSBA_CRE_KMAX, 224/npiv));     // workgroups per pivot (they share its product and stores)
        LAUNCHK(k_cre_elim, dim3(npiv*K), dim3(CRE_T), le, c->stream, W, Ws, bwp, P, h, 0, K, kb, c->CRcontrib, c->CRfac, c->CRgate, c->cre_epoch); }
    LAUNCHK(k_cre_elim, dim3(1), dim3(CRE_T), le, c->stream, W, Ws, bwp, P, 0, W.ring ? 2 : 1, 1, 0, c->CRcontrib, c->CRfac, c->CRgate, c->cre_epoch);
    // back substitution: a launch per level -- or one launch through the inverse factors and products of the solve phase (k_sv_linv + k_cre_back_tree)
    // where the iterative path needs those anyway (maps with long-range blocks) or the tree is deep enough to pay for k_sv_linv (28 us at 48-row
    // separators against 10.5 us per level)
    if ((c->far_B > 0 || (htop >= 32 && bwp <= 60)) && ms_available(c) && !(c->dbg.sv_per_level & 2) && c->dbg.pcg_refactor != 1 && mmax >= 2 && grid_resident(c, (const void *)k_cre_back_tree, SV_CT, 0, mmax - 1) && sv_reserve(c) == TSBA_OK) {
        launch_sv_prepare(c, Ws.Sy);
        LAUNCHK(k_cre_back_tree, dim3(mmax - 1), dim3(SV_CT), 0, c->stream, W, Ws, bwp, P, (const double *)c->CRfac, c->sv);
    } else for (int h = htop; h >= 1; h >>= 1) {
        const int npiv = cr_level_pivots(mmax, h, lab0, &kb);
        if (npiv > 0) LAUNCHK(k_cre_back, dim3(npiv), dim3(CRE_BT), lbk, c->stream, W, Ws, bwp, P, h, kb, (const double *)c->CRfac); }
}
// the same by the pivot / update / back kernels of tsba_bandcr.h (sep_solver = 3, chains: A/B runs)
static void launch_sep_cr(Ctx *c, int bwp, int P) {
    Work &W = c->W, &Ws = c->Wsep; const int mmax = cr_mmax(W.ring, P, W.ring_g);
    const int lp = (int)(cr_pivot_lds_doubles(bwp)*sizeof(double)), lu = (int)(cr_update_lds_doubles(bwp)*sizeof(double)), lb = (int)(cr_back_lds_doubles(bwp)*sizeof(double));
    int htop = 1;
    for (int h = 1; h < mmax; htop = h, h <<= 1) {
        const int npiv = (mmax + 2*h - 1)/(2*h);           // >= the pivots (2k + 1) h < m; workgroups past the end return
        LAUNCHK(k_cr_pivot, dim3(npiv), dim3(CR_T), lp, c->stream, W, Ws, bwp, P, h, 0);
        LAUNCHK(k_cr_update, dim3(2*npiv + 1), dim3(CR_T), lu, c->stream, W, Ws, bwp, P, h, npiv);
    }
    LAUNCHK(k_cr_pivot, dim3(1), dim3(CR_T), lp, c->stream, W, Ws, bwp, P, 0, 1);
    LAUNCHK(k_cr_back, dim3(1), dim3(CR_T), lb, c->stream, W, Ws, bwp, P, 0, 1);
    for (int h = htop; h >= 1; h >>= 1) LAUNCHK(k_cr_back, dim3((mmax + 2*h - 1)/(2*h)), dim3(CR_T), lb, c->stream, W, Ws, bwp, P, h, 0);
}
// the separator system: cyclic reduction in log2(P - 1) levels, or (no block pool) the streaming solve of its band of 2 bwp - 6 rows
static void launch_sep_solve(Ctx *c, int bwp, int P) {
    if (!c->sep_cr) launch_band_stream(c, c->Wsep, 2*bwp - 6, c->Lcol_sep);
    else if (c->dbg.sep_solver != 3 || c->W.ring) launch_sep_cre(c, bwp, P);
    else launch_sep_cr(c, bwp, P);
}
static void launch_bandp_solve(Ctx *c, int bwp, int P) {
    Work &W = c->W, &Ws = c->Wsep; Ws.st = W.st; Ws.ldS = (P - 1)*bwp; Ws.N = (P - 1)*bwp; const int cbp = bandp_chunk_blocks(bwp);
    if (!c->sep_cr) hipMemsetAsync(c->Ssep, 0, sizeof(double)*((size_t)Ws.ldS*Ws.ldS + Ws.ldS), c->stream);
    LAUNCHK(k_bandp_factor, dim3(P), dim3(BANDP_T), (int)(bandp_lds_doubles(bwp, cbp)*sizeof(double)), c->stream, W, bwp, cbp, P, c->Lcol, c->Lb, c->Tbuf);
    launch_bandp_assemble(c, bwp, P);
    launch_sep_solve(c, bwp, P);
    const int nup = (bwp + 63)/64, ldsp = (int)((2*(size_t)BAND_CK*(2*(size_t)bwp*6 + 32) + 6*BAND_RINGB + 2*bwp + 64)*sizeof(double));
    if (nup <= 1) LAUNCHK(k_bandp_backsub<1>, dim3(P), dim3(BAND_BS_T), ldsp, c->stream, W, bwp, P, (const double *)c->Lcol, (const double *)c->Lb, (const double *)Ws.Sy);
    else LAUNCHK(k_bandp_backsub<2>, dim3(P), dim3(BAND_BS_T), ldsp, c->stream, W, bwp, P, (const double *)c->Lcol, (const double *)c->Lb, (const double *)Ws.Sy);
    LAUNCHK(k_bandp_dp, dim3((W.n_kf + 255)/256), dim3(256), 0, c->stream, W);
}
// direct solve of the reduced camera system: LDS kernel for small windows, the band solvers where the layout chose them (tsba_layout.h), multi-workgroup blocked Cholesky otherwise
static void launch_solve(Ctx *c) {
    c->sv_prepared = false;
    int use_lds; const int lds = solve_lds_bytes(c, &use_lds), bw = std::max(6, c->cur_bw_rows);
    if (use_lds) launch_lds_solve(c, lds);
    else if (c->band_stream && c->band_parts > 1) launch_bandp_solve(c, bw, c->band_parts);
    else if (c->band_stream) {                                     // narrow band
        if (c->dbg.verbose) fprintf(stderr, "[launch_solve] band stream bw %d cb %d lds %zu B\n", bw, band_chunk_blocks(bw), band_lds_doubles(bw, band_chunk_blocks(bw))*sizeof(double));
        launch_band_stream(c, c->W, bw, c->Lcol); }
    else launch_dense_chol(c, c->W, std::min(c->cur_bw_rows, c->W.N));
}

// ---- solve phase for T right-hand sides (tsba_bandms.h): M.R -> M.X, columns 0 .. T - 1 of the reserved buffers.  mx: the separators in
// product form (tsba_bandmx.h) -- c->sv holds the inverse factors of this factorisation
static void launch_ms_solve(Ctx *c, int T, bool mx = false) {
    Work &W = c->W, &Ws = c->Wsep; Ws.st = W.st; MsBuf M = c->ms; M.T = T;
    const int bwp = std::max(6, c->cur_bw_rows), P = c->band_parts, B = bwp/6, ncg = (T + 63)/64;
    mx = mx && bwp >= 36 && bwp <= MX_SMAX && bwp % 6 == 0;
    const size_t ldsf = ms_cre_lds_doubles(bwp, 1)*sizeof(double), ldsb = (ms_cre_lds_doubles(bwp, 3) + 8*(size_t)(bwp + 2))*sizeof(double), ldsx = mx_lds_doubles(bwp)*sizeof(double);
    LAUNCHK(k_ms_fwd_int, dim3(P, ncg), dim3(64), 0, c->stream, W, bwp, P, (const double *)c->Lcol, M);
    LAUNCHK(k_ms_sep_rhs, dim3(P - 1, ncg), dim3(64*B), 0, c->stream, W, bwp, P, (const double *)c->Lcol, (const double *)c->Lb, M);
    const int mmax = cr_mmax(0, P, 0); int htop = 0, kb; const double *Li = c->sv.Li, *Lid = c->sv.Lid;
    // (the product-form kernels are instantiated per separator size: compile-time loop bounds and LDS offsets)
#define MX_K(SS, KERN, GRID, ...) case SS: LAUNCHK(KERN<SS>, GRID, dim3(MX_T), ldsx, c->stream, __VA_ARGS__); break;
#define MX_LAUNCH(...) switch (bwp) { MX_K(36, __VA_ARGS__) MX_K(42, __VA_ARGS__) MX_K(48, __VA_ARGS__) MX_K(54, __VA_ARGS__) MX_K(60, __VA_ARGS__) MX_K(66, __VA_ARGS__) default: break; }
    for (int h = 1; h < mmax; h <<= 1) { const int npiv = cr_level_pivots(mmax, h, 0, &kb); if (npiv <= 0) continue;
        if (mx) MX_LAUNCH(k_mx_cre_fwd, dim3(npiv, ncg), W, Ws, bwp, P, h, kb, M, Li, Lid)
        else LAUNCHK(k_ms_cre_fwd, dim3(npiv, ncg), dim3(MS_CT), ldsf, c->stream, W, Ws, bwp, P, h, kb, (const double *)c->CRfac, M);
        htop = h; }
    if (mx) MX_LAUNCH(k_mx_cre_root, dim3(1, ncg), W, bwp, P, M, Li, Lid)
    else LAUNCHK(k_ms_cre_root, dim3(1, ncg), dim3(256), ldsf, c->stream, W, Ws, bwp, P, (const double *)c->CRfac, M);
    for (int h = htop; h >= 1; h >>= 1) { const int npiv = cr_level_pivots(mmax, h, 0, &kb); if (npiv <= 0) continue;
        if (mx) MX_LAUNCH(k_mx_cre_back, dim3(npiv, ncg), W, Ws, bwp, P, h, kb, M, Li)
        else LAUNCHK(k_ms_cre_back, dim3(npiv, ncg), dim3(MS_CT), ldsb, c->stream, W, Ws, bwp, P, h, kb, (const double *)c->CRfac, M); }
#undef MX_LAUNCH
#undef MX_K
    LAUNCHK(k_ms_back_border, dim3(P, ncg), dim3(BB_T), 0, c->stream, W, bwp, P, (const double *)c->Lb, M);
    LAUNCHK(k_ms_back_int, dim3(P, ncg), dim3(64), 0, c->stream, W, bwp, P, (const double *)c->Lcol, M);
}

// ---- the same for ONE right-hand side (tsba_bandsv.h): x = M^-1 (rs * r) into c->sv.X.  launch_sv_prepare once per factorisation, then any number of launch_sv_solve.
// bound of an interior's length in pose blocks (bandp_part: the device partitions the FREE poses -- at most n_kf -- into at most band_parts interiors of at
// least 2 B + 2 blocks; where it has to take fewer interiors they stay below twice that)
static int sv_lmax_of(int n_kf, int B, int P) { return std::max(n_kf/std::max(1, P) + 2, 5*B + 8); }
static int sv_lmax(const Ctx *c) { return sv_lmax_of(c->n_kf, std::max(6, c->cur_bw_rows)/6, c->band_parts); }
extern "C++" {            // (a template inside the extern "C" block of tsba.hip)
template <int NREG>      // window rows per lane of the interior kernels (64 NREG >= 6 B): launch_sv_solve picks it
static void launch_sv_solve_t(Ctx *c, const double *r, double rs, const double *rdot, double *rz_part, SvUpd upd) {
    Work &W = c->W, &Ws = c->Wsep; Ws.st = W.st; const MsBuf &M = c->sv;
    const int bwp = std::max(6, c->cur_bw_rows), P = c->band_parts, B = bwp/6, lmax = sv_lmax(c), mmax = cr_mmax(0, P, 0);
    const size_t ldf = sv_fwd_lds_doubles(B)*sizeof(double), ldb = sv_back_lds_doubles(B, lmax)*sizeof(double);
    int htop = 0, kb;
    for (int h = 1; h < mmax; h <<= 1) if (cr_level_pivots(mmax, h, 0, &kb) > 0) htop = h;
    // the highest level has one pivot (3 h >= 2 h >= the number of separators): its forward step, the root and its back substitution are one workgroup's work
    const bool fuse_top = htop > 0 && cr_level_pivots(mmax, htop, 0, &kb) == 1;
    const bool tb_fits = grid_resident(c, (const void *)k_sv_tree_back<NREG>, SV_T, ldb, P);
    const int tree = fuse_top && !(c->dbg.sv_per_level & 1) && grid_resident(c, (const void *)k_sv_cre_tree, SV_CT, 0, mmax - 1);           // the whole tree in one launch (k_sv_cre_tree): its workgroups poll each other
    LAUNCHK(k_sv_fwd_int<NREG>, dim3(P), dim3(SV_T), ldf, c->stream, W, bwp, P, (const double *)c->Lcol, (const double *)c->Lb, r, rs, M, tree, upd);
    if (tree && !(c->dbg.sv_per_level & 8) && tb_fits) {          // ... and the interiors' back substitution in the tree's launch (k_sv_tree_back)
        LAUNCHK(k_sv_tree_back<NREG>, dim3(P), dim3(SV_T), ldb, c->stream, W, bwp, P, htop, lmax, (const double *)c->Lcol, (const double *)c->Lb, M, rdot, rz_part);
        return; }
    if (tree) LAUNCHK(k_sv_cre_tree, dim3(mmax - 1), dim3(SV_CT), 0, c->stream, W, Ws, bwp, P, htop, M);
    else {
        for (int h = 1; h <= htop; h <<= 1) { const int npiv = cr_level_pivots(mmax, h, 0, &kb); if (npiv <= 0 || (fuse_top && h == htop)) continue;
            LAUNCHK(k_sv_cre_fwd, dim3(npiv), dim3(SV_CT), 0, c->stream, W, Ws, bwp, P, h, 0, M); }
        if (fuse_top) LAUNCHK(k_sv_cre_top, dim3(1), dim3(SV_CT), 0, c->stream, W, Ws, bwp, P, htop, M);
        else LAUNCHK(k_sv_cre_root, dim3(1), dim3(SV_CT), 0, c->stream, W, bwp, P, M);
        for (int h = htop; h >= 1; h >>= 1) { const int npiv = cr_level_pivots(mmax, h, 0, &kb);
            if (npiv > 0 && !(fuse_top && h == htop)) LAUNCHK(k_sv_cre_back, dim3(npiv), dim3(SV_CT), 0, c->stream, W, Ws, bwp, P, h, 0, M); }
    }
    LAUNCHK(k_sv_back_int<NREG>, dim3(P), dim3(SV_T), ldb, c->stream, W, bwp, P, lmax, (const double *)c->Lcol, (const double *)c->Lb, M, rdot, rz_part);
}
}
static void launch_sv_solve(Ctx *c, const double *r, double rs, const double *rdot = nullptr, double *rz_part = nullptr, SvUpd upd = SvUpd{0, 0, 0, 0}) {
    if (std::max(6, c->cur_bw_rows)/6 <= 10) launch_sv_solve_t<1>(c, r, rs, rdot, rz_part, upd);      // (a window of up to 10 pose blocks: one row per lane)
    else launch_sv_solve_t<2>(c, r, rs, rdot, rz_part, upd);
}

// ---- The reduced system of one LM trial: a direct solve, or -- band + long-range blocks -- conjugate gradients preconditioned with the band
// solver (tsba_pcg.h).  The host enqueues iteration k only once the device has reached iteration k - 2 (pinned progress word), so a solve
// that converges wastes two iterations of empty launches; every rank of a sharded run iterates on its own copy of the summed system.
static bool pcg_finished(const Ctx *c, unsigned int seq, int it) {      // true: the device reported convergence (or the end of the pass); else waits until it is within two iterations of `it`
    if (!c->hprog || it < 2) return false;
    const auto tw = std::chrono::steady_clock::now();
    for (int spin = 0;; spin++) {
        const unsigned long long w = ((volatile unsigned long long *)c->hprog)[1];
        if ((unsigned int)(w >> 32) == seq) { if (w & 1) return true; if ((int)((w & 0xffffffffu) >> 1) + 2 >= it) return false; }
        PlanPool::cpu_relax();
        if ((spin & 1023) == 1023 && std::chrono::steady_clock::now() - tw > std::chrono::seconds(5)) return false;      // never hang on it
    }
}
// What the conjugate gradients of this trial run on: chosen once, with the reservations the choice depends on (a failed one falls to the next line)
struct PcgChoice {
    bool svok;           // c->sv holds (or is about to hold) the separators' inverse factors: the single-vector solve phase and the product form of the many-column one use them
    bool ecg, wb;        // enlarged conjugate gradients, ECG_T columns per application of M^-1 (pcg_block = 2); else: M^-1 corrected by the low-rank part exactly (loop closures, tsba_wb.h)
    enum { REFACTOR, MS1, SV } minv;      // M^-1 r: the factorisation run again on r / the many-column solve phase with one column / the single-vector solve phase
    bool fused_dot, fused_upd;            // SV: r.z comes out of the solve phase's last kernel (no k_pcg_dot); and the iteration's update step (alpha; x, r) goes into its first (no k_pcg_update)
    int cap; double tol2; unsigned int seq;      // iteration cap, squared relative tolerance, this solve's ordinal in the progress word
    int nmv, pq_off, rz2_off;             // W.pc_part: the matvec's workgroups (a wave per keyframe), where their partial p.q go (nmv <= 2 nbp), the partial r.z of the fused dot
};
static PcgChoice pcg_choose(Ctx *c, const LevelDev &D) {
    PcgChoice ch{}; const int rf = c->dbg.pcg_refactor; const bool msa = ms_available(c);
    ch.cap = c->dbg.pcg_max_it > 0 ? c->dbg.pcg_max_it : 200;
    const double tol = c->dbg.pcg_tol_exp > 0 ? pow(10.0, -(double)c->dbg.pcg_tol_exp) : 1e-10; ch.tol2 = tol*tol;
    ch.seq = ++c->pcg_seq; ch.nmv = (c->n_kf + PCG_MW - 1)/PCG_MW; ch.pq_off = 3*c->pcg_parts + 8; ch.rz2_off = 5*c->pcg_parts + 16;
    const size_t nch = (c->n_kf + ECG_CH - 1)/ECG_CH, kk = 6*(size_t)D.n_wb;
    const size_t ecg_need = (2*(size_t)c->W.N*ECG_T + nch*2*(ECG_T*ECG_T + 1) + 4*(size_t)ECG_T*ECG_T + 4*ECG_T + 16)*sizeof(double);
    const size_t wb_need = (3*kk*kk + 2*kk + (size_t)c->W.N + (kk + 1)*kk + 4*kk + 64 + 2*(size_t)D.n_wb + 16)*sizeof(double);
    ch.svok = msa && rf != 1 && sv_reserve(c) == TSBA_OK;       // (pcg_refactor = 3: as 0 with r.z by its own kernel, for A/B runs)
    // Enlarged conjugate gradients on the many-column solve phase of the band solver (ECG_T columns per application of M^-1): an option (pcg_block = 2).
    // It halves the iterations where the coupling outside the band is a few hundred blocks (outlying eigenvalues, captured 32 at a time), but an
    // application costs 0.8 ms at 5000 keyframes against 0.13 ms of the single-vector solve phase (tsba_bandsv.h) -- measured when the single-vector
    // iteration still re-ran the factorisation (0.57 ms), ms per solve single / enlarged: two loop closures 410 / 303, 1 % long-range points 247 / 320
    ch.ecg = msa && c->dbg.pcg_block == 2 && ms_reserve(c, std::max(ECG_T, c->ms_T)) == TSBA_OK && reserve(c, c->ecg_alloc, nullptr, ecg_need) == TSBA_OK;
    if (ch.ecg) return ch;
    // Loop closures (E touches a few dozen keyframes): the band solve corrected by the low-rank part exactly (tsba_wb.h) is the preconditioner --
    // set up once per trial (one solve phase with k columns, the k x k matrix), then a band solve and a k x k Cholesky per application
    ch.wb = D.n_wb > 0 && msa && c->dbg.far_solver != 3 && ms_reserve(c, std::max(6*D.n_wb, c->ms_T)) == TSBA_OK && reserve(c, c->wb_alloc, nullptr, wb_need) == TSBA_OK;
    // M^-1 on the residual: the solve phase of the partitioned band solver on the factor this trial's first solve left (tsba_bandms.h); where
    // that is not available (a single interior, the sequential separator solve) the factorisation is run again with the residual as right-hand side
    // (measured at 5000 keyframes, one column: 1.3 ms per application against 0.57 ms for the factorisation re-run -- the solve phase pays for 64
    // columns whether it has them or not; it is the default only for the block variants.  pcg_refactor = 2 selects it for the single-vector iteration)
    if (!ch.wb && msa && rf == 2 && ms_reserve(c, std::max(1, c->ms_T)) == TSBA_OK) ch.minv = PcgChoice::MS1;
    else if (ch.svok && (rf == 0 || rf == 3)) ch.minv = PcgChoice::SV;      // (the single-vector solve phase, tsba_bandsv.h: the default)
    else ch.minv = PcgChoice::REFACTOR;
    ch.fused_dot = ch.minv == PcgChoice::SV && !ch.wb && c->band_parts <= 144 && rf == 0;
    ch.fused_upd = ch.fused_dot && !(c->dbg.sv_per_level & 4);
    return ch;
}
static void launch_ecg(Ctx *c, const LevelDev &D, const PcgChoice &ch) {
    Work &W = c->W; const int nbp = c->pcg_parts, B = std::max(6, c->cur_bw_rows)/6, nch = (c->n_kf + ECG_CH - 1)/ECG_CH; const size_t n6 = (size_t)W.N;
    EcgBuf &E = c->ecg; MsBuf M = c->ms; M.T = ECG_T; double *q = c->ecg_alloc.as<double>();
    E.P = q; q += n6*ECG_T; E.Q = q; q += n6*ECG_T; E.part = q; q += (size_t)nch*2*(ECG_T*ECG_T + 1); E.Cm = q; q += ECG_T*ECG_T; E.Lm = q; q += ECG_T*ECG_T + ECG_T;
    E.Y = q; q += ECG_T*ECG_T; E.y1 = q; q += ECG_T; E.scal = q; E.nchunk = nch;
    LAUNCHK(k_ecg_begin, dim3(nbp), dim3(PCG_ET), 0, c->stream, W, M);
    launch_ms_solve(c, ECG_T, ch.svok);
    LAUNCHK(k_ecg_gram, dim3(nch), dim3(256), 0, c->stream, W, (const double *)M.X, (const double *)M.X, (const double *)nullptr, (const double *)M.R, (const double *)M.X, E);
    LAUNCHK(k_ecg_small, dim3(1), dim3(1024), 0, c->stream, W, E, 0, 0, ch.seq, ch.tol2);
    LAUNCHK(k_ecg_update, dim3(nbp), dim3(256), 0, c->stream, W, M, E, 2, 1);
    int it = 0;
    for (; it < ch.cap && !pcg_finished(c, ch.seq, it); it++) {
        LAUNCHK(k_ecg_matvec, dim3(nbp), dim3(256), 0, c->stream, W, D, B, E);
        LAUNCHK(k_ecg_gram, dim3(nch), dim3(256), 0, c->stream, W, (const double *)E.P, (const double *)E.Q, (const double *)M.R, (const double *)nullptr, (const double *)nullptr, E);
        LAUNCHK(k_ecg_small, dim3(1), dim3(1024), 0, c->stream, W, E, 1, it, ch.seq, ch.tol2);
        LAUNCHK(k_ecg_update, dim3(nbp), dim3(256), 0, c->stream, W, M, E, 1, 0);
        launch_ms_solve(c, ECG_T, ch.svok);
        LAUNCHK(k_ecg_gram, dim3(nch), dim3(256), 0, c->stream, W, (const double *)E.Q, (const double *)M.X, (const double *)nullptr, (const double *)M.R, (const double *)M.X, E);
        LAUNCHK(k_ecg_small, dim3(1), dim3(1024), 0, c->stream, W, E, 2, it, ch.seq, ch.tol2);
        LAUNCHK(k_ecg_update, dim3(nbp), dim3(256), 0, c->stream, W, M, E, 2, 0);
    }
    LAUNCHK(k_ecg_finish, dim3(nbp), dim3(PCG_ET), 0, c->stream, W, it);
}
struct WbTrial { double *K2; bool factored; };      // the k x k matrix of this trial's low-rank correction; factored: c->Wk holds its Cholesky factor
// low-rank correction, once per trial: one solve phase with k = 6 n_wb columns, then the k x k matrix (c->Wk: the dense system that factors a copy of it)
static WbTrial launch_wb_setup(Ctx *c, const LevelDev &D, const PcgChoice &ch) {
    Work &W = c->W, &Wk = c->Wk; WbBuf &Bw = c->wb; const int kk = 6*D.n_wb; double *q = c->wb_alloc.as<double>();
    Bw.k = kk; Bw.n_u = D.n_wb; Bw.wb_kf = D.wb_kf; Bw.wb_idx = D.wb_idx;
    Bw.Gm = q; q += (size_t)kk*kk; Bw.T1 = q; q += (size_t)kk*kk; double *K2 = q; q += (size_t)kk*kk; Bw.xu = q; q += kk; Bw.vu = q; q += kk; Bw.z = q; q += W.N;
    memset(&Wk, 0, sizeof(Wk)); Wk.N = kk; Wk.n_kf = D.n_wb; Wk.ldS = kk; Wk.band = 0; Wk.st = W.st;
    Wk.S = q; q += ((size_t)kk + 1)*kk; Wk.Sy = q; q += kk + 8; Wk.g = q; q += kk; Wk.dp = q; q += kk; Wk.LDbuf = q; q += kk + 8;
    Wk.fidx = (int *)q; Wk.nfree = Wk.fidx + D.n_wb + 2;
    MsBuf M = c->ms; M.T = kk;
    LAUNCHK(k_wb_init, dim3(1), dim3(64), 0, c->stream, Wk.fidx, Wk.nfree, D.n_wb);
    LAUNCHK(k_wb_units, dim3(1024), dim3(256), 0, c->stream, W, M, Bw);
    launch_ms_solve(c, kk, ch.svok);
    LAUNCHK(k_wb_gather, dim3(std::min(1024, (kk*kk + 255)/256)), dim3(256), 0, c->stream, W, M, Bw);
    LAUNCHK(k_wb_EG, dim3(D.n_wb), dim3(256), 0, c->stream, W, D, Bw);
    LAUNCHK(k_wb_K2, dim3(std::min(2048, (kk*kk + 255)/256)), dim3(256), 0, c->stream, W, Bw, K2);
    return WbTrial{K2, false};
}
// its application: z = M_W^-1 r (into c->wb.z) from y = M^-1 r = ys * yp[]
static void launch_wb_apply(Ctx *c, const LevelDev &D, WbTrial &T, const double *yp, double ys) {
    Work &W = c->W, &Wk = c->Wk; WbBuf &Bw = c->wb; const int kk = 6*D.n_wb; MsBuf M = c->ms; M.T = kk;
    LAUNCHK(k_wb_rhs, dim3(1), dim3(512), 0, c->stream, W, Bw, yp, ys, Wk.g);
    if (!T.factored) {                                         // once per LM trial: the k x k factor (in place, over a copy), with this right-hand side riding along
        hipMemcpyAsync(Wk.S, T.K2, sizeof(double)*(size_t)kk*kk, hipMemcpyDeviceToDevice, c->stream);
        launch_dense_chol(c, Wk, kk); T.factored = true;
    } else {                                                   // later applications: the two substitutions on that factor (0.28 ms of factorisation each before)
        LAUNCHK(k_chol_rhs, dim3((kk + 255)/256), dim3(256), 0, c->stream, Wk);
        LAUNCHK(k_chol_fwd, dim3(1), dim3(1024), chol_subst_lds_bytes(), c->stream, Wk, kk);
        LAUNCHK(k_chol_backsub, dim3(1), dim3(1024), chol_subst_lds_bytes(), c->stream, Wk, kk);
    }
    LAUNCHK(k_wb_Gw, dim3(1), dim3(512), 0, c->stream, W, Bw, (const double *)Wk.dp);
    LAUNCHK(k_wb_Ex, dim3(D.n_wb), dim3(64), 0, c->stream, W, D, Bw, (const double *)Bw.xu);
    LAUNCHK(k_wb_apply, dim3(512), dim3(256), 0, c->stream, W, M, Bw, yp, ys);
}
// z = M^-1 r of iteration `it`, as *zs * (*zp)[]
static void launch_pcg_minv(Ctx *c, const LevelDev &D, const PcgChoice &ch, WbTrial &T, int it, const double **zp, double *zs) {
    Work &W = c->W; *zp = c->sv.X; *zs = 1.0;
    if (ch.minv == PcgChoice::REFACTOR) { launch_solve(c); *zp = W.Sy; *zs = -1.0; }
    else if (ch.minv == PcgChoice::MS1) { launch_ms_solve(c, 1, ch.svok); *zp = c->ms.X; }
    else if (ch.fused_upd) launch_sv_solve(c, W.pc_r, 1.0, W.pc_r, W.pc_part + ch.rz2_off, SvUpd{1, it, ch.nmv, ch.pq_off});      // (the update step inside the first kernel)
    else if (ch.fused_dot) launch_sv_solve(c, c->sv.R, 1.0, c->sv.R, W.pc_part + ch.rz2_off);      // (r.z comes along: no k_pcg_dot)
    else launch_sv_solve(c, c->sv.R, 1.0);
    if (ch.wb) { launch_wb_apply(c, D, T, *zp, *zs); *zp = c->wb.z; *zs = 1.0; }
}
// single-vector conjugate gradients from the direct solve's x0 = M^-1 b
static void launch_pcg(Ctx *c, const LevelDev &D, const PcgChoice &ch) {
    Work &W = c->W; const int nbp = c->pcg_parts, B = std::max(6, c->cur_bw_rows)/6, nmv = ch.nmv, pq_off = ch.pq_off, rz2_off = ch.rz2_off;
    WbTrial T{}; const double *zp = W.Sy; double zs = -1.0;      // x0 = M^-1 b: what the direct solve left in W.Sy
    if (ch.wb) { T = launch_wb_setup(c, D, ch); launch_wb_apply(c, D, T, zp, zs); zp = c->wb.z; zs = 1.0; }
    LAUNCHK(k_pcg_begin, dim3(nbp), dim3(PCG_ET), 0, c->stream, W, zp, zs);
    if (ch.wb) LAUNCHK(k_pcg_rcheck, dim3(1), dim3(64), 0, c->stream, W, -1, nbp, 0.0);
    double *const r = ch.minv == PcgChoice::MS1 ? c->ms.R : ch.minv == PcgChoice::SV ? c->sv.R : W.g; const double rs = ch.minv == PcgChoice::REFACTOR ? -1.0 : 1.0;      // the residual goes where M^-1 reads it (the factorisation re-run: into -g)
    int it = 0;
    for (; it < ch.cap && !pcg_finished(c, ch.seq, it); it++) {
        LAUNCHK(k_pcg_matvec, dim3(nmv), dim3(64*PCG_MW), 0, c->stream, W, D, it, ch.seq, B, ch.tol2, (it > 0 && ch.fused_dot) ? rz2_off : 0, (it > 0 && ch.fused_dot) ? c->band_parts : nbp, pq_off, zp, zs);
        if (!ch.fused_upd) { LAUNCHK(k_pcg_update, dim3(nbp), dim3(PCG_ET), 0, c->stream, W, it, nbp, pq_off, nmv, r, rs);
            if (ch.wb) LAUNCHK(k_pcg_rcheck, dim3(1), dim3(64), 0, c->stream, W, it, nbp, 1e-20); }      // |r| <= 1e-10 |b|
        launch_pcg_minv(c, D, ch, T, it, &zp, &zs);
        if (!ch.fused_dot) LAUNCHK(k_pcg_dot, dim3(nbp), dim3(PCG_ET), 0, c->stream, W, zp, zs);
    }
    LAUNCHK(k_pcg_finish, dim3(nbp), dim3(PCG_ET), 0, c->stream, W, it);
}
static void launch_solve_full(Ctx *c, const LevelDev &D) {
    launch_solve(c);
    if (D.far_B <= 0) return;
    const PcgChoice ch = pcg_choose(c, D);
    if (ch.svok && !c->sv_prepared) launch_sv_prepare(c, nullptr);       // (the direct solve of a chain has run it already: its back substitution uses the same products)
    if (ch.ecg) launch_ecg(c, D, ch); else launch_pcg(c, D, ch);
}
