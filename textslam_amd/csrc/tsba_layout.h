// Which solver the reduced camera system of an uploaded problem goes through, and the geometry of its storage: pure host arithmetic -- no HIP runtime call,
// no context, no allocation -- so that the choice can be read and tested without a device (tsba_debug_solver_layout, tests/test_solver_layout.py).
// (part of the single translation unit tsba.hip: included there behind the band headers whose constants and helpers it uses)
#pragma once
struct SolverLayout {
    int bw_rows;          // (input) widest band of the levels on the device, in rows
    int use_lds;          // the whole system fits the one-workgroup LDS solver (tsba_solve.h)
    int band;             // storage of S: 0 dense [(N + 1) N], 1 band (skewed view, below)
    int S_up;             // band storage: columns stored right of the diagonal + 1
    size_t LDB, nrow;     // band storage: doubles per row, rows (+ the ghost rows of the first separator on a ring map)
    size_t S_count;       // doubles behind S
    int band_stream;      // the streaming band solver (tsba_band.h) and what builds on it
    int P;                // interiors of the partitioned band solver (tsba_bandp.h); 1: one workgroup streams down the whole band
    int partitioned;      // P > 1: interiors in parallel + a separator system
    int sep_cr;           // separator system by cyclic reduction (tsba_bandcre.h) instead of the sequential streaming solve
    int nsepb, nsep, bws; // separator system: labels (ring: the last one is the ghost of the loop's first separator), rows, band
    int ring, ring_G;     // ring map solved with ghost rows (Work.ring); interiors in the loop (a power of two)
    int ring_k0;          // first keyframe of the loop (-1: not solved as a ring)
    int xchg_wp;          // multi-GPU, band storage: packed row width of the exchange (k_band_pack)
    int err;              // TSBA_ERR_STATE: a ring plan, but the partitioned solver with cyclic reduction is not available for it
};
// multi: the problem is solved by several ranks (they all-reduce the band)
static SolverLayout choose_solver_layout(int n_kf, int bwmax, int ring, int ring_k0, int multi, const tsba_debug_options &dbg) {
    SolverLayout L{}; const int N = 6*n_kf;
    L.bw_rows = bwmax; L.P = 1; L.ring_k0 = -1;
    L.err = ring ? TSBA_ERR_STATE : 0;                                                       // (until the partitioned solver below takes the ring)
    // reduced camera matrix: dense for the LDS solver; for the large-system Cholesky only its band (rows overlap in a skewed
    // view: S(i,j) = base[i*(LDB-1) + j], LDB = band + 96 columns of the diagonal block's upper triangle, where the inverse
    // diagonal factors are kept) -- 80 MB instead of 7.2 GB at 5000 keyframes, and what the ranks all-reduce
    L.use_lds = lds_solver_fits(N);
    // band storage: row i holds the columns [i - Wb, i + up) (skewed view S(i, j) = base[i (LDB - 1) + j]).  The blocked Cholesky of
    // tsba_chol.h writes 96-wide blocks on both sides of the diagonal (up = CH_NB, Wb = band + CH_NB - 1); the streaming / partitioned
    // solvers read the band only (up = 6: the diagonal pose block is stored square) -- 72 instead of 251 columns per row at a band of
    // 60, and the band is cleared before every Schur assembly (60 MB per LM trial at 5000 keyframes with the wide rows)
    const bool stream_ok = bwmax >= 6 && bwmax <= BAND_BW_MAX && band_chunk_blocks(bwmax) > 0 && !dbg.no_band_stream;
    L.S_up = stream_ok ? 6 : CH_NB;
    L.band = !(L.use_lds || (size_t)bwmax + 2*CH_NB - 1 >= (size_t)N);
    if (!L.band) { L.S_count = (size_t)(N + 1)*N; return L; }
    L.nrow = (size_t)N + (ring ? bwmax : 0);                                                 // + the ghost rows of the first separator
    L.LDB = stream_ok ? (size_t)bwmax + 12 : (size_t)bwmax + 2*CH_NB - 1;
    L.S_count = L.nrow*L.LDB + L.LDB;
    L.xchg_wp = multi ? std::min(N, bwmax + 6) : 0;
    if (!stream_ok) return L;
    L.band_stream = 1;
    // substructuring: P interiors on P workgroups + a separator system (again a band, 2 bw - 6 wide)
    // number of interiors: the interiors run in parallel (n_kf / P blocks each, ~3.5 us per block, 5 us once the border makes the
    // panel waves take two rounds), the separator system is sequential again ((P - 1) B blocks at ~4.5 us, 5.5 us when its band
    // exceeds 115 rows): the sum is smallest near sqrt(n_kf t_f / (B t_s))
    const int Bq = bwmax/6;
    const double t_f = bwmax > 57 ? 5.0 : 3.5, t_s = 2*bwmax - 6 > 115 ? 5.5 : 4.5;
    int P = (int)lround(sqrt((double)n_kf*t_f/((double)std::max(Bq, 1)*t_s)));
    bool want_cr = false;
    if (bwmax <= CR_SMAX && dbg.sep_solver != 1) {
        // separator system by cyclic reduction (tsba_bandcre.h): its cost grows with log2(P) only (~45 us per level: one elimination
        // and one back-substitution launch; 130 us with the three kernels of round 1), so many more, shorter interiors pay.
        // Measured at 5000 keyframes / band 10 (ms per 20-iteration solve): P = 64 / 80 / 96 / 112 / 127 / 150 -> 20.6 / 20.3 / 19.4 /
        // 18.6 / 18.0 / 18.8 (150: an eighth level)
        double best = 1e300; int bestP = P;
        for (int q = 4; q <= BANDP_MAXP; q++) {
            if ((n_kf - (q - 1)*Bq)/q < 2*Bq + 2) break;          // (the kernels need 2 B + 2 blocks per interior; until round 6 this loop stopped at 2 B + 8 -- C5: 11 interiors, 9.39 ms; 13: 8.76 ms, tools/diag/gpu_sweep_parts.py)
            int lev = 1; for (int hh = 1; hh < q - 1; hh <<= 1) lev++;
            const double cost = (double)n_kf/q*t_f + 45.0*lev;
            if (cost < best) { best = cost; bestP = q; }
        }
        // (few, long interiors -- some hundred keyframes -- are still cheaper with the sequential separator solve: compare)
        const int Ps = std::max(1, std::min(P, BANDP_MAXP));
        const double cost_seq = (double)n_kf/Ps*t_f + (double)(Ps - 1)*Bq*t_s;
        if (best < cost_seq) { P = bestP; want_cr = true; }
    }
    if (dbg.sep_solver >= 2 && bwmax <= CR_SMAX) want_cr = true;
    if (dbg.band_parts > 0) P = dbg.band_parts;
    P = std::max(1, std::min(P, BANDP_MAXP));
    if (ring) {                       // ring: a power of two interiors in the loop (the separator tree ends in its first separator and the ghost), cyclic reduction only
        const int cap = dbg.band_parts > 0 ? dbg.band_parts : 128, nloop = n_kf - ring_k0;
        int Pr = 4; while (2*Pr <= cap && (nloop - 2*Pr*Bq)/(2*Pr) >= 2*Bq + 8) Pr *= 2;
        L.ring_G = Pr;
        int Pt = 0;                   // a tail before the loop: interiors of about the loop's size
        if (ring_k0 > 0) { const int ql = (nloop - Pr*Bq)/Pr; Pt = std::max(1, std::min(std::min(RING_OFF - 1, BANDP_MAXP - Pr), (ring_k0 + ql/2)/(ql + Bq)));
            while (Pt > 1 && (ring_k0 - (Pt - 1)*Bq)/Pt < 2*Bq + 8) Pt--; }
        P = Pr + Pt; want_cr = true;
    }
    while (!ring && P > 1 && (n_kf - (P - 1)*Bq)/P < ((dbg.band_parts > 0 || want_cr) ? 2*Bq + 2 : 4*Bq + 4)) P--;     // (2 B + 2: the least the kernels take; the sequential separator solve pays only for interiors of a few bands)
    if (P > 1 && bandp_chunk_blocks(bwmax) > 0 && 2*bwmax - 6 <= BAND_BW_MAX && band_chunk_blocks(2*bwmax - 6) > 0) {
        L.partitioned = 1; L.P = P;
        L.nsepb = cr_mmax(ring, P, L.ring_G);
        L.nsep = L.nsepb*bwmax; L.bws = 2*bwmax - 6;
        L.sep_cr = want_cr && P >= 4;
        L.ring = (ring && L.sep_cr) ? 1 : 0;
        if (L.ring) { L.ring_k0 = ring_k0; L.err = 0; }
    }
    return L;
}
