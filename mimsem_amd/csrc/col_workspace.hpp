// mimsem_amd/csrc/col_workspace.hpp -- where every buffer of the column workspace (mimsem_ctx::d_col) lies.  Host only, no HIP and no
// mimsem_ctx: column_kernels.hip carves with it, tests/cpp/col_workspace_cli.cpp checks it with a plain C++ compiler.
//
// One plan struct per user of the workspace: its members are the buffers, its carve() performs every take of that call.  A call
// runs its plan twice (plan_col in column_kernels.hip): on a counting arena, whose final offset is what the call asks of ensure_col,
// then on d_col.  The size of the request and the place of every buffer so come from the same lines; a buffer is added or resized in
// carve() alone.  The arena never pads and never hands memory out twice: a buffer used under a second name is a named member that
// says when its first use ends.
#pragma once
#include <climits>

namespace mimsem {

struct ColDims {
    long long nEl, nk, n2, mp12;      // columns, levels, block size (n*n), quadrature points of an element
    long long nn() const { return n2*n2; }
};

// block-array view X[e][slot][n2*n2] with ns slots per column, and the block-banded matrix of column_hs.inc: nr block rows, nc block
// columns, nb stored blocks per row, the first of them at block column row + lo.  Kernel arguments: plain data.
struct BA { double* p; int ns; };
struct Band { double* p; int nr, nc, lo, nb; };

// take(n) hands out the next n doubles: base + offset, or null while counting (base == null: no arithmetic on it).  An offset that
// would pass LLONG_MAX/8 -- no byte count could hold it -- sets `bad` and the take returns null; nothing wraps.
struct ColArena {
    double* base;
    long long off = 0;
    bool bad = false;
    explicit ColArena(double* b = nullptr) : base(b) {}
    double* take(long long n) {
        if (n < 0 || n > LLONG_MAX/8 - off) { bad = true; return nullptr; }
        double* p = base ? base + off : nullptr;
        off += n;
        return p;
    }
    BA blocks(const ColDims& d, int ns) { BA b; b.ns = ns; b.p = take(d.nEl*ns*d.nn()); return b; }
    Band band(const ColDims& d, int nr, int nc, int lo, int nb) { Band b; b.nr = nr; b.nc = nc; b.lo = lo; b.nb = nb; b.p = take(d.nEl*nr*nb*d.nn()); return b; }
};

// scratch of colop_blocks_into and the stored-block MatMult: coefficients cq [nEl][<= 2 (nk + 1)][mp12], two block arrays of temporaries
// (four of nk slots for EOS_BLOCK_INV), the blocks M, and for the theta diagnoses the right-hand side on the nk + 1 interfaces
struct ColopWS {
    double *cq, *tmpM, *M, *frt;
    void carve(ColArena& a, const ColDims& d, bool rhs) {
        const long long nbmax = d.nEl*(d.nk + 1)*2;
        cq = a.take(nbmax*d.mp12); tmpM = a.take(2*nbmax*d.nn()); M = a.take(nbmax*d.nn());
        frt = rhs ? a.take(d.nEl*(d.nk + 1)*d.n2) : nullptr;
    }
};

// one value per (column, level, quadrature point): mimsem_column_eos, mimsem_column_temp_forcing_hs
struct QuadWS {
    double* q;
    void carve(ColArena& a, const ColDims& d) { q = a.take(d.nEl*d.nk*d.mp12); }
};

// mimsem_colop_block_inverse_apply on nlev levels
struct BlockInvWS {
    double *cq, *M;
    void carve(ColArena& a, const ColDims& d, long long nlev) { const long long nb = d.nEl*nlev; cq = a.take(nb*d.mp12); M = a.take(nb*d.nn()); }
};

// factors of the Helmholtz operator on the wide / row / wave kernels (schur_assemble, schur_operator, mimsem_column_solve_schur_eta)
struct SchurWS {
    double *cq, *tmpM;               // as ColopWS
    BA B, Binv, Ainv, T, Rr, X, Npi, Nrho, M1, G, AB0, AB1, R2, C2, DIVl, DIVu, Gl, Gu, L;      // R2, C2: RHODPI, CONLIN_W stored [k][2]
    double *gpi, *geta, *rlump, *tA, *tB, *tC;
    // the block-Thomas solve of L d_pi = F_pi runs between the right-hand side updates and the back substitution, on buffers free by then:
    double* Gws;                     // = G.p, the sweep's factors: G is taken for this alone
    double* Dinv;                    // = Npi.p, the sweep's inverted diagonals: Npi's last reader is the launch that writes L
    double* th_y;                    // = tB, the sweep's forward vector: tB is otherwise used inside grad() only
    double* th_r;                    // = tA, the refinement's residual: tA's last reader is the F_pi update, the back substitution writes it afresh
    double* th_dd;                   // = tC, the refinement's correction: tC's last reader (the row kernels' tR) is the launch that writes L
    void carve(ColArena& a, const ColDims& d) {
        const int nk = (int)d.nk, nm = nk - 1;
        cq = a.take(d.nEl*(d.nk + 1)*2*d.mp12);
        tmpM = a.take(d.nEl*(d.nk + 1)*2*d.nn()*2);
        B = a.blocks(d, nk); Binv = a.blocks(d, nk); Ainv = a.blocks(d, nm); T = a.blocks(d, nm); Rr = a.blocks(d, nm); X = a.blocks(d, nm);
        Npi = a.blocks(d, nk); Nrho = a.blocks(d, nk); M1 = a.blocks(d, nm); G = a.blocks(d, nk); AB0 = a.blocks(d, nm); AB1 = a.blocks(d, nm);
        R2 = a.blocks(d, 2*nk); C2 = a.blocks(d, 2*nk);
        DIVl = a.blocks(d, nk); DIVu = a.blocks(d, nk); Gl = a.blocks(d, nm); Gu = a.blocks(d, nm);
        L = a.blocks(d, 3*nk);
        gpi = a.take(d.nEl*nm*d.n2); geta = a.take(d.nEl*nm*d.n2); rlump = a.take(d.nEl*nm*d.n2);
        tA = a.take(d.nEl*d.nk*d.n2); tB = a.take(d.nEl*d.nk*d.n2); tC = a.take(d.nEl*d.nk*d.n2);
        Gws = G.p; Dinv = Npi.p; th_y = tB; th_r = tA; th_dd = tC;
    }
};

// the sweep path of the Helmholtz solve (column_dpp.inc): L, the Thomas factors, interface / level vectors
struct SweepWS {
    double *L, *G, *D, *y, *rl, *geta, *fu2;
    void carve(ColArena& a, const ColDims& d) {
        const long long lev = d.nEl*d.nk;
        L = a.take(lev*3*d.nn()); G = a.take(lev*d.nn()); D = a.take(lev*d.nn()); y = a.take(lev*d.n2);
        rl = a.take(lev*d.n2); geta = a.take(lev*d.n2); fu2 = a.take(lev*d.n2);
    }
};

// the fused _3 solve (column_schur3_sweep.inc): the five bands, the penta factors, six block arrays of the walk, two vectors, and the
// dump blocks of the sweep (one per task, <= nk/2 + 1 tasks per column, columns rounded up to 4)
struct S3FusedWS {
    double *L, *Fac, *GGl, *GGu, *Mui, *X, *Binv, *Brti, *yws, *fu2, *dump;
    void carve(ColArena& a, const ColDims& d) {
        const long long lev = d.nEl*d.nk;
        L = a.take(lev*5*d.nn()); Fac = a.take(lev*4*d.nn());
        GGl = a.take(lev*d.nn()); GGu = a.take(lev*d.nn()); Mui = a.take(lev*d.nn()); X = a.take(lev*d.nn()); Binv = a.take(lev*d.nn()); Brti = a.take(lev*d.nn());
        yws = a.take(lev*d.n2); fu2 = a.take(lev*d.n2);
        dump = a.take(((d.nEl + 3)*(d.nk/2 + 1) + 8)*d.nn());
    }
};

// the chain of mimsem_column_solve_schur_3 (column_hs.inc).  `dpp`: the bands come from the row-algebra kernels (the factor launches or
// the chain launches: the same buffers), else from the banded products; `own_cv`: VBA(velz) has a band of its own (not the box flavour);
// `penta`: the five bands are eliminated directly, else through the 2x2 super-blocks Tm, whose row sweep (`rows`) keeps D^-1
struct Schur3WS {
    double* Tm;                      // the super-block form of L, [nEl][K][3][2 n2][2 n2]
    double *cq, *tmpM;               // as ColopWS
    Band B, Ainv, V01, V10, Muinv, Mrhoinv, Npiinv;
    double *tA, *tB, *tC;
    double* rr;                      // = tA, the residual of the super-block refinement step: tA's last reader is the pressure gradient
    Band VBA, Brinv, T, Rr, Brt, Brtinv, Bth, X, Cv, Drho, Nrt, QM, GN, GG, DDM, L;
    Band VAB, t_a, G_rt, DTV1, AinvDTV1, G_pi, DX, D_rt, t_d, Q, GNN, QMD, DD, DGG;      // the banded products only
    Band Mrt;                        // = B: M_rt is VB, read only
    double *Fac, *yws;               // penta: 4 nn and n2 doubles per (column, level); yws also the super-block sweep's
    double *fpad, *dpad, *Gws, *Dinv;
    void carve(ColArena& a, const ColDims& d, bool dpp, bool own_cv, bool penta, bool rows) {
        const int nk = (int)d.nk, nm = nk - 1;
        const long long m = 2*d.n2, K = (d.nk + 1)/2;
        *this = Schur3WS{};
        auto band = [&](int nr, int nc, int lo, int nb) { return a.band(d, nr, nc, lo, nb); };
        Tm = a.take(d.nEl*K*3*m*m);
        cq = a.take(d.nEl*(d.nk + 1)*2*d.mp12);
        tmpM = a.take(d.nEl*(d.nk + 1)*2*d.nn()*2);
        B = band(nk, nk, 0, 1); Ainv = band(nm, nm, 0, 1); V01 = band(nm, nk, 0, 2); V10 = band(nk, nm, -1, 2);
        Muinv = band(nm, nm, 0, 1); Mrhoinv = band(nk, nk, 0, 1); Mrt = B; Npiinv = band(nk, nk, 0, 1);
        tA = a.take(d.nEl*d.nk*d.n2); tB = a.take(d.nEl*d.nk*d.n2); tC = a.take(d.nEl*d.nk*d.n2); rr = tA;
        VBA = band(nk, nm, -1, 2);
        if (dpp) {
            Brinv = band(nk, nk, 0, 1); T = band(nm, nm, 0, 1); Rr = band(nm, nm, 0, 1); Brt = band(nk, nk, 0, 1); Brtinv = band(nk, nk, 0, 1);
            Bth = band(nk, nk, 0, 1); X = band(nm, nm, 0, 1);
            Cv = own_cv ? band(nk, nm, -1, 2) : VBA;        // (the box flavour multiplies by VBA(pressure gradient) itself)
            Drho = band(nk, nm, -1, 2); Nrt = band(nk, nk, 0, 1); QM = band(nk, nk, -1, 3); GN = band(nm, nk, 0, 2); GG = band(nm, nk, 0, 2);
            DDM = band(nk, nm, -2, 4); L = band(nk, nk, -2, 5);
        } else {
            VAB = band(nm, nk, 0, 2); Brinv = band(nk, nk, 0, 1); t_a = band(nm, nk, 0, 2); G_rt = band(nm, nk, 0, 2);
            DTV1 = band(nm, nk, 0, 2); AinvDTV1 = band(nm, nk, 0, 2); T = band(nm, nm, 0, 1); G_pi = band(nm, nk, 0, 2);
            Rr = band(nm, nm, 0, 1); X = band(nm, nm, 0, 1); DX = band(nk, nm, -1, 2);
            Drho = band(nk, nm, -1, 2);
            Brt = band(nk, nk, 0, 1); D_rt = band(nk, nm, -1, 2);
            t_d = band(nk, nk, 0, 1);
            Nrt = band(nk, nk, 0, 1);
            Bth = band(nk, nk, 0, 1); Q = band(nk, nk, -1, 3);
            QM = band(nk, nk, -1, 3); GN = band(nm, nk, 0, 2); GG = band(nm, nk, 0, 2);
            GNN = band(nm, nk, 0, 2); QMD = band(nk, nm, -2, 4); DD = band(nk, nm, -2, 4); DGG = band(nk, nk, -2, 5);
            DDM = band(nk, nm, -2, 4); L = band(nk, nk, -2, 5);
        }
        if (penta) { Fac = a.take(d.nEl*d.nk*4*d.nn()); yws = a.take(d.nEl*d.nk*d.n2); return; }
        fpad = a.take(d.nEl*K*m); dpad = a.take(d.nEl*K*m);
        Gws = a.take(d.nEl*K*m*m); yws = a.take(d.nEl*K*m);
        if (rows) Dinv = a.take(d.nEl*K*m*m);
    }
};

// interface results the level kernels of the two Newton residuals read: mimsem_column_newton_residual has five vectors,
// mimsem_column_newton2_residual the four without wF
struct NewtonWS {
    double *F, *G, *u, *wF, *fwA;
    void carve(ColArena& a, const ColDims& d, bool with_wF) {
        const long long per = d.nEl*d.nk*d.n2;
        F = a.take(per); G = a.take(per); u = a.take(per); wF = with_wF ? a.take(per) : nullptr; fwA = a.take(per);
    }
};

// what the back substitution of mimsem_column_diag_theta_wup reads per interface: G_I = D'_I^-1 U_I for the nk interfaces that have one
// above them (blocks lane-major, as the Thomas factors of SweepWS) and the forward vector y_I on all nk + 1
struct ThetaWupWS {
    double *G, *y;
    void carve(ColArena& a, const ColDims& d) { G = a.take(d.nEl*d.nk*d.nn()); y = a.take(d.nEl*(d.nk + 1)*d.n2); }
};

}  // namespace mimsem
