// mimsem_mass.hpp -- what the C++ hosts share around the fixed-length solve of the 1-form mass matrix: the counterpart of krylov.MassSolver
// (mimsem_amd/krylov.py) and the small pieces beside it, written once for src::SWEqn, HorizSolve, src::ThermalSW_EEC_2 and VertSolveEta.
//   cheb            coefficient tables, safety margins, step counts and the acceptance rule of a logged check (plain arithmetic: a program
//                   that uses nothing else of this header needs no library)
//   DeviceArrays    owner of a class's device arrays (a constructor that throws frees them: members are destroyed, no handler needed)
//   KspHandle       the same for a raw mimsem_ksp*
//   CheckLog        {|r|^2, |ref|^2} pairs of the checked solves in one device array, read with one copy
//   FixedMassSolve  M1 x = b as a Chebyshev semi-iteration of FIXED length on the element-block preconditioner: one context (one call for the
//                   whole solve, or one per sweep) or sharded (exchanges inside, no inner product)
// Header-only, C++17, no HIP toolchain needed (everything goes through include/mimsem_hip.h).
#pragma once
#include <algorithm>
#include <cmath>
#include <functional>
#include <limits>
#include <tuple>
#include <utility>
#include <vector>
#include "mimsem_shard.hpp"

namespace mimsem_host {

namespace cheb {
// p_k = z_k + beta_k p_{k-1}; x += alpha_k p_k for a spectrum inside an ellipse with centre d and foci d +- c (Manteuffel 1977); c2 = c^2
// may be negative (foci d +- i|c|: a spectrum stretched along the imaginary direction) -- the recurrence stays real
inline std::vector<std::pair<double, double>> ellipse(double d, double c2, int steps) {
    std::vector<std::pair<double, double>> co;
    double al = 1.0/d;
    co.emplace_back(al, 0.0);
    for (int k = 1; k < steps; k++) {
        const double be = (k == 1 ? 0.5 : 0.25)*c2*al*al;
        al = 1.0/(d - be/al);
        co.emplace_back(al, be);
    }
    return co;
}
// asymptotic convergence factor for an ellipse with centre d > 0 and semi-axes a_re, a_im
inline double ellipse_rate(double d, double a_re, double a_im) {
    const double c2 = a_re*a_re - a_im*a_im;
    return (a_re + a_im)/(d + std::sqrt(std::max(d*d - c2, 0.0)));
}
// contraction per step on a real interval [lmin, lmax]
inline double interval_rate(double lmin, double lmax) { const double s = std::sqrt(lmax/lmin); return (s - 1.0)/(s + 1.0); }
constexpr double NO_CAP = std::numeric_limits<double>::infinity();
// safety margins (factors for the lower / upper end) around a Ritz interval, the arithmetic of krylov.ritz_margins with the caller's caps:
// three times what an end moved between the 25- and the 40-step estimate, at least 1 %, at most the cap; a re-estimate after a missed
// check (widen > 1) opens them by 10 % / 5 % per unit
inline std::pair<double, double> margins(double lo, double hi, double lo_prev, double hi_prev, double cap_lo, double cap_hi, double widen) {
    return {1.0 - std::min(cap_lo, std::max({0.01, 3.0*std::fabs(lo - lo_prev)/lo, 0.1*(widen - 1.0)})),
            1.0 + std::min(cap_hi, std::max({0.01, 3.0*std::fabs(hi - hi_prev)/hi, 0.05*(widen - 1.0)}))};
}
// steps of the M1 iteration on [l1, l2] until the last sweep sees a residual of rtol
inline int interval_steps(double l1, double l2, double rtol) { return std::max(2, (int)std::ceil(std::log(2.0/rtol)/std::log(1.0/interval_rate(l1, l2)))); }
// steps of an iteration that contracts by `rate` whose RESULT reaches rtol (the [u|h] system, the upwinded 0-form mass)
inline int rate_steps(double rate, double rtol) { return std::max(2, (int)std::ceil(std::log(0.5*rtol)/std::log(rate)) + 1); }
// |r| / |ref| of a logged pair: 0 where both are exactly zero (a slot not written, a zero right-hand side), NaN where the reference is
// no positive number
inline double relative(double r2, double ref2) {
    if (r2 == 0.0 && ref2 == 0.0) return 0.0;
    return ref2 > 0.0 ? std::sqrt(r2/ref2) : std::numeric_limits<double>::quiet_NaN();
}
// THE acceptance rule of a check (NaN compares false: a miss)
inline bool accepted(double r2, double ref2, double bound) { return relative(r2, ref2) <= bound; }
}  // namespace cheb

inline size_t even(long long n) { return (size_t)((n + 1) & ~1LL); }      // (a second row at an even offset starts 16-byte aligned)

class DeviceArrays {
public:
    DeviceArrays() = default;
    ~DeviceArrays() { for (double* p : held) mimsem_free(p); }
    DeviceArrays(const DeviceArrays&) = delete; DeviceArrays& operator=(const DeviceArrays&) = delete;
    double* get(size_t n) {
        held.reserve(held.size() + 1);
        void* p = nullptr;
        check(mimsem_malloc(&p, (long long)(std::max<size_t>(n, 1)*sizeof(double))), "mimsem_malloc");
        held.push_back((double*)p);
        return (double*)p;
    }
private:
    std::vector<double*> held;
};

struct KspHandle {
    mimsem_ksp* h = nullptr;
    KspHandle(Mesh* m, int type) { check(mimsem_ksp_create(m->ctx, type, &h), "mimsem_ksp_create"); }
    ~KspHandle() { mimsem_ksp_destroy(h); }
    KspHandle(const KspHandle&) = delete; KspHandle& operator=(const KspHandle&) = delete;
    operator mimsem_ksp*() const { return h; }
};

class CheckLog {
public:
    // reuse_last: a log that is read at the caller's leisure (HorizSolve) keeps taking solves when it is full -- they share the last slot
    CheckLog(Mesh* m, int nslots_, bool reuse_last_ = false) : mesh(m), nslots(nslots_), reuse_last(reuse_last_), kinds(nslots_, 0) { chk = mem.get(2*(size_t)nslots); clear(); }
    int size() const { return slot; }
    int capacity() const { return nslots; }
    int kind(int k) const { return kinds[k]; }
    void rewind() { slot = 0; }
    void clear() { check(mimsem_memset(mesh->ctx, chk, 0, 2LL*nslots*8), "mimsem_memset"); slot = 0; }
    // the next slot: device {|r|^2, |ref|^2}, for a caller that fills it with launches of its own
    double* claim(int kind = 0) {
        if (slot >= nslots && !reuse_last) throw std::runtime_error("CheckLog: check-norm slots exhausted");
        const int k = slot < nslots ? slot++ : nslots - 1;
        kinds[k] = kind;
        return chk + 2*k;
    }
    // one norm: |v|^2, or (sharded) this rank's ownership-weighted part of it (tmp: n doubles of scratch)
    void norm(const double* v, long long n, double* out, const double* wgt = nullptr, double* tmp = nullptr) {
        if (wgt) mesh->combine(n, 1.0, v, 1, wgt, 0.0, nullptr, tmp);
        check(mimsem_krylov_rowdot(mesh->ctx, 1, n, wgt ? tmp : v, n, v, n, out), "mimsem_krylov_rowdot");
    }
    // (r | ref) side by side, the second row even(n) doubles after the first: both norms with ONE two-row dot (sharded: the two weighted dots)
    void pair(const double* side_by_side, long long n, int kind = 0, const double* wgt = nullptr, double* tmp = nullptr) {
        if (wgt) { weighted(side_by_side, side_by_side + even(n), n, wgt, tmp, kind); return; }
        check(mimsem_krylov_rowdot(mesh->ctx, 2, n, side_by_side, (long long)even(n), side_by_side, (long long)even(n), claim(kind)), "mimsem_krylov_rowdot");
    }
    void two(const double* r, const double* ref, long long n, int kind = 0) { weighted(r, ref, n, nullptr, nullptr, kind); }
    void weighted(const double* r, const double* ref, long long n, const double* wgt, double* tmp, int kind = 0) {
        double* s = claim(kind);
        norm(r, n, s, wgt, tmp); norm(ref, n, s + 1, wgt, tmp);
    }
    // ONE device-to-host copy of the first n slots (default: all); v: 2 n doubles
    void read(double* v, int n = -1) { mesh->to_host(v, chk, 2*(size_t)(n < 0 ? nslots : n)); }
private:
    Mesh* mesh; int nslots; bool reuse_last; std::vector<int> kinds; DeviceArrays mem; double* chk = nullptr; int slot = 0;
};

// a Ritz estimate of the spectral region of a preconditioned operator from `steps` Arnoldi steps: KSP::ritz and Shard::ritz both fit
using Ritz = std::function<void(int steps, double* lo, double* hi, double* im)>;

// the region from TWO estimates (25 and 40 steps) with its margins: what the ends still move between them is the measure of their uncertainty
struct RitzInterval {
    double lo = 0.0, hi = 0.0, im = 0.0, margin_lo = 0.99, margin_hi = 1.01;
    double lmin() const { return margin_lo*lo; }
    double lmax() const { return margin_hi*hi; }
};
inline RitzInterval ritz_interval(const Ritz& ritz, double cap_lo, double cap_hi, double widen) {
    RitzInterval r;
    double lo_prev = 0.0, hi_prev = 0.0;
    for (const int steps : {25, 40}) { lo_prev = r.lo; hi_prev = r.hi; ritz(steps, &r.lo, &r.hi, &r.im); }
    std::tie(r.margin_lo, r.margin_hi) = cheb::margins(r.lo, r.hi, lo_prev, hi_prev, cap_lo, cap_hi, widen);
    return r;
}

class FixedMassSolve {
public:
    bool whole_solve = true;             // one context: a solve is ONE mimsem_block_chebyshev_solve call where the order has it (false: sweep calls)
    int steps = 0;
    double margin_lo = 0.90, margin_hi = 1.05;      // the safety margins in force around the Ritz interval (calibrate)
    bool log_two_dots = false;           // one context: the check norms as two dots instead of one two-row dot

    // M1 of `rows` levels (rows of n1 doubles) with the thickness flags and scale of the host; shard + wgt (ownership weights of all rows):
    // the sharded form.  The element blocks come from the host's PCSetUp (use_blocks) before calibrate()
    FixedMassSolve(Mesh* m, int rows, double scale_, unsigned flags_, Shard* shard = nullptr, const double* wgt_ = nullptr)
        : mesh(m), sh(shard), wgt(wgt_), nk(rows), n1(m->n1), tot((long long)rows*m->n1), ld(rows > 1 ? m->n1 : 0), es(rows > 1 ? m->nEl_ : 0), scale(scale_), flags(flags_) {
        p_ = mem.get((size_t)tot);
        pair_ = mem.get(2*even(tot));
        if (sh) { y = mem.get((size_t)tot); z = mem.get((size_t)tot); }
    }
    void use_blocks(const double* blocks, const double* elem_scale) { blocks_ = blocks; escale_ = elem_scale; }
    // the interval of P M1 with its margins, the step count for rtol and the coefficients; false: no element blocks, or no usable interval
    bool calibrate(const Ritz& ritz, double rtol, double cap_lo, double cap_hi, double widen = 1.0) {
        coef.clear(); flat_.clear();
        if (!blocks_) return false;
        const RitzInterval r = ritz_interval(ritz, cap_lo, cap_hi, widen);
        if (!(r.lo > 0.02)) return false;
        margin_lo = r.margin_lo; margin_hi = r.margin_hi;
        const double l1 = r.lmin(), l2 = r.lmax();
        steps = cheb::interval_steps(l1, l2, rtol);
        coef = cheb::ellipse(0.5*(l1 + l2), 0.25*(l2 - l1)*(l2 - l1), steps);
        for (const auto& ab : coef) { flat_.push_back(ab.first); flat_.push_back(ab.second); }
        return true;
    }
    // sharded: the estimate of the COMPLETED operator from the host's own Arnoldi process (the library's sees one context's elements only)
    Ritz shard_ritz(unsigned seed) {
        return [this, seed](int m, double* lo, double* hi, double* im) {
            sh->ritz(tot, m, wgt, [&](const double* v, double* w) { apply_M1(v); apply_P(y, w); }, [&](double* v) { sh->complete1(v, nk); }, lo, hi, im, seed);
        };
    }
    void shorten(int n) { if ((int)coef.size() > n) { coef.resize(n); flat_.resize(2*(size_t)n); steps = n; } }      // (tests: a solve that must miss its check)

    // x = M1^-1 b from x = 0.  In every form the first step's update is P b and the last step's the preconditioned residual it saw: both norms
    // go into one slot of the log.  MIMSEM_ERR_UNSUPPORTED (an order the fused sweep does not cover) is returned, nothing logged
    int solve(const double* b, double* x, CheckLog& log, int kind = 0) {
        mimsem_ctx* c = mesh->ctx;
        bool whole = false;
        if (!sh && whole_solve) {        // (the first step has no operator pass and clears nothing: the same bits as the sweeps below)
            const int rc = mimsem_block_chebyshev_solve(c, MIMSEM_OP_UMAT, 0, nk, scale, flags, nullptr, 0, blocks_, escale_, es, b, ld, (int)coef.size(), flat_.data(),
                                                        x, ld, ref(), ld, upd(), ld);
            if (rc == MIMSEM_ERR_UNSUPPORTED) whole_solve = false;
            else { check(rc, "mimsem_block_chebyshev_solve"); whole = true; }
        }
        if (!whole) { mesh->zero(tot, x); mesh->zero(tot, p_); }
        for (size_t k = 0; k < coef.size() && !whole; k++) {
            double* u = k + 1 == coef.size() ? upd() : (k == 0 ? ref() : nullptr);
            if (sh) {
                // z = P (b - M1 x) with both element-local sums completed over the halo; p = z + beta p; x += alpha p; u = z -- no inner product
                apply_M1(x);
                mesh->combine(n1, -1.0, y, 0, nullptr, 1.0, b, y, nk);
                apply_P(y, z);
                check(mimsem_krylov_chebyshev_px(c, nk, n1, coef[k].first, coef[k].second, z, n1, nullptr, 0, nullptr, 0, p_, n1, x, n1, u, n1), "mimsem_krylov_chebyshev_px");
                continue;
            }
            const int rc = mimsem_block_chebyshev_sweep(c, MIMSEM_OP_UMAT, 0, nk, scale, flags, nullptr, 0, blocks_, escale_, es, b, ld, coef[k].first, coef[k].second,
                                                        p_, ld, x, ld, u, ld);
            if (k == 0 && rc == MIMSEM_ERR_UNSUPPORTED) return rc;
            check(rc, "mimsem_block_chebyshev_sweep");
        }
        log_last(log, kind);
        return MIMSEM_OK;
    }
    // the check of a solve whose launches the caller issued on these arrays (src::SWEqn's shared launches of two solves)
    void log_last(CheckLog& log, int kind = 0) {
        if (log_two_dots) log.two(upd(), ref(), tot, kind);
        else log.pair(pair_, tot, kind, sh ? wgt : nullptr, y);
    }
    double* upd() const { return pair_; }                        // the last step's update | P b, side by side
    double* ref() const { return pair_ + even(tot); }
    double* p() const { return p_; }
    const double* blocks() const { return blocks_; }
    const double* elem_scale() const { return escale_; }
    const std::vector<double>& flat() const { return flat_; }    // (alpha_0, beta_0, alpha_1, ...)
private:
    void apply_M1(const double* v) {                             // y = M1 v, completed
        check(mimsem_op_apply(mesh->ctx, MIMSEM_OP_UMAT, 0, nk, scale, flags, nullptr, 0, v, ld, y, ld, 1.0), "UMAT");
        sh->complete1(y, nk);
    }
    void apply_P(const double* r, double* w) {                   // w = P r, completed
        check(mimsem_elem_blocks_apply(mesh->ctx, 1, nk, 0, blocks_, 0, escale_, es, r, ld, w, ld, 1.0), "mimsem_elem_blocks_apply");
        sh->complete1(w, nk);
    }
    Mesh* mesh; Shard* sh; const double* wgt; int nk, n1; long long tot, ld, es; double scale; unsigned flags;
    DeviceArrays mem; double *p_ = nullptr, *pair_ = nullptr, *y = nullptr, *z = nullptr;
    const double *blocks_ = nullptr, *escale_ = nullptr;
    std::vector<std::pair<double, double>> coef; std::vector<double> flat_;
};

}  // namespace mimsem_host
