// spline_plan.h — the scripted racer's trajectory planner, one function for host and device.
//
// What hardcoded.plan() does with scipy per drone (user_controller/HardCodedController.py:63-115): 16 waypoints
// from the start xy and the four nominal gates, a parametric smoothing spline through them
// (splprep(s = 0.1): FITPACK parcur / fpparc, k = 3, idim = 3, unit weights) and splev at L parameter values.
// Float64 only.  No HIP header is needed: under hipcc the functions are __host__ __device__, under a plain
// C++ compiler they are ordinary inline functions (csrc/plan_host.cpp builds the CPU twin from this file).
//
// The fit follows the compiled routine, not scipy's Python restatement of it:
//   part 1 (knots): least-squares spline on the current knots by Givens rotations row by row; new knots are
//     placed by fpknot from one residual pass per fit, nplus of them WITHOUT refitting in between;
//   part 2 (smoothing parameter p): the rows of the discontinuity matrix b / p are rotated into a copy of the
//     triangle, f(p) = fp(p) - s is driven to |f| < tol * s by the rational iteration (fprati), maxit = 20.
// Arrays are indexed from 1 inside the fit, as the Fortran, so every loop bound can be read against it.
#pragma once

#include <math.h>

#if defined(__HIPCC__)
#define ADRP_PLAN_HD __host__ __device__
#else
#define ADRP_PLAN_HD
#endif

namespace adrp_plan {

constexpr int kDeg = 3, kK1 = kDeg + 1, kK2 = kDeg + 2, kDim = 3;
constexpr int kMaxIt = 20;
constexpr double kTol = 1e-3;
constexpr int kHardPoints = 16;          // waypoints of the HardCodedController
constexpr double kHardSmooth = 0.1;      // its splprep(s = 0.1)
constexpr double kCeiling = 2.5;         // "Drone must stay below the ceiling"

// status word of one plan
constexpr int kStatNotIer0 = 1;          // the fit did not end with FITPACK's ier = 0
constexpr int kStatCeiling = 2;          // a sample z >= 2.5
constexpr int kStatKnotShift = 8;        // bits 8..15: knot count n
constexpr int kStatIterShift = 16;       // bits 16..23: p-iterations taken

// The fit of M points: n knots t[0..n), coefficients c[d][0..n-4).
template <int M>
struct Spline {
    int n;
    int flags;      // kStatNotIer0 or 0
    int iters;
    double t[M + kK1];
    double c[kDim][M];
};

// Working set of one fit (about 470 doubles at M = 16), indexed from 1.
template <int M>
struct Work {
    double u[M + 1];
    double t[M + kK1 + 2];
    double a[M + 1][kK1 + 1];      // banded upper triangle of the observation matrix
    double z[kDim][M + 1];         // rotated right-hand sides
    double c[kDim][M + 1];
    double q[M + 1][kK1 + 1];      // the non-zero B-splines at each data point
    double b[M + 1][kK2 + 1];      // discontinuity rows
    double g[M + 1][kK2 + 1];      // working copy of a per p-iteration
    double fpint[M + kK1 + 1];
    int nrdata[M + kK1 + 1];
};

// HardCodedController.py:63-107 (hardcoded.waypoints): x0, y0 the start; gxy the four gates' x, y.
ADRP_PLAN_HD inline void hardcoded_waypoints(double x0, double y0, const double* gxy, double* w /* [16][3] */) {
    const double zl = 0.3, zh = 0.775, zm = (zl + zh) / 2;
    const double g0x = gxy[0], g0y = gxy[1], g1x = gxy[2], g1y = gxy[3], g2x = gxy[4], g2y = gxy[5], g3x = gxy[6], g3y = gxy[7];
    const double mx = (g0x + g1x) / 2, my = (g0y + g1y) / 2;
    const double p[kHardPoints][3] = {
        {x0, y0, 0.3}, {1, 0, zl},
        {g0x + 0.2, g0y + 0.1, zl}, {g0x + 0.1, g0y, zl}, {g0x - 0.1, g0y, zl},
        {mx - 0.7, my - 0.3, zm}, {mx - 0.5, my - 0.6, zm},
        {g1x - 0.3, g1y - 0.2, zh}, {g1x + 0.2, g1y + 0.2, zh},
        {g2x, g2y - 0.4, zl}, {g2x, g2y + 0.2, zl}, {g2x, g2y + 0.2, zh + 0.2},
        {g3x, g3y + 0.1, zh}, {g3x, g3y - 0.1, zh + 0.1},
        {-0.5, -1.2, zh}, {-0.5, -1.4, zh}};
    for (int i = 0; i < kHardPoints; ++i)
        for (int d = 0; d < 3; ++d) w[i * 3 + d] = p[i][d];
}

// fpbspl: the k+1 non-zero B-splines at t(l) <= x < t(l+1) into h[1..4]; knot t(i) is t[i - o]
ADRP_PLAN_HD inline void fpbspl(const double* t, double x, int l, double* h, int o = 0) {
    double hh[kK1];
    h[1] = 1.0;
    for (int j = 1; j <= kDeg; ++j) {
        for (int i = 1; i <= j; ++i) hh[i] = h[i];
        h[1] = 0.0;
        for (int i = 1; i <= j; ++i) {
            const int li = l + i - o, lj = li - j;
            if (t[li] == t[lj]) {
                h[i + 1] = 0.0;
                continue;
            }
            const double f = hh[i] / (t[li] - t[lj]);
            h[i] = h[i] + f * (t[li] - x);
            h[i + 1] = f * (x - t[lj]);
        }
    }
}

// fpgivs / fprota
ADRP_PLAN_HD inline void fpgivs(double piv, double& ww, double& co, double& si) {
    const double store = fabs(piv);
    double dd;
    if (store >= ww) {
        const double r = ww / piv;
        dd = store * sqrt(1.0 + r * r);
    } else {
        const double r = piv / ww;
        dd = ww * sqrt(1.0 + r * r);
    }
    co = ww / dd;
    si = piv / dd;
    ww = dd;
}
ADRP_PLAN_HD inline void fprota(double co, double si, double& a, double& b) {
    const double s1 = a, s2 = b;
    b = co * s2 + si * s1;
    a = co * s1 - si * s2;
}

// fpback: solve the banded upper triangular system a c = z (n rows, bandwidth k); a has row width W
template <int W>
ADRP_PLAN_HD inline void fpback(const double (*a)[W], const double* z, int n, int k, double* c) {
    const int k1 = k - 1;
    c[n] = z[n] / a[n][1];
    int i = n - 1;
    for (int j = 2; j <= n; ++j) {
        double store = z[i];
        const int i1 = j <= k1 ? j - 1 : k1;
        int m = i;
        for (int l = 1; l <= i1; ++l) {
            m += 1;
            store -= c[m] * a[i][l + 1];
        }
        c[i] = store / a[i][1];
        i -= 1;
    }
}

// weighted sum of squared residuals of point `it` (unit weights) with the B-splines saved in q
template <int M>
ADRP_PLAN_HD inline double point_residual(const Work<M>& k, const double* x, int it, int l) {
    const int l0 = l - kK2;
    double term = 0.0;
    for (int d = 0; d < kDim; ++d) {
        double fac = 0.0;
        for (int j = 1; j <= kK1; ++j) fac += k.c[d][l0 + j] * k.q[it][j];
        const double r = fac - x[(it - 1) * kDim + d];
        term += r * r;
    }
    return term;
}

// fpknot (istart = 1): one more knot at the middle data point of the interval with the largest fpint.
// Returns false when no interval can take a knot.
template <int M>
ADRP_PLAN_HD inline bool fpknot(Work<M>& k, int& n, int& nrint) {
    const int kk = (n - nrint - 1) / 2;
    double fpmax = 0.0;
    int jbegin = 1, number = 0, maxpt = 0, maxbeg = 0;
    for (int j = 1; j <= nrint; ++j) {
        const int jpoint = k.nrdata[j];
        if (!(fpmax >= k.fpint[j] || jpoint == 0)) {
            fpmax = k.fpint[j];
            number = j;
            maxpt = jpoint;
            maxbeg = jbegin;
        }
        jbegin += jpoint + 1;
    }
    if (number == 0) return false;
    const int ihalf = maxpt / 2 + 1;
    const int nrx = maxbeg + ihalf;
    const int next = number + 1;
    for (int jj = nrint; jj >= next; --jj) {
        k.fpint[jj + 1] = k.fpint[jj];
        k.nrdata[jj + 1] = k.nrdata[jj];
        const int jk = jj + kk;
        k.t[jk + 1] = k.t[jk];
    }
    k.nrdata[number] = ihalf - 1;
    k.nrdata[next] = maxpt - ihalf;
    const double am = maxpt;
    k.fpint[number] = fpmax * double(k.nrdata[number]) / am;
    k.fpint[next] = fpmax * double(k.nrdata[next]) / am;
    k.t[next + kk] = k.u[nrx];
    n += 1;
    nrint += 1;
    return true;
}

// fpdisc: the jumps of the third derivative of the B-splines at the interior knots into b[1..n-8][1..5]
template <int M>
ADRP_PLAN_HD inline void fpdisc(Work<M>& k, int n) {
    const int k1 = kK1, kd = kDeg, nk1 = n - k1, nrint = nk1 - kd;
    const double fac = double(nrint) / (k.t[nk1 + 1] - k.t[k1]);
    double h[2 * kK1 + 1];
    for (int l = kK2; l <= nk1; ++l) {
        const int lmk = l - k1;
        for (int j = 1; j <= k1; ++j) {
            const int ik = j + k1, lj = l + j, lk = lj - kK2;
            h[j] = k.t[l] - k.t[lk];
            h[ik] = k.t[l] - k.t[lj];
        }
        int lp = lmk;
        for (int j = 1; j <= kK2; ++j) {
            int jk = j;
            double prod = h[j];
            for (int i = 1; i <= kd; ++i) {
                jk += 1;
                prod = prod * h[jk] * fac;
            }
            const int lk = lp + k1;
            k.b[lmk][j] = (k.t[lk] - k.t[lp]) / prod;
            lp += 1;
        }
    }
}

ADRP_PLAN_HD inline double fprati(double& p1, double& f1, double p2, double f2, double& p3, double& f3) {
    double p;
    if (p3 > 0.0) {
        const double h1 = f1 * (f2 - f3), h2 = f2 * (f3 - f1), h3 = f3 * (f1 - f2);
        p = -(p1 * p2 * h3 + p2 * p3 * h1 + p3 * p1 * h2) / (p1 * h1 + p2 * h2 + p3 * h3);
    } else {
        p = (p1 * (f1 - f3) * f2 - p2 * (f2 - f3) * f1) / ((f1 - f2) * f3);
    }
    if (f2 < 0.0) {
        p3 = p2;
        f3 = f2;
    } else {
        p1 = p2;
        f1 = f2;
    }
    return p;
}

// The parametric smoothing fit of M points x[M][3] (parcur with ipar = 0, iopt = 0: fpparc).
template <int M>
ADRP_PLAN_HD inline void smoothing_fit(const double* x, double s, Work<M>& k, Spline<M>& out) {
    constexpr int m = M, k1 = kK1, k2 = kK2, nmin = 2 * kK1, nmax = M + kK1;
    // parameters: cumulative chord length over the total
    k.u[1] = 0.0;
    for (int i = 2; i <= m; ++i) {
        double dist = 0.0;
        for (int d = 0; d < kDim; ++d) {
            const double e = x[(i - 1) * kDim + d] - x[(i - 2) * kDim + d];
            dist += e * e;
        }
        k.u[i] = k.u[i - 1] + sqrt(dist);
    }
    for (int i = 2; i <= m; ++i) k.u[i] = k.u[i] / k.u[m];
    k.u[m] = 1.0;
    const double ub = 0.0, ue = 1.0;

    const double acc = kTol * s;
    int n = nmin, nplus = 0, nrint = 1, nk1 = n - k1;
    int flags = kStatNotIer0, iters = 0;
    double fp = 0.0, fpold = 0.0, fp0 = 0.0, fpms = 0.0;
    k.nrdata[1] = m - 2;
    bool part2 = false, first = true;
    double h[kK2 + 2], xi[kDim];

    for (int iter = 1; iter <= m; ++iter) {
        nrint = n - nmin + 1;
        nk1 = n - k1;
        for (int j = 1; j <= k1; ++j) {
            k.t[j] = ub;
            k.t[nk1 + j] = ue;
        }
        // the least-squares spline on the current knots
        fp = 0.0;
        for (int i = 1; i <= nk1; ++i) {
            for (int d = 0; d < kDim; ++d) k.z[d][i] = 0.0;
            for (int j = 1; j <= k1; ++j) k.a[i][j] = 0.0;
        }
        int l = k1;
        for (int it = 1; it <= m; ++it) {
            const double ui = k.u[it];
            for (int d = 0; d < kDim; ++d) xi[d] = x[(it - 1) * kDim + d];
            while (ui >= k.t[l + 1] && l != nk1) l += 1;
            fpbspl(k.t, ui, l, h);
            for (int i = 1; i <= k1; ++i) k.q[it][i] = h[i];
            int j = l - k1;
            for (int i = 1; i <= k1; ++i) {
                j += 1;
                const double piv = h[i];
                if (piv == 0.0) continue;
                double co, si;
                fpgivs(piv, k.a[j][1], co, si);
                for (int d = 0; d < kDim; ++d) fprota(co, si, xi[d], k.z[d][j]);
                if (i == k1) break;
                int i2 = 1;
                for (int i1 = i + 1; i1 <= k1; ++i1) {
                    i2 += 1;
                    fprota(co, si, h[i1], k.a[j][i2]);
                }
            }
            for (int d = 0; d < kDim; ++d) fp += xi[d] * xi[d];
        }
        if (first) fp0 = fp;
        for (int d = 0; d < kDim; ++d) fpback<kK1 + 1>(k.a, k.z[d], nk1, k1, k.c[d]);
        fpms = fp - s;
        if (fabs(fpms) < acc) {
            // (on the first pass this is the least-squares polynomial: FITPACK's ier = -2, not 0)
            if (!first) flags = 0;
            break;
        }
        if (fpms < 0.0) {
            part2 = !first;
            break;
        }
        if (n == nmax) break;                 // the interpolating spline: ier = -1
        if (first) {
            nplus = 1;
            first = false;
        } else {
            int npl1 = nplus * 2;
            const double rn = nplus;
            if (fpold - fp > acc) npl1 = int(rn * fpms / (fpold - fp));
            int hi = npl1 > nplus / 2 ? npl1 : nplus / 2;
            if (hi < 1) hi = 1;
            nplus = nplus * 2 < hi ? nplus * 2 : hi;
        }
        fpold = fp;
        // the residual sum of every knot interval, once per fit
        double fpart = 0.0;
        int i = 1;
        l = k2;
        for (int it = 1; it <= m; ++it) {
            bool fresh = false;
            if (k.u[it] >= k.t[l] && l <= nk1) {
                fresh = true;
                l += 1;
            }
            const double term = point_residual(k, x, it, l);
            fpart += term;
            if (fresh) {
                const double store = term * 0.5;
                k.fpint[i] = fpart - store;
                i += 1;
                fpart = store;
            }
        }
        k.fpint[nrint] = fpart;
        bool full = false;
        for (int a = 1; a <= nplus; ++a) {
            if (!fpknot(k, n, nrint) || n == nmax) {
                full = true;                  // FITPACK would go on to the interpolating spline
                break;
            }
        }
        if (full) break;
    }

    if (part2) {
        // part 2: the smoothing spline sp(p) on these knots with fp(p) = s
        fpdisc(k, n);
        nk1 = n - k1;
        const int n8 = n - nmin;
        double p1 = 0.0, f1 = fp0 - s, p3 = -1.0, f3 = fpms;
        double p = 0.0;
        for (int i = 1; i <= nk1; ++i) p += k.a[i][1];
        p = double(nk1) / p;
        int ich1 = 0, ich3 = 0;
        const double con1 = 0.1, con9 = 0.9, con4 = 0.04;
        flags = kStatNotIer0;                 // ier = 3 unless the loop ends otherwise
        for (int iter = 1; iter <= kMaxIt; ++iter) {
            iters = iter;
            const double pinv = 1.0 / p;
            for (int i = 1; i <= nk1; ++i) {
                for (int d = 0; d < kDim; ++d) k.c[d][i] = k.z[d][i];
                k.g[i][k2] = 0.0;
                for (int j = 1; j <= k1; ++j) k.g[i][j] = k.a[i][j];
            }
            for (int it = 1; it <= n8; ++it) {
                for (int i = 1; i <= k2; ++i) h[i] = k.b[it][i] * pinv;
                for (int d = 0; d < kDim; ++d) xi[d] = 0.0;
                for (int j = it; j <= nk1; ++j) {
                    const double piv = h[1];
                    double co, si;
                    fpgivs(piv, k.g[j][1], co, si);
                    for (int d = 0; d < kDim; ++d) fprota(co, si, xi[d], k.c[d][j]);
                    if (j == nk1) break;
                    int i2 = k1;
                    if (j > n8) i2 = nk1 - j;
                    for (int i = 1; i <= i2; ++i) {
                        const int i1 = i + 1;
                        fprota(co, si, h[i1], k.g[j][i1]);
                        h[i] = h[i1];
                    }
                    h[i2 + 1] = 0.0;
                }
            }
            for (int d = 0; d < kDim; ++d) fpback<kK2 + 1>(k.g, k.c[d], nk1, k2, k.c[d]);
            fp = 0.0;
            int l = k2;
            for (int it = 1; it <= m; ++it) {
                if (k.u[it] >= k.t[l] && l <= nk1) l += 1;
                fp += point_residual(k, x, it, l);
            }
            fpms = fp - s;
            if (fabs(fpms) < acc) {
                flags = 0;
                break;
            }
            const double p2 = p, f2 = fpms;
            if (ich3 == 0) {
                if (f2 - f3 <= acc) {         // the initial choice of p is too large
                    p3 = p2;
                    f3 = f2;
                    p = p * con4;
                    if (p <= p1) p = p1 * con9 + p2 * con1;
                    continue;
                }
                if (f2 < 0.0) ich3 = 1;
            }
            if (ich1 == 0) {
                if (f1 - f2 <= acc) {         // the initial choice of p is too small
                    p1 = p2;
                    f1 = f2;
                    p = p / con4;
                    if (p3 < 0.0) continue;
                    if (p >= p3) p = p2 * con1 + p3 * con9;
                    continue;
                }
                if (f2 > 0.0) ich1 = 1;
            }
            if (f2 >= f1 || f2 <= f3) break;  // ier = 2
            p = fprati(p1, f1, p2, f2, p3, f3);
        }
    }

    out.n = n;
    out.flags = flags;
    out.iters = iters;
    nk1 = n - k1;
    for (int i = 0; i < M + kK1; ++i) out.t[i] = i < n ? k.t[i + 1] : 0.0;
    for (int d = 0; d < kDim; ++d)
        for (int i = 0; i < M; ++i) out.c[d][i] = i < nk1 ? k.c[d][i + 1] : 0.0;
}

// splev: the curve at parameter x from knots t[0..n) and coefficients c (cd doubles apart per coordinate);
// x >= t[n-4] falls in the last non-empty interval.
ADRP_PLAN_HD inline void spline_eval(const double* t, const double* c, int cd, int n, double x, double* out) {
    const int nk1 = n - kK1;
    int l = kK1;                              // 1-based interval index: t(l) <= x < t(l+1)
    while (l != nk1 && x >= t[l]) l += 1;     // t(l+1) is t[l]
    double h[kK1 + 1];
    fpbspl(t, x, l, h, 1);
    for (int d = 0; d < kDim; ++d) {
        double sp = 0.0;
        for (int j = 1; j <= kK1; ++j) sp += c[d * cd + (l - kK1 + j - 1)] * h[j];
        out[d] = sp;
    }
}

// One drone's plan from its reset observation row: obs[0:2] the start, obs[12:28] the nominal gates.
ADRP_PLAN_HD inline void hardcoded_fit(const float* obs, Work<kHardPoints>& k, Spline<kHardPoints>& out) {
    double gxy[8], w[kHardPoints * 3];
    for (int g = 0; g < 4; ++g) {
        gxy[2 * g] = double(obs[12 + 4 * g]);
        gxy[2 * g + 1] = double(obs[13 + 4 * g]);
    }
    hardcoded_waypoints(double(obs[0]), double(obs[1]), gxy, w);
    smoothing_fit<kHardPoints>(w, kHardSmooth, k, out);
}

ADRP_PLAN_HD inline int status_word(int flags, int n, int iters) { return flags | (n << kStatKnotShift) | (iters << kStatIterShift); }

}  // namespace adrp_plan
