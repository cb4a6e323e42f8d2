// sbm_sf_quadrature.hpp -- the scale-factor entropy integral (reference linear_scale_factor.py:63-81)
//
//     log I,   I = integral du exp(f(u)),   f(u) = -alpha (e^u - 1)^2 - (u - c)^2 / (2 sigma^2),
//     alpha = a B*^2 / (2 T),   c = mu - log B*,   B* = b / a,
//
// by a fixed rule: the same nodes for the same (alpha, c, sigma), no adaptivity, evaluated as a max-subtracted
// log-sum-exp, so that an integrand whose maximum is exp(-1000) gives a finite logarithm.  Compiles for the host too
// (tests/test_sf_quadrature_cpu.py pins it against mpmath); the kernel in sbm_core.hip spreads the panels over the
// lanes of a wavefront.
//
// The integrand.  e^f is the product of a likelihood factor that is Gaussian in B = e^u B* and a prior factor that is
// Gaussian in u.  f is concave for u >= -log 2 only: (e^u - 1)^2 flattens to 1 for u -> -inf, so for c < -log 2 there
// can be a second maximum near the prior's centre, of width >= sigma, next to the one near u = 0, of width
// (2 alpha y (2 y - 1) + 1 / sigma^2)^(-1/2), y = e^u.  Every stationary point lies between 0 and c.
//
// The rule.
//  1. m0 = max(f(0), f(c)) <= max f.  Both factors are <= 1 and unimodal, so {f >= m0 - 40} lies inside
//     [L, U] = {likelihood exponent >= m0 - 40} intersected with {prior exponent >= m0 - 40}; what is left outside is
//     below exp(-40) of the maximum and falls off at least like a Gaussian from there.
//  2. Centres: z_A, the stationary point in [max(c, -log 2), 0] (c < 0) or [0, c] (c >= 0), where f' is monotone:
//     bracketed Newton; and for c < -log 2 z_C, the first stationary point to the right of c: the damped iteration
//     u += sigma^2 f'(u), which cannot step over it because f'' >= -1 / sigma^2 on u <= -log 2.
//  3. [L, p] and [p, U], p halfway between the centres, are each mapped by u = z + s sinh(tau): steps of width s next to
//     the centre z that grow by e^dtau per panel away from it.  Uniform panels of width dtau = 1/4 in tau (more when the
//     128 panels do not reach), a 16-point Gauss-Legendre rule on each.  A Gaussian bump of standard deviation s is
//     integrated to 5e-18 of its mass by this rule on panels up to 4 s wide; panels wider than that lie more than
//     16 s from the centre, where the bump is below exp(-128).
#ifndef SBM_SF_QUADRATURE_HPP
#define SBM_SF_QUADRATURE_HPP

#include <math.h>

#if defined(__HIPCC__)
#define SBM_SFQ_FN __host__ __device__ __forceinline__
#else
#define SBM_SFQ_FN inline
#endif

enum { SBM_SFQ_PANELS = 128, SBM_SFQ_NODES = 16 };

struct sbm_sfq_plan {
  double alpha, c, inv2s2;   // f(u) = -alpha expm1(u)^2 - (u - c)^2 inv2s2
  double z[2], s[2];         // sinh map of the two segments: u = z + s sinh(tau)
  double tau0[2], dtau[2];   // first panel edge and panel width, in tau
  int n[2];                  // panels of each segment; n[0] + n[1] <= SBM_SFQ_PANELS
};

SBM_SFQ_FN double sbm_sfq_f(const sbm_sfq_plan& q, double u) {
  const double t = expm1(u), d = u - q.c;
  return -q.alpha * t * t - d * d * q.inv2s2;
}

// f'(u); y = e^u
SBM_SFQ_FN double sbm_sfq_df(const sbm_sfq_plan& q, double u) {
  const double y = exp(u);
  return -2.0 * q.alpha * y * (y - 1.0) - 2.0 * (u - q.c) * q.inv2s2;
}

// alpha and c of the integrand from the two sums of a scale-factor group; false where B* = b / a is not a positive
// finite number (the reference takes log B*)
SBM_SFQ_FN bool sbm_sfq_params(double a, double b, double mu, double temperature, double* alpha, double* c) {
  const double bstar = b / a;
  if (!(bstar > 0.0) || !(bstar < 1.0e300)) return false;
  *alpha = a * bstar * bstar / (2.0 * temperature);
  *c = mu - log(bstar);
  return *alpha > 0.0 && *alpha < 1.0e300;
}

SBM_SFQ_FN void sbm_sfq_make_plan(double alpha, double c, double sigma, sbm_sfq_plan* out) {
  sbm_sfq_plan q;
  const double s2 = sigma * sigma, ln2 = 0.69314718055994530942;
  q.alpha = alpha; q.c = c; q.inv2s2 = 0.5 / s2;
  // 1. the interval
  const double m0 = fmax(sbm_sfq_f(q, 0.0), sbm_sfq_f(q, c));
  const double drop = 40.0 - m0;
  const double r = sqrt(drop / alpha), w = sigma * sqrt(2.0 * drop);
  const double U = fmin(log1p(r), c + w);
  const double L = r < 1.0 ? fmax(log1p(-r), c - w) : c - w;
  // 2. the centres
  double xl = c >= 0.0 ? 0.0 : fmax(c, -ln2), xr = c >= 0.0 ? c : 0.0;   // f'(xr) <= 0; f' decreases on [xl, xr]
  if (L < xr && U > xl) { xl = fmax(xl, L); xr = fmin(xr, U); }           // (the maximum lies in [L, U])
  double zA = xl;
  if (sbm_sfq_df(q, xl) > 0.0) {
    double x = fmin(fmax(c / (1.0 + 2.0 * alpha * s2), xl), xr);        // where the two Gaussians in u would peak
    for (int it = 0; it < 100; ++it) {
      const double y = exp(x);
      const double d1 = -2.0 * alpha * y * (y - 1.0) - 2.0 * (x - c) * q.inv2s2;
      const double d2 = -2.0 * alpha * y * (2.0 * y - 1.0) - 2.0 * q.inv2s2;
      if (d1 > 0.0) xl = x; else xr = x;
      double xn = x - d1 / d2;
      if (!(xn > xl) || !(xn < xr)) xn = 0.5 * (xl + xr);
      const bool done = fabs(xn - x) <= 1.0e-9 * (fabs(x) + 1.0e-300) || xr - xl <= 0.0;
      x = xn;
      if (done) break;
    }
    zA = x;
  }
  const double yA = exp(zA);
  const double sA = 1.0 / sqrt(2.0 * alpha * yA * fmax(2.0 * yA - 1.0, 0.0) + 1.0 / s2);
  double zC = zA, sC = sA, p = zA;
  if (c < -ln2) {
    double x = c;
    for (int it = 0; it < 40; ++it) {
      const double d1 = sbm_sfq_df(q, x);
      if (!(d1 > 0.0)) break;
      const double xn = fmin(x + s2 * d1, -ln2);
      if (xn - x <= 1.0e-6 * sigma) { x = xn; break; }
      x = xn;
    }
    zC = x; sC = sigma;
    p = 0.5 * (zA + zC);
  }
  p = fmin(fmax(p, L), U);
  // 3. the panels
  q.z[0] = zC; q.s[0] = sC; q.z[1] = zA; q.s[1] = sA;
  const double t0a = asinh((L - zC) / sC), t0b = asinh((p - zC) / sC);
  const double t1a = asinh((p - zA) / sA), t1b = asinh((U - zA) / sA);
  const double span0 = fmax(t0b - t0a, 0.0), span1 = fmax(t1b - t1a, 0.0);
  int n0 = (int)ceil(span0 * 4.0), n1 = (int)ceil(span1 * 4.0);
  if (!(span0 + span1 < 1.0e6)) { n0 = 0; n1 = 0; }                      // (an interval that is no interval: NaN)
  if (n0 + n1 > SBM_SFQ_PANELS) {
    n0 = (int)(SBM_SFQ_PANELS * (span0 / (span0 + span1)) + 0.5);
    if (n0 < 1 && span0 > 0.0) n0 = 1;
    if (n0 > SBM_SFQ_PANELS - 1 && span1 > 0.0) n0 = SBM_SFQ_PANELS - 1;
    n1 = SBM_SFQ_PANELS - n0;
  }
  q.n[0] = n0; q.n[1] = n1;
  q.tau0[0] = t0a; q.dtau[0] = n0 > 0 ? span0 / n0 : 0.0;
  q.tau0[1] = t1a; q.dtau[1] = n1 > 0 ? span1 / n1 : 0.0;
  *out = q;
}

// Panel j of the plan, added to a running log-sum-exp (m, sum): the integral so far is exp(m) * sum.  Start from
// m = -inf, sum = 0.  Panels beyond the plan's add nothing.
SBM_SFQ_FN void sbm_sfq_add_panel(const sbm_sfq_plan& q, int j, double* m, double* sum) {
  // 16-point Gauss-Legendre on [-1, 1]: the eight positive nodes and their weights
  constexpr double gx[8] = {0.095012509837637440185, 0.28160355077925891323, 0.45801677765722738634, 0.61787624440264374845,
                            0.7554044083550030339,   0.86563120238783174388, 0.94457502307323257608, 0.9894009349916499326};
  constexpr double gw[8] = {0.18945061045506849629, 0.18260341504492358887, 0.16915651939500253819, 0.14959598881657673208,
                            0.12462897125553387205, 0.09515851168249278481, 0.062253523938647892863, 0.027152459411754094852};
  if (j < 0 || j >= q.n[0] + q.n[1]) return;
  const int seg = j < q.n[0] ? 0 : 1;
  const int jj = seg ? j - q.n[0] : j;
  const double half = 0.5 * q.dtau[seg], mid = q.tau0[seg] + (2 * jj + 1) * half;
  const double z = q.z[seg], s = q.s[seg];
  double fv[SBM_SFQ_NODES], wj[SBM_SFQ_NODES];
  double pm = -INFINITY;
#pragma unroll
  for (int k = 0; k < SBM_SFQ_NODES; ++k) {
    const double tau = mid + (k & 1 ? half : -half) * gx[k >> 1];
    const double e = exp(tau), ei = 1.0 / e;
    fv[k] = sbm_sfq_f(q, z + s * 0.5 * (e - ei));
    wj[k] = gw[k >> 1] * half * s * 0.5 * (e + ei);       // weight x du / dtau
    pm = fmax(pm, fv[k]);
  }
  if (!(pm > -INFINITY)) return;                           // every node underflowed (or is NaN): nothing to add
  const double mn = fmax(*m, pm);
  double acc = *sum * exp(*m - mn);                        // (exp(-inf) = 0 on the first panel)
#pragma unroll
  for (int k = 0; k < SBM_SFQ_NODES; ++k) acc += wj[k] * exp(fv[k] - mn);
  *m = mn;
  *sum = acc;
}

// the whole rule on one thread (host use; the kernel spreads the panels over a wavefront)
SBM_SFQ_FN double sbm_sfq_log_integral(double alpha, double c, double sigma) {
  sbm_sfq_plan q;
  sbm_sfq_make_plan(alpha, c, sigma, &q);
  double m = -INFINITY, sum = 0.0;
  for (int j = 0; j < q.n[0] + q.n[1]; ++j) sbm_sfq_add_panel(q, j, &m, &sum);
  return m + log(sum);
}

#endif /* SBM_SF_QUADRATURE_HPP */
