/* Plain Forward / Backward / posterior decoding / null2 / optimal accuracy / bias null of a profile HMM, one scalar loop in node order.
 * TEST INFRASTRUCTURE ONLY: the bulk loop of tests/fb_reference.py, whose numpy statement is the definition (the host test holds the
 * two together to 1e-12).  It shares nothing with p7oracle.c: no PROF, no padded 64-lane layout, no canonical order, no expf tables, no
 * rescaling by xE.  Its parameters are the probability arrays fb_reference.py parsed from the HMM text:
 *     bm[k]            local entry B -> M_k, k = 1..M (index 0 unused)
 *     t[k*7 + j]       MM MI MD IM II DM DD out of node k, k = 0..M, node M's MI II MD DD already zero
 *     odds[x*(M+1)+k]  match odds of residue code x (0..28) at node k (index 0 unused); insert odds are 1
 *     sp[4]            move, loop (N, J, C), E->J, E->C
 * Range: whenever a row's largest value leaves [2^-30, 2^30] the row is multiplied by an exact power of two and the exponent is kept
 * beside it (N and C have exponents of their own), so no rounding depends on it.
 * The file compiles itself three times: real = double (the reference), real = float (the plain float32 evaluation from which
 * fb_reference.py measures its tolerances) and real = long double (the reference of the envelopes: a unihit envelope that holds two
 * domains has, in one row, the first domain's leftovers and the second domain's beginnings further apart than a double's exponent). */
#ifndef FBP_BODY
#define FBP_BODY
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

enum { MM = 0, MI, MD, IM, II, DM, DD };
#define T(k, j) t[(size_t)(k) * 7 + (j)]
#define BIG 1073741824.0       /* 2^30 */

#define real double
#define FN(n) fbp_##n##_f64
#define LDEXP ldexp
#define ILOGB ilogb
#define LOG(v) log((double)(v))
#include "fb_plain.c"
#undef real
#undef FN
#undef LDEXP
#undef ILOGB
#undef LOG
#define real float
#define FN(n) fbp_##n##_f32
#define LDEXP ldexpf
#define ILOGB ilogbf
#define LOG(v) log((double)(v))
#include "fb_plain.c"
#undef real
#undef FN
#undef LDEXP
#undef ILOGB
#undef LOG
#define real long double
#define FN(n) fbp_##n##_f80
#define LDEXP ldexpl
#define ILOGB ilogbl
#define LOG(v) ((double)logl(v))
#include "fb_plain.c"
#undef real
#undef FN
#undef LDEXP
#undef ILOGB
#undef LOG

#else  /* ---- the body, once per `real` ---- */

static real FN(scale)(real v, int e) { return (real)LDEXP(v, e); }

/* Forward.  N is kept as its true value and C with an exponent of its own (ec): in a unihit envelope that holds two domains C carries the
 * first one's mass while the second one's cells still descend from N, further apart than one exponent per row can hold.  The core cells,
 * E, J and B share the row's exponent.  Optional outputs: fM, fI [(L+1)*(M+1)] (rows as stored), xs [(L+1)*5] = E N J B C (as stored),
 * ex [L+1] (the row's exponent), exc [L+1] (C's), lxe [L+1] = log of the true xE of each row (-inf where it is 0).
 * Returns log(C(L) * move) in nats. */
static double FN(fwd)(int M, const real *bm, const real *t, const real *odds, const real *sp, const uint8_t *dsq, int L,
                      real *fM, real *fI, real *xs, int32_t *ex, int32_t *exc, double *lxe)
{
  real move = sp[0], loop = sp[1], eloop = sp[2], emove = sp[3];
  size_t W = (size_t)M + 1;
  real *buf = calloc(6 * W, sizeof(real));
  real *pM = buf, *pI = buf + W, *pD = buf + 2 * W, *cM = buf + 3 * W, *cI = buf + 4 * W, *cD = buf + 5 * W;
  real xN = 1, xJ = 0, xC = 0, xB = xN * move, xE = 0;
  int e = 0, ec = 0;
  if (fM) memset(fM, 0, sizeof(real) * W);
  if (fI) memset(fI, 0, sizeof(real) * W);
  if (xs) { xs[0] = 0; xs[1] = xN; xs[2] = 0; xs[3] = xB; xs[4] = 0; }
  if (ex) ex[0] = 0;
  if (exc) exc[0] = 0;
  if (lxe) lxe[0] = -INFINITY;
  for (int i = 1; i <= L; i++) {
    const real *o = odds + (size_t)dsq[i - 1] * W;
    xE = 0; cM[0] = cI[0] = cD[0] = 0;
    for (int k = 1; k <= M; k++) {
      real sv = xB * bm[k] + pM[k - 1] * T(k - 1, MM) + pI[k - 1] * T(k - 1, IM) + pD[k - 1] * T(k - 1, DM);
      cM[k] = sv * o[k];
      cI[k] = pM[k] * T(k, MI) + pI[k] * T(k, II);
      cD[k] = cM[k - 1] * T(k - 1, MD) + cD[k - 1] * T(k - 1, DD);
      xE += cM[k] + cD[k];
    }
    xN = xN * loop;
    xJ = xJ * loop + xE * eloop;
    { int ne = (xC > 0 && ec > e) ? ec : e; xC = FN(scale)(xC, ec - ne) * loop + FN(scale)(xE, e - ne) * emove; ec = ne; }
    xB = (FN(scale)(xN, -e) + xJ) * move;
    if (xC > (real)BIG) { int d = -ILOGB(xC); xC = FN(scale)(xC, d); ec -= d; }
    real top = xE > xB ? xE : xB;
    if (top < (real)(1.0 / BIG)) for (int k = 1; k <= M; k++) if (cI[k] > top) top = cI[k];
    if (top > (real)BIG || (top > 0 && top < (real)(1.0 / BIG))) {
      int d = -ILOGB(top);
      for (int k = 1; k <= M; k++) { cM[k] = FN(scale)(cM[k], d); cI[k] = FN(scale)(cI[k], d); cD[k] = FN(scale)(cD[k], d); }
      xE = FN(scale)(xE, d); xJ = FN(scale)(xJ, d); xB = FN(scale)(xB, d);
      e -= d;
    }
    if (fM) memcpy(fM + (size_t)i * W, cM, sizeof(real) * W);
    if (fI) memcpy(fI + (size_t)i * W, cI, sizeof(real) * W);
    if (xs) { real *r = xs + (size_t)i * 5; r[0] = xE; r[1] = xN; r[2] = xJ; r[3] = xB; r[4] = xC; }
    if (ex) ex[i] = e;
    if (exc) exc[i] = ec;
    if (lxe) lxe[i] = LOG(xE) + (double)e * M_LN2;
    { real *s; s = pM; pM = cM; cM = s; s = pI; pI = cI; cI = s; s = pD; pD = cD; cD = s; }
  }
  free(buf);
  return LOG(xC * move) + (double)ec * M_LN2;
}

/* Backward, one row at a time from row L down to row 0. */
typedef struct {
  int M, e, en;                  /* e: the exponent of the core cells, E, J and B; en: N's own; C is kept as its true value */
  real *buf, *nM, *nI, *nD, *cM, *cI, *cD, *mn;
  real xE, xN, xJ, xB, xC;
} FN(BWD);

static void FN(bwd_rescale)(FN(BWD) *b)
{
  real mx = b->xE;
  for (int k = 1; k <= b->M; k++) { if (b->cM[k] > mx) mx = b->cM[k]; if (b->cI[k] > mx) mx = b->cI[k]; if (b->cD[k] > mx) mx = b->cD[k]; }
  if (b->xJ > mx) mx = b->xJ; if (b->xB > mx) mx = b->xB;
  if (mx > (real)BIG || (mx > 0 && mx < (real)(1.0 / BIG))) {
    int d = -ILOGB(mx);
    for (int k = 1; k <= b->M; k++) { b->cM[k] = FN(scale)(b->cM[k], d); b->cI[k] = FN(scale)(b->cI[k], d); b->cD[k] = FN(scale)(b->cD[k], d); }
    b->xE = FN(scale)(b->xE, d); b->xJ = FN(scale)(b->xJ, d); b->xB = FN(scale)(b->xB, d);
    b->e -= d;
  }
  if (b->xN > (real)BIG) { int d = -ILOGB(b->xN); b->xN = FN(scale)(b->xN, d); b->en -= d; }
}

/* row L: only C -> T (move) remains; a match or delete state reaches E at cost 1, or goes down the D chain first */
static void FN(bwd_init)(FN(BWD) *b, int M, const real *t, const real *sp)
{
  size_t W = (size_t)M + 2;
  b->M = M; b->e = 0; b->en = 0;
  b->buf = calloc(7 * W, sizeof(real));
  b->nM = b->buf; b->nI = b->buf + W; b->nD = b->buf + 2 * W; b->cM = b->buf + 3 * W; b->cI = b->buf + 4 * W; b->cD = b->buf + 5 * W; b->mn = b->buf + 6 * W;
  b->xC = sp[0]; b->xJ = 0; b->xN = 0; b->xB = 0;
  b->xE = b->xC * sp[3] + b->xJ * sp[2];
  for (int k = M; k >= 1; k--) {
    b->cD[k] = b->xE + T(k, DD) * b->cD[k + 1];
    b->cM[k] = b->xE + T(k, MD) * b->cD[k + 1];
    b->cI[k] = 0;
  }
}

/* row i from row i + 1; x is residue i + 1.  On return the c* arrays and the specials hold row i. */
static void FN(bwd_step)(FN(BWD) *b, const real *bm, const real *t, const real *odds, const real *sp, int x)
{
  int M = b->M;
  real move = sp[0], loop = sp[1], eloop = sp[2], emove = sp[3];
  const real *o = odds + (size_t)x * ((size_t)M + 1);
  { real *s; s = b->nM; b->nM = b->cM; b->cM = s; s = b->nI; b->nI = b->cI; b->cI = s; s = b->nD; b->nD = b->cD; b->cD = s; }
  real *mn = b->mn, *nI = b->nI, *cM = b->cM, *cI = b->cI, *cD = b->cD;
  real xB = 0;
  for (int k = 1; k <= M; k++) { mn[k] = b->nM[k] * o[k]; xB += bm[k] * mn[k]; }
  mn[M + 1] = 0; cD[M + 1] = 0;
  b->xB = xB;
  b->xJ = xB * move + b->xJ * loop;
  b->xC = b->xC * loop;
  b->xE = FN(scale)(b->xC, -b->e) * emove + b->xJ * eloop;
  { int ne = (b->xN > 0 && b->en > b->e) ? b->en : b->e; b->xN = FN(scale)(xB, b->e - ne) * move + FN(scale)(b->xN, b->en - ne) * loop; b->en = ne; }
  for (int k = M; k >= 1; k--) {
    cD[k] = b->xE + T(k, DM) * mn[k + 1] + T(k, DD) * cD[k + 1];
    cI[k] = T(k, IM) * mn[k + 1] + T(k, II) * nI[k];
    cM[k] = b->xE + T(k, MM) * mn[k + 1] + T(k, MI) * nI[k] + T(k, MD) * cD[k + 1];
  }
  FN(bwd_rescale)(b);
}

/* Whole-sequence Forward alone: out[0] = score in nats; lxe[L+1] as above. */
int FN(forward)(int M, const real *bm, const real *t, const real *odds, const real *sp, const uint8_t *dsq, int L, double *out, double *lxe)
{
  out[0] = FN(fwd)(M, bm, t, odds, sp, dsq, L, NULL, NULL, NULL, NULL, NULL, lxe);
  return 0;
}

/* Forward and Backward of the whole sequence, specials only: per residue i = 1..L (index 0 unused)
 *   mocc[i] = 1 - P(residue i emitted by N, J or C),  bt[i] = P(B used at row i - 1),  et[i] = P(E used at row i).
 * out[0] = Forward score, out[1] = the same total from Backward's N(0). */
int FN(occupancy)(int M, const real *bm, const real *t, const real *odds, const real *sp, const uint8_t *dsq, int L,
                  double *out, double *mocc, double *bt, double *et)
{
  real *xs = malloc(sizeof(real) * 5 * ((size_t)L + 1)); int32_t *ex = malloc(sizeof(int32_t) * 2 * ((size_t)L + 1)), *exc = ex + L + 1;
  out[0] = FN(fwd)(M, bm, t, odds, sp, dsq, L, NULL, NULL, xs, ex, exc, NULL);
  real z = xs[(size_t)L * 5 + 4] * sp[0]; int ez = exc[L];
  FN(BWD) b; FN(bwd_init)(&b, M, t, sp);
  mocc[0] = bt[0] = et[0] = 0;
  for (int i = L; i >= 0; i--) {
    if (i < L) FN(bwd_step)(&b, bm, t, odds, sp, dsq[i]);
    const real *f = xs + (size_t)i * 5;
    if (i >= 1) {
      const real *fp = xs + (size_t)(i - 1) * 5;
      et[i] = (double)FN(scale)(f[0] * b.xE / z, ex[i] + b.e - ez);
      real njc = FN(scale)(fp[1] * sp[1] * b.xN / z, b.en - ez) + FN(scale)(fp[2] * sp[1] * b.xJ / z, ex[i - 1] + b.e - ez) +
                 FN(scale)(fp[4] * sp[1] * b.xC / z, exc[i - 1] - ez);
      mocc[i] = (double)((real)1 - njc);
    }
    if (i < L) bt[i + 1] = (double)FN(scale)(f[3] * b.xB / z, ex[i] + b.e - ez);
  }
  out[1] = LOG(b.xN) + (double)b.en * M_LN2;
  free(b.buf); free(xs); free(ex);
  return 0;
}

static void FN(upd)(double *gap, real best, real second) { if (second > -INFINITY && (double)best - (double)second < *gap) *gap = (double)best - (double)second; }

/* Envelope rescoring of dsq[0..Ld-1] (the caller passes the envelope's residues and the unihit specials of the full length).
 * ppM, ppI [(Ld+1)*(M+1)]: work space, on return the posterior probabilities of the match and insert states (row 0 zero).
 * ppX [(Ld+1)*3]: N J C per residue.  null2[20].  coords[4] = hmm_from hmm_to ali_from ali_to, envelope-local (all 0 when no path).
 * out: [0] envsc  [1] Backward's total  [2] largest |sum of a residue's posteriors - 1|  [3] OA score  [4] runner-up gap of the trace
 *      [5] the posteriors the trace collects outside the core: C's of the residues behind the last match state, N's of those before the first.
 * path [M+1]: the residue (envelope-local, 1-based) that match node k emits on the trace, 0 if none (index 0 unused).
 * pp_path [Ld+1]: the posterior of residue i in the state that emits it on the trace (M or I), 0 off ali_from..ali_to.
 * lxe, lbt [Ld+1]: the log of the true xE of every Forward row, and of the largest true value (cells and specials) of every Backward row. */
int FN(envelope)(int M, const real *bm, const real *t, const real *odds, const real *sp, const uint8_t *dsq, int Ld,
                 real *ppM, real *ppI, real *ppX, double *null2, int32_t *coords, double *out, double *lxe, double *lbt,
                 int32_t *path, double *pp_path)
{
  size_t W = (size_t)M + 1;
  real *xs = malloc(sizeof(real) * 5 * ((size_t)Ld + 1)); int32_t *ex = malloc(sizeof(int32_t) * 2 * ((size_t)Ld + 1)), *exc = ex + Ld + 1;
  out[0] = FN(fwd)(M, bm, t, odds, sp, dsq, Ld, ppM, ppI, xs, ex, exc, lxe);
  real z = xs[(size_t)Ld * 5 + 4] * sp[0]; int ez = exc[Ld];
  real *me = calloc(2 * W, sizeof(real)), *ie = me + W;
  real xfac = 0; double dev = 0;
  FN(BWD) b; FN(bwd_init)(&b, M, t, sp);
  ppX[0] = ppX[1] = ppX[2] = 0;
  for (int i = Ld; i >= 0; i--) {
    if (i < Ld) FN(bwd_step)(&b, bm, t, odds, sp, dsq[i]);
    {
      real mx = b.xE; if (b.xJ > mx) mx = b.xJ; if (b.xB > mx) mx = b.xB;
      for (int k = 1; k <= M; k++) { if (b.cM[k] > mx) mx = b.cM[k]; if (b.cI[k] > mx) mx = b.cI[k]; if (b.cD[k] > mx) mx = b.cD[k]; }
      double core = LOG(mx) + (double)b.e * M_LN2, n = b.xN > 0 ? LOG(b.xN) + (double)b.en * M_LN2 : -INFINITY, c = LOG(b.xC);
      lbt[i] = core > n ? core : n; if (c > lbt[i]) lbt[i] = c;
    }
    if (i == 0) break;
    real *fm = ppM + (size_t)i * W, *fi = ppI + (size_t)i * W;
    const real *fp = xs + (size_t)(i - 1) * 5;
    int d = ex[i] + b.e - ez, dp = ex[i - 1] + b.e - ez;
    real rs = 0;
    for (int k = 1; k <= M; k++) {
      fm[k] = FN(scale)(fm[k] * b.cM[k] / z, d); fi[k] = FN(scale)(fi[k] * b.cI[k] / z, d);
      me[k] += fm[k]; ie[k] += fi[k]; rs += fm[k] + fi[k];
    }
    real *px = ppX + (size_t)i * 3;
    px[0] = FN(scale)(fp[1] * sp[1] * b.xN / z, b.en - ez); px[1] = FN(scale)(fp[2] * sp[1] * b.xJ / z, dp); px[2] = FN(scale)(fp[4] * sp[1] * b.xC / z, exc[i - 1] - ez);
    xfac += px[0] + px[1] + px[2]; rs += px[0] + px[1] + px[2];
    if (!(fabs((double)rs - 1.0) <= dev)) dev = fabs((double)rs - 1.0);
  }
  out[1] = LOG(b.xN) + (double)b.en * M_LN2; out[2] = dev;
  free(b.buf);
  /* null2 by expectation */
  for (int x = 0; x < 20; x++) {
    const real *o = odds + (size_t)x * W; real s = 0;
    for (int k = 1; k <= M; k++) s += me[k] / (real)Ld * o[k] + ie[k] / (real)Ld;
    null2[x] = (double)(s + xfac / (real)Ld);
  }
  free(me);
  /* optimal accuracy: the path with the largest expected number of correctly labelled residues, over transitions of probability > 0 */
  size_t R = (size_t)Ld + 1;
  real *oM = malloc(sizeof(real) * 3 * R * W), *oI = oM + R * W, *oD = oI + R * W;
  real *oN = malloc(sizeof(real) * 5 * R), *oB = oN + R, *oE = oB + R, *oJ = oE + R, *oC = oJ + R;
  for (size_t k = 0; k < W; k++) oM[k] = oI[k] = oD[k] = -INFINITY;
  oN[0] = 0; oB[0] = 0; oE[0] = oJ[0] = oC[0] = -INFINITY;
#define GATE(p, v) ((p) > 0 ? (v) : (real)-INFINITY)
#define MAX2(a, b) ((a) > (b) ? (a) : (b))
  for (int i = 1; i <= Ld; i++) {
    real *pm = oM + (size_t)(i - 1) * W, *pi = oI + (size_t)(i - 1) * W, *pd = oD + (size_t)(i - 1) * W;
    real *cm = oM + (size_t)i * W, *ci = oI + (size_t)i * W, *cd = oD + (size_t)i * W;
    const real *qm = ppM + (size_t)i * W, *qi = ppI + (size_t)i * W, *px = ppX + (size_t)i * 3;
    real e = -INFINITY;
    cm[0] = ci[0] = cd[0] = -INFINITY;
    for (int k = 1; k <= M; k++) {
      real best = GATE(bm[k], oB[i - 1]);
      best = MAX2(best, GATE(T(k - 1, MM), pm[k - 1])); best = MAX2(best, GATE(T(k - 1, IM), pi[k - 1])); best = MAX2(best, GATE(T(k - 1, DM), pd[k - 1]));
      cm[k] = best + qm[k];
      ci[k] = MAX2(GATE(T(k, MI), pm[k]), GATE(T(k, II), pi[k])) + qi[k];
      cd[k] = MAX2(GATE(T(k - 1, MD), cm[k - 1]), GATE(T(k - 1, DD), cd[k - 1]));
      e = MAX2(e, cm[k]);
    }
    oE[i] = e;
    oJ[i] = MAX2(oJ[i - 1] + px[1], GATE(sp[2], e));
    oC[i] = MAX2(oC[i - 1] + px[2], GATE(sp[3], e));
    oN[i] = oN[i - 1] + px[0];
    oB[i] = MAX2(oN[i], oJ[i]);
  }
  out[3] = (double)oC[Ld];
  double gap = INFINITY, flank = 0;
  memset(path, 0, sizeof(int32_t) * W); memset(pp_path, 0, sizeof(double) * R);
  int i = Ld, k = 0, st = 0, fi_ = 0, fk = 0, li = 0, lk = 0, done = 0;       /* st: 0 C, 1 E, 2 M, 3 I, 4 D */
  while (!done) {
    real *cm = oM + (size_t)i * W, *cd = oD + (size_t)i * W;
    real *pm = i > 0 ? oM + (size_t)(i - 1) * W : NULL, *pi = i > 0 ? oI + (size_t)(i - 1) * W : NULL, *pd = i > 0 ? oD + (size_t)(i - 1) * W : NULL;
    switch (st) {
    case 0: {
      if (i == 0) { done = 1; break; }
      real a = oC[i - 1] + ppX[(size_t)i * 3 + 2], e = oE[i];
      FN(upd)(&gap, MAX2(a, e), a > e ? e : a);
      if (a >= e) { flank += (double)ppX[(size_t)i * 3 + 2]; i--; } else st = 1;
    } break;
    case 1: {
      real second = -INFINITY; k = 0;
      for (int q = 1; q <= M; q++) if (k == 0 || cm[q] > cm[k]) k = q;
      for (int q = 1; q <= M; q++) if (q != k && cm[q] > second) second = cm[q];
      if (!(cm[k] > -INFINITY)) { done = 1; break; }
      FN(upd)(&gap, cm[k], second);
      li = i; lk = k; st = 2;
    } break;
    case 2: {
      fi_ = i; fk = k;
      path[k] = i; pp_path[i] = (double)ppM[(size_t)i * W + k];
      real c[4] = { GATE(T(k - 1, MM), pm[k - 1]), GATE(T(k - 1, IM), pi[k - 1]), GATE(T(k - 1, DM), pd[k - 1]), GATE(bm[k], oB[i - 1]) };
      int best = 0; for (int q = 1; q < 4; q++) if (c[q] > c[best]) best = q;
      real second = -INFINITY; for (int q = 0; q < 4; q++) if (q != best && c[q] > second) second = c[q];
      FN(upd)(&gap, c[best], second);
      i--;
      if (best == 3) { done = 1; for (int r = 1; r <= i; r++) flank += (double)ppX[(size_t)r * 3]; } else { k--; st = best == 0 ? 2 : best == 1 ? 3 : 4; }
    } break;
    case 3: {
      real a = GATE(T(k, MI), pm[k]), c = GATE(T(k, II), pi[k]);
      FN(upd)(&gap, MAX2(a, c), a > c ? c : a);
      pp_path[i] = (double)ppI[(size_t)i * W + k];
      i--; st = a >= c ? 2 : 3;
    } break;
    case 4: {
      real a = GATE(T(k - 1, MD), cm[k - 1]), c = GATE(T(k - 1, DD), cd[k - 1]);
      FN(upd)(&gap, MAX2(a, c), a > c ? c : a);
      k--; st = a >= c ? 2 : 4;
    } break;
    }
  }
#undef GATE
#undef MAX2
  coords[0] = fk; coords[1] = lk; coords[2] = fi_; coords[3] = li;
  out[4] = gap; out[5] = flank;
  free(oM); free(oN); free(xs); free(ex);
  return 0;
}

/* Forward of the two-state composition model against the background, as odds: p[6] = t00 t01 t10 t11 pi0 pi1, eo1[29] the second
 * state's emission odds (the first state's are 1).  out[0] = log of the total.  L >= 1 (returns -1 otherwise). */
int FN(bias)(const real *p, const real *eo1, const uint8_t *dsq, int L, double *out)
{
  if (L < 1) { out[0] = 0; return -1; }
  real d0 = p[4], d1 = p[5] * eo1[dsq[0]]; int e = 0;
  for (int i = 1; i < L; i++) {
    real n0 = d0 * p[0] + d1 * p[2], n1 = (d0 * p[1] + d1 * p[3]) * eo1[dsq[i]];
    d0 = n0; d1 = n1;
    real mx = d0 > d1 ? d0 : d1;
    if (mx > (real)BIG || (mx > 0 && mx < (real)(1.0 / BIG))) { int d = -ILOGB(mx); d0 = FN(scale)(d0, d); d1 = FN(scale)(d1, d); e -= d; }
  }
  out[0] = LOG(d0 + d1) + (double)e * M_LN2;
  return 0;
}
#endif
