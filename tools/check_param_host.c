/* Stand-alone check of the host arithmetic of the parameter-error entry (jur_scene.c: jur_param_layout, jur_param_check_args,
 * jur_param_check_bwptr, jur_param_check_values, jur_param_maps), meant for a sanitizer build on the CPU; no GPU, no
 * library:
 *
 *   gcc -std=gnu99 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=undefined -D__HIP_PLATFORM_AMD__ \
 *       -I/opt/rocm/include -Iinclude -Ijurassic-gpu_amd/csrc -DJUR_ND=100 -DJUR_NG=30 \
 *       -o check_param_host tools/check_param_host.c jurassic-gpu_amd/csrc/jur_scene.c -lm && ./check_param_host
 *
 * 400 seeded ragged scenes of 0 .. 40 rays in 1 .. 7 slices, widths w and wb of 0, 1, 2, 7, 63, 64, 65 and 130 among them,
 * slices without rays, rays without a slice (any width in rowptr_b), the rays of the slices interleaved; every array
 * malloc'ed to its exact size so that a read or write beyond it is an error of the sanitizer.  Checked per scene: every
 * offset of jur_param_layout against a direct count, with all outputs, with each alone and with none (a first call
 * counts); the tile map covers every (element, parameter) pair of every slice exactly once and counts what its first
 * call counted; the checks of bwptr and of the values accept what is right; every refusal is planted once and held to
 * its words, the outputs of a refused layout untouched; what lies above the diagonal of a full covariance holds NaN and
 * is never read. */
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "jur_internal.h"

static char g_msg[512];
void jur_set_error(char const *fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_msg, sizeof g_msg, fmt, ap);
  va_end(ap);
}

static unsigned long long g_state = 88172645463325252ULL;
static unsigned long long rnd(void) { g_state ^= g_state << 13; g_state ^= g_state >> 7; g_state ^= g_state << 17; return g_state; }

static int refused(long rc, char const *words, char const *what) {
  if (rc == JUR_EINVAL && 0 == strcmp(g_msg, words)) return 1;
  printf("%s: expected JUR_EINVAL with \"%s\", got %ld: %s\n", what, words, rc, g_msg);
  return 0;
}

static long const EDGES[] = {0, 1, 2, 7, 63, 64, 65, 130};
#define NEDGE ((long)(sizeof EDGES / sizeof EDGES[0]))
#define SENT (-77L)

static long *longs(long n) { return (long *)malloc(sizeof(long) * (size_t)(n > 0 ? n : 1)); }

static int check_scene(int trial) {
  long const nslice = 1 + (long)(rnd() % 7), nr = (long)(rnd() % 41);
  long *w = longs(nslice), *wb = longs(nslice), *wptr = longs(nslice + 1), *used = longs(nslice);
  int *sid = (int *)malloc(sizeof(int) * (size_t)(nr ? nr : 1));
  long *rowptr = longs(nr + 1), *rowptr_b = longs(nr + 1);
  int ok = 1;
  char words[512];
  wptr[0] = 0;
  for (long q = 0; q < nslice; q++) {
    w[q] = EDGES[1 + rnd() % (NEDGE - 1)];                        /* (a slice has elements) */
    wb[q] = EDGES[rnd() % NEDGE];
    wptr[q + 1] = wptr[q] + w[q];
    used[q] = 0;
  }
  rowptr[0] = rowptr_b[0] = 0;
  for (long r = 0; r < nr; r++) {
    sid[r] = (r == 0 || rnd() % 8 == 0) ? -1 : (int)(rnd() % (unsigned long long)nslice);
    rowptr[r + 1] = rowptr[r] + (sid[r] < 0 ? 0 : w[sid[r]]);
    rowptr_b[r + 1] = rowptr_b[r] + (sid[r] < 0 ? (long)(rnd() % 4) : wb[sid[r]]);
    if (sid[r] >= 0) used[sid[r]]++;
  }
  /* the direct count */
  long *bw = longs(nslice + 1), *cp = longs(nslice + 1), *bb = longs(nslice + 1);
  bw[0] = cp[0] = bb[0] = 0;
  for (long q = 0; q < nslice; q++) {
    long const x = used[q] ? wb[q] : 0;
    bw[q + 1] = bw[q] + x; cp[q + 1] = cp[q] + w[q] * x; bb[q + 1] = bb[q] + x * x;
  }
  long *o1 = longs(nslice + 1), *o2 = longs(nslice + 1), *o3 = longs(nslice + 1);
  long const n0 = jur_param_layout(nslice, wptr, nr, rowptr, rowptr_b, sid, NULL, NULL, NULL);
  long const n1 = jur_param_layout(nslice, wptr, nr, rowptr, rowptr_b, sid, o1, o2, o3);
  if (n0 != cp[nslice] || n1 != n0) { printf("trial %d: the layout counts %ld and %ld, the scene has %ld\n", trial, n0, n1, cp[nslice]); ok = 0; }
  for (long q = 0; q <= nslice && ok; q++)
    if (o1[q] != bw[q] || o2[q] != cp[q] || o3[q] != bb[q]) { printf("trial %d: offsets of slice %ld differ from the count\n", trial, q); ok = 0; }
  for (int which = 0; which < 3 && ok; which++) {                 /* each output alone */
    long *only = longs(nslice + 1);
    long const n = jur_param_layout(nslice, wptr, nr, rowptr, rowptr_b, sid, which == 0 ? only : NULL, which == 1 ? only : NULL, which == 2 ? only : NULL);
    long const *want = which == 0 ? bw : which == 1 ? cp : bb;
    if (n != n0 || memcmp(only, want, sizeof(long) * (size_t)(nslice + 1))) { printf("trial %d: output %d alone differs\n", trial, which); ok = 0; }
    free(only);
  }
  /* the tile map */
  if (ok) {
    long const nt = jur_param_maps(nslice, wptr, bw, NULL);
    int *cmap = (int *)malloc(sizeof(int) * 3 * (size_t)(nt ? nt : 1));
    unsigned char *seen = (unsigned char *)calloc((size_t)(cp[nslice] ? cp[nslice] : 1), 1);
    if (jur_param_maps(nslice, wptr, bw, cmap) != nt) { printf("trial %d: the tile map counts differently when it writes\n", trial); ok = 0; }
    for (long t = 0; t < nt && ok; t++) {
      long const q = cmap[3 * t], i0 = cmap[3 * t + 1], j0 = cmap[3 * t + 2], x = bw[q + 1] - bw[q];
      if (q < 0 || q >= nslice || i0 % JUR_PARAM_TILE || j0 % JUR_PARAM_TILE || i0 >= w[q] || j0 >= x) { printf("trial %d: tile %ld is misplaced\n", trial, t); ok = 0; break; }
      if (t > 0 && (cmap[3 * t - 3] > q)) { printf("trial %d: the tiles do not ascend by slice\n", trial); ok = 0; }
      for (long i = i0; i < i0 + JUR_PARAM_TILE && i < w[q]; i++)
        for (long j = j0; j < j0 + JUR_PARAM_TILE && j < x; j++) seen[cp[q] + i * x + j]++;
    }
    for (long e = 0; e < cp[nslice] && ok; e++) if (seen[e] != 1) { printf("trial %d: entry %ld of C is met %d times\n", trial, e, seen[e]); ok = 0; }
    free(cmap); free(seen);
  }
  /* bwptr and the values: accepted as they are, then one planted fault each */
  if (ok && jur_param_check_bwptr("who", nslice, bw, o1)) { printf("trial %d: a right bwptr is refused: %s\n", trial, g_msg); ok = 0; }
  if (ok) {
    int const nvar = (int)(rnd() % 4), ncov = (int)(rnd() % 3);
    size_t const nbw = (size_t)bw[nslice], nbb = (size_t)bb[nslice];
    double *var = (double *)malloc(sizeof(double) * ((size_t)nvar * nbw > 0 ? (size_t)nvar * nbw : 1));
    double *cov = (double *)malloc(sizeof(double) * ((size_t)ncov * nbb > 0 ? (size_t)ncov * nbb : 1));
    for (size_t e = 0; e < (size_t)nvar * nbw; e++) var[e] = (double)(rnd() % 100) / 10;
    for (int c = 0; c < ncov; c++)
      for (long q = 0; q < nslice; q++) {
        long const x = bw[q + 1] - bw[q];
        for (long j = 0; j < x; j++)
          for (long l = 0; l < x; l++)
            cov[(size_t)c * nbb + (size_t)bb[q] + (size_t)(j * x + l)] = l > j ? NAN : l == j ? 1. + (double)(rnd() % 10) : -0.25;   /* (above the diagonal: never read) */
      }
    jur_param_in_t in = {nvar, ncov, var, cov};
    double sig;
    jur_param_out_t out = {NULL, &sig};
    if (jur_param_check_args("who", &in, &out) || jur_param_check_values("who", nslice, bw, bb, &in)) { printf("trial %d: right values are refused: %s\n", trial, g_msg); ok = 0; }
    long q = -1;
    for (long t = 0; t < nslice; t++) if (bw[t + 1] - bw[t] > 1) q = t;   /* a slice with two parameters or more */
    if (ok && q >= 0 && nvar > 0) {
      size_t const at = (size_t)(nvar - 1) * nbw + (size_t)bw[q] + 1;
      double const keep = var[at];
      var[at] = -3.;
      snprintf(words, sizeof words, "who: the variance of component %d, slice %ld, element 1 is -3: negative or not finite", nvar - 1, q);
      ok = ok && refused(jur_param_check_values("who", nslice, bw, bb, &in), words, "a negative variance");
      var[at] = INFINITY;
      snprintf(words, sizeof words, "who: the variance of component %d, slice %ld, element 1 is inf: negative or not finite", nvar - 1, q);
      ok = ok && refused(jur_param_check_values("who", nslice, bw, bb, &in), words, "an infinite variance");
      var[at] = keep;
    }
    if (ok && q >= 0 && ncov > 0) {
      long const x = bw[q + 1] - bw[q];
      size_t const base = (size_t)(ncov - 1) * nbb + (size_t)bb[q];
      cov[base + (size_t)x] = INFINITY;                           /* element (1, 0) */
      snprintf(words, sizeof words, "who: cov of component %d, slice %ld, element (1, 0) is inf: not finite", nvar + ncov - 1, q);
      ok = ok && refused(jur_param_check_values("who", nslice, bw, bb, &in), words, "an infinite entry of cov");
      cov[base + (size_t)x] = -0.25;
      cov[base + (size_t)x + 1] = -2.;                            /* element (1, 1) */
      snprintf(words, sizeof words, "who: the diagonal of cov of component %d, slice %ld, element 1 is -2: negative", nvar + ncov - 1, q);
      ok = ok && refused(jur_param_check_values("who", nslice, bw, bb, &in), words, "a negative diagonal of cov");
    }
    if (ok && q >= 0) {
      long const x = bw[q + 1] - bw[q];
      for (long t = q + 1; t <= nslice; t++) o1[t]++;
      snprintf(words, sizeof words, "who: bwptr gives slice %ld %ld columns, its rays have %ld in rowptr_b", q, x + 1, x);
      ok = ok && refused(jur_param_check_bwptr("who", nslice, o1, bw), words, "a bwptr that disagrees");
      o1[q + 1] = o1[q] - 1;
      snprintf(words, sizeof words, "who: bwptr is not an ascending running sum of widths from 0 (slice %ld)", q);
      ok = ok && refused(jur_param_check_bwptr("who", nslice, o1, bw), words, "a bwptr that descends");
    }
    in.nvar = 5; in.ncov = 4;
    ok = ok && refused(jur_param_check_args("who", &in, &out), "who: nvar = 5, ncov = 4: 0 to 8 components per call", "nine components");
    in.nvar = 1; in.ncov = 0; out.sigma_param = NULL;
    ok = ok && refused(jur_param_check_args("who", &in, &out), "who: null argument (sigma_param) with nvar + ncov = 1", "no sigma_param");
    ok = ok && refused(jur_param_check_args("who", NULL, &out), "who: null argument (in)", "no in");
    free(var); free(cov);
  }
  /* the layout refusals, the outputs untouched */
  for (long q = 0; q <= nslice; q++) o1[q] = o2[q] = o3[q] = SENT;
  if (ok) {
    long two[2] = {-1, -1};                                       /* two rays of one slice */
    for (long r = 0; r < nr && two[1] < 0; r++)
      for (long r2 = r + 1; r2 < nr && two[1] < 0; r2++)
        if (sid[r] >= 0 && sid[r] == sid[r2]) { two[0] = r; two[1] = r2; }
    if (two[1] >= 0) {
      long *rb = longs(nr + 1);
      memcpy(rb, rowptr_b, sizeof(long) * (size_t)(nr + 1));
      long first = two[0];
      for (long r = 0; r < two[0]; r++) if (sid[r] == sid[two[0]]) { first = r; break; }
      long second = -1;                                           /* the first ray of that slice after `first` */
      for (long r = first + 1; r < nr; r++) if (sid[r] == sid[first]) { second = r; break; }
      for (long r = second + 1; r <= nr; r++) rb[r]++;
      snprintf(words, sizeof words, "jur_param_layout: rays %ld and %ld of slice %d have %ld and %ld columns in rowptr_b", first, second,
               sid[first], wb[sid[first]], wb[sid[first]] + 1);
      ok = ok && refused(jur_param_layout(nslice, wptr, nr, rowptr, rb, sid, o1, o2, o3), words, "two widths in one slice");
      free(rb);
    }
    if (nr > 0) {
      long const r = (long)(rnd() % (unsigned long long)nr);
      long *rb = longs(nr + 1);
      memcpy(rb, rowptr_b, sizeof(long) * (size_t)(nr + 1));
      /* (the rays before r are as they were, so none of them is refused first) */
      for (long t = r + 1; t <= nr; t++) rb[t] -= (rb[r + 1] - rb[r]) + 1;
      snprintf(words, sizeof words, "jur_param_layout: rowptr_b is not ascending at ray %ld", r);
      ok = ok && refused(jur_param_layout(nslice, wptr, nr, rowptr, rb, sid, o1, o2, o3), words, "a descending rowptr_b");
      rb[0] = 1;
      ok = ok && refused(jur_param_layout(nslice, wptr, nr, rowptr, rb, sid, o1, o2, o3), "jur_param_layout: rowptr_b does not start at 0", "rowptr_b from 1");
      free(rb);
      long at = -1;
      for (long t = 0; t < nr; t++) if (sid[t] >= 0) { at = t; break; }
      if (at >= 0) {
        long *rp = longs(nr + 1);
        memcpy(rp, rowptr, sizeof(long) * (size_t)(nr + 1));
        for (long t = at + 1; t <= nr; t++) rp[t]++;
        snprintf(words, sizeof words, "jur_param_layout: the block of ray %ld has %ld columns, its slice %d has %ld elements", at, w[sid[at]] + 1, sid[at], w[sid[at]]);
        ok = ok && refused(jur_param_layout(nslice, wptr, nr, rp, rowptr_b, sid, o1, o2, o3), words, "a ray wider than its slice");
        free(rp);
        int const keep = sid[at];
        sid[at] = (int)nslice;
        snprintf(words, sizeof words, "jur_param_layout: sid of ray %ld is %ld: outside -1..%ld", at, nslice, nslice - 1);
        ok = ok && refused(jur_param_layout(nslice, wptr, nr, rowptr, rowptr_b, sid, o1, o2, o3), words, "a slice that does not exist");
        sid[at] = keep;
      }
    }
    long const last = wptr[nslice];
    wptr[nslice] = wptr[nslice - 1] - 1;
    snprintf(words, sizeof words, "jur_param_layout: wptr is not an ascending running sum of widths from 0 (slice %ld)", nslice - 1);
    ok = ok && refused(jur_param_layout(nslice, wptr, nr, rowptr, rowptr_b, sid, o1, o2, o3), words, "a descending wptr");
    wptr[nslice] = last;
    ok = ok && refused(jur_param_layout(nslice, wptr, nr, rowptr, NULL, sid, o1, o2, o3), "jur_param_layout: null argument", "no rowptr_b");
    ok = ok && refused(jur_param_layout(-1, wptr, nr, rowptr, rowptr_b, sid, o1, o2, o3), "jur_param_layout: bad arguments", "a negative nslice");
    for (long q = 0; q <= nslice && ok; q++)
      if (o1[q] != SENT || o2[q] != SENT || o3[q] != SENT) { printf("trial %d: a refused layout wrote its outputs\n", trial); ok = 0; }
  }
  free(w); free(wb); free(wptr); free(used); free(sid); free(rowptr); free(rowptr_b); free(bw); free(cp); free(bb); free(o1); free(o2); free(o3);
  return ok;
}

int main(void) {
  int bad = 0;
  for (int trial = 0; trial < 400; trial++) bad += !check_scene(trial);
  /* nothing at all: one entry per array */
  long zero[1] = {0}, o[3] = {SENT, SENT, SENT};
  if (jur_param_layout(0, zero, 0, zero, zero, NULL, &o[0], &o[1], &o[2]) != 0 || o[0] || o[1] || o[2]) { printf("the empty layout: %s\n", g_msg); bad++; }
  if (jur_param_maps(0, zero, zero, NULL) != 0) { printf("the empty tile map\n"); bad++; }
  printf(bad ? "check_param_host: %d scenes FAILED\n" : "check_param_host: 400 scenes ok\n", bad);
  return bad ? 1 : 0;
}
