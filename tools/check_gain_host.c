/* Stand-alone check of the host arithmetic of the gain entries (jur_scene.c: jur_gain_maps, jur_gain_check_args,
 * jur_gain_check_layout, jur_gain_check_var, jur_error_components, with jur_scene_rays_by_slice for the row lists), meant
 * for a sanitizer build on the CPU; no GPU, no library:
 *
 *   gcc -std=gnu99 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=undefined -D__HIP_PLATFORM_AMD__ \
 *       -I/opt/rocm/include -Iinclude -Ijurassic-gpu_amd/csrc -DJUR_ND=100 -DJUR_NG=30 \
 *       -o check_gain_host tools/check_gain_host.c jurassic-gpu_amd/csrc/jur_scene.c -lm && ./check_gain_host
 *
 * Seeded ragged layouts: widths and numbers of measurement rows per slice 1 below, at and above 16, 64 and 256 among
 * others, slices without rays and of width 0, rays without a slice, rays of the slices interleaved; every array malloc'ed
 * to its exact size so that a read or write beyond it is an error of the sanitizer.  Checked per layout: the tile map
 * covers every (measurement, element) pair of every slice exactly once, in order, and counts what its first call counted;
 * the row of every measurement -- as jur_scene_gain_kernel finds it from srays, sptr and koff -- is the row of that ray
 * and channel in the blocks, every row of the blocks is met once, and the rows of a slice ascend; the layout and variance
 * checks accept what is right and refuse one planted fault by its words, reading the variances of live measurements only
 * (the others hold NaN); jur_error_components against its rule written out here, NaN, infinities and zeros among y. */
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
static double uni(double a, double b) { return a + (b - a) * (double)(rnd() % 1000001) / 1e6; }
static int same(double a, double b) { return 0 == memcmp(&a, &b, sizeof a); }

static int refused(int rc, char const *words, char const *what) {
  if (rc == JUR_EINVAL && strstr(g_msg, words)) return 1;
  printf("%s: expected JUR_EINVAL with \"%s\", got %d: %s\n", what, words, rc, g_msg);
  return 0;
}

static long const EDGES[] = {1, 2, 15, 16, 17, 63, 64, 65, 100, 255, 256, 257, 300};
#define NEDGE ((long)(sizeof EDGES / sizeof EDGES[0]))

static int check_layout(int trial) {
  long const nslice = 1 + (long)(rnd() % 5);
  int const nd = 1 + (int)(rnd() % 4);
  long *wptr = (long *)malloc(sizeof(long) * (size_t)(nslice + 1)), *nrays = (long *)malloc(sizeof(long) * (size_t)nslice);
  long nr = 0;
  wptr[0] = 0;
  for (long q = 0; q < nslice; q++) {
    long const w = (rnd() % 9 == 0) ? 0 : EDGES[rnd() % NEDGE];
    long rows = (rnd() % 9 == 0) ? 0 : EDGES[rnd() % NEDGE];       /* measurement rows wanted: rays = ceil(rows / nd) */
    wptr[q + 1] = wptr[q] + w;
    nrays[q] = w == 0 ? 0 : (rows + nd - 1) / nd;                  /* (a ray of a slice of width 0 would have no slice) */
    nr += nrays[q];
  }
  long const nfree = (long)(rnd() % 3);                            /* rays without a slice */
  nr += nfree;
  int *sid = (int *)malloc(sizeof(int) * (size_t)(nr ? nr : 1));
  {                                                                /* the rays of the slices interleaved: a shuffle */
    long at = 0;
    for (long q = 0; q < nslice; q++) for (long i = 0; i < nrays[q]; i++) sid[at++] = (int)q;
    for (long i = 0; i < nfree; i++) sid[at++] = -1;
    for (long i = nr - 1; i > 0; i--) { long const j = (long)(rnd() % (unsigned long long)(i + 1)); int const t = sid[i]; sid[i] = sid[j]; sid[j] = t; }
  }
  long *rowptr = (long *)malloc(sizeof(long) * (size_t)(nr + 1)), *koff = (long *)malloc(sizeof(long) * (size_t)(nr ? nr : 1));
  rowptr[0] = 0;
  for (long r = 0; r < nr; r++) {
    rowptr[r + 1] = rowptr[r] + (sid[r] < 0 ? 0 : wptr[sid[r] + 1] - wptr[sid[r]]);
    koff[r] = rowptr[r] * nd;
  }
  long *sptr = (long *)malloc(sizeof(long) * (size_t)(nslice + 1));
  int *srays = (int *)malloc(sizeof(int) * (size_t)(nr ? nr : 1));
  int ok = 1;
  long const nlist = jur_scene_rays_by_slice(nr, nslice, sid, sptr, srays);
  if (nlist != nr - nfree) { printf("trial %d: %ld rays in the lists, %ld have a slice\n", trial, nlist, nr - nfree); ok = 0; }
  if (jur_gain_check_layout("t", nslice, wptr, nr, rowptr, sid) != JUR_OK) { printf("trial %d: a good layout refused: %s\n", trial, g_msg); ok = 0; }

  /* the tile map: counted, then written into an array of exactly that size */
  long const ntile = jur_gain_maps(nslice, wptr, sptr, nd, NULL);
  int *gmap = (int *)malloc(sizeof(int) * 3 * (size_t)(ntile ? ntile : 1));
  if (jur_gain_maps(nslice, wptr, sptr, nd, gmap) != ntile) { printf("trial %d: the two calls of jur_gain_maps disagree\n", trial); ok = 0; }
  long t = 0;
  for (long q = 0; q < nslice && ok; q++) {
    long const w = wptr[q + 1] - wptr[q], M = (sptr[q + 1] - sptr[q]) * nd;
    for (long m0 = 0; m0 < M && ok; m0 += JUR_GAIN_TILE)
      for (long i0 = 0; i0 < w; i0 += JUR_GAIN_TILE, t++)
        if (t >= ntile || gmap[3 * t] != q || gmap[3 * t + 1] != m0 || gmap[3 * t + 2] != i0) {
          printf("trial %d: tile %ld is not (%ld, %ld, %ld)\n", trial, t, q, m0, i0); ok = 0; break;
        }
  }
  if (ok && t != ntile) { printf("trial %d: %ld tiles expected, %ld in the map\n", trial, t, ntile); ok = 0; }

  /* the rows: measurement m of slice q is channel m % nd of ray srays[sptr[q] + m / nd], its row koff[ray] + channel * w;
   * every row of the blocks (rowptr[nr] * nd doubles, rows of w doubles) is met exactly once */
  size_t const nk = (size_t)rowptr[nr] * (size_t)nd;
  unsigned char *met = (unsigned char *)calloc(nk ? nk : 1, 1);
  for (long q = 0; q < nslice && ok; q++) {
    long const w = wptr[q + 1] - wptr[q], M = (sptr[q + 1] - sptr[q]) * nd;
    long last = -1;
    for (long m = 0; m < M && ok; m++) {
      long const r = srays[sptr[q] + m / nd], id = m % nd, at = koff[r] + id * w;
      if (sid[r] != q || at <= last || at < 0 || (size_t)(at + w) > nk) { printf("trial %d: slice %ld, measurement %ld: a bad row\n", trial, q, m); ok = 0; break; }
      last = at;
      for (long i = 0; i < w; i++) met[at + i]++;
    }
  }
  for (size_t i = 0; i < nk && ok; i++) if (met[i] != 1) { printf("trial %d: double %zu of the blocks is met %d times\n", trial, i, met[i]); ok = 0; }

  /* the variances: NaN wherever the measurement is not live, one fault planted on a live one */
  size_t const nrd = (size_t)nr * (size_t)nd;
  int const ncomp = 1 + (int)(rnd() % JUR_GAIN_MAXCOMP);
  unsigned char *live = (unsigned char *)malloc(nrd ? nrd : 1);
  double *var = (double *)malloc(sizeof(double) * (nrd ? nrd * (size_t)ncomp : 1));
  long nlive = 0;
  for (size_t i = 0; i < nrd; i++) { live[i] = sid[i / (size_t)nd] >= 0 && rnd() % 4 != 0; nlive += live[i]; }
  for (size_t i = 0; i < nrd * (size_t)ncomp; i++) var[i] = live[i % nrd] ? (rnd() % 5 == 0 ? 0. : uni(0., 3.)) : NAN;
  if (ok && jur_gain_check_var("t", ncomp, nr, nd, var, live) != JUR_OK) { printf("trial %d: good variances refused: %s\n", trial, g_msg); ok = 0; }
  if (ok && nlive > 0) {
    size_t at = rnd() % nrd;
    while (!live[at]) at = (at + 1) % nrd;
    int const c = (int)(rnd() % (unsigned)ncomp);
    double const bad[3] = {-1., NAN, INFINITY};
    char words[96];
    snprintf(words, sizeof words, "component %d, ray %ld, channel %d is", c, (long)(at / (size_t)nd), (int)(at % (size_t)nd));
    for (int b = 0; b < 3 && ok; b++) {
      double const keep = var[(size_t)c * nrd + at];
      var[(size_t)c * nrd + at] = bad[b];
      ok = refused(jur_gain_check_var("t", ncomp, nr, nd, var, live), words, "a bad variance");
      var[(size_t)c * nrd + at] = keep;
    }
  }
  /* a planted fault in the layout: a slice out of range, a block of the wrong width */
  if (ok && nr > 0) {
    long const r = (long)(rnd() % (unsigned long long)nr);
    int const keep = sid[r];
    sid[r] = (int)nslice;
    ok = refused(jur_gain_check_layout("t", nslice, wptr, nr, rowptr, sid), "sid of ray", "a slice out of range");
    sid[r] = keep;
    if (ok) {
      for (long i = r + 1; i <= nr; i++) rowptr[i]++;
      ok = refused(jur_gain_check_layout("t", nslice, wptr, nr, rowptr, sid), "columns, its slice", "a block of the wrong width");
    }
  }
  free(wptr); free(nrays); free(sid); free(rowptr); free(koff); free(sptr); free(srays); free(gmap); free(met); free(live); free(var);
  return ok;
}

static int check_components(int trial) {
  int const nd = 1 + (int)(rnd() % 5);
  long const nr = (long)(rnd() % 40);
  size_t const nrd = (size_t)nr * (size_t)nd;
  double *y = (double *)malloc(sizeof(double) * (nrd ? nrd : 1)), *en = (double *)malloc(sizeof(double) * (size_t)nd),
         *ef = (double *)malloc(sizeof(double) * (size_t)nd), *var = (double *)malloc(sizeof(double) * (nrd ? 2 * nrd : 1)),
         *weight = (double *)malloc(sizeof(double) * (nrd ? nrd : 1));
  double const odd[6] = {NAN, INFINITY, -INFINITY, 0., -0., 1e200};
  for (size_t i = 0; i < nrd; i++) y[i] = rnd() % 6 == 0 ? odd[rnd() % 6] : uni(-1., 4.);
  for (int id = 0; id < nd; id++) { en[id] = rnd() % 4 == 0 ? 0. : uni(0., 0.5); ef[id] = rnd() % 4 == 0 ? 0. : uni(0., 3.); }
  int ok = 1;
  if (jur_error_components(nd, nr, y, en, ef, var, weight) != JUR_OK) { printf("components %d: refused: %s\n", trial, g_msg); ok = 0; }
  for (size_t i = 0; i < nrd && ok; i++) {
    int const id = (int)(i % (size_t)nd);
    double const vn = en[id] * en[id], f = ef[id] / 100 * y[i], vf = f * f, sum = vn + vf;
    int const good = sum > 0 && isfinite(sum);
    if (!same(var[i], good ? vn : 0.) || !same(var[nrd + i], good ? vf : 0.) || !same(weight[i], good ? 1 / sum : 0.)) {
      printf("components %d: measurement %zu (y = %g) against the rule\n", trial, i, y[i]); ok = 0;
    }
  }
  int const id = (int)(rnd() % (unsigned)nd);
  double const bad[3] = {-0.5, NAN, INFINITY};
  for (int b = 0; b < 3 && ok; b++) {
    double keep = en[id];
    en[id] = bad[b];
    ok = refused(jur_error_components(nd, nr, y, en, ef, var, weight), "err_noise of channel", "a bad err_noise");
    en[id] = keep; keep = ef[id]; ef[id] = bad[b];
    if (ok) ok = refused(jur_error_components(nd, nr, y, en, ef, var, weight), "err_formod of channel", "a bad err_formod");
    ef[id] = keep;
  }
  free(y); free(en); free(ef); free(var); free(weight);
  return ok;
}

int main(void) {
  int ok = 1;
  jur_gain_in_t in = {0, NULL};
  jur_gain_out_t out = {NULL, NULL};
  double one = 1.;
  ok &= jur_gain_check_args("t", &in, &out) == JUR_OK;             /* the gain only */
  ok &= refused(jur_gain_check_args("t", NULL, &out), "null argument (in)", "in == NULL");
  ok &= refused(jur_gain_check_args("t", &in, NULL), "null argument (out)", "out == NULL");
  in.ncomp = -1; ok &= refused(jur_gain_check_args("t", &in, &out), "ncomp = -1: 0 to 8", "ncomp -1");
  in.ncomp = 9; ok &= refused(jur_gain_check_args("t", &in, &out), "ncomp = 9: 0 to 8", "ncomp 9");
  in.ncomp = 2; in.var = &one; ok &= refused(jur_gain_check_args("t", &in, &out), "null argument (sigma_comp)", "sigma_comp == NULL");
  out.sigma_comp = &one; in.var = NULL; ok &= refused(jur_gain_check_args("t", &in, &out), "null argument (var)", "var == NULL");
  in.var = &one; ok &= jur_gain_check_args("t", &in, &out) == JUR_OK;
  int ntrial = 0;
  for (int t = 0; t < 600 && ok; t++, ntrial++) ok &= check_layout(t);
  for (int t = 0; t < 300 && ok; t++) ok &= check_components(t);
  printf(ok ? "check_gain_host: %d layouts and 300 sets of error components passed\n" : "check_gain_host: FAILED after %d layouts\n", ntrial);
  return ok ? 0 : 1;
}
