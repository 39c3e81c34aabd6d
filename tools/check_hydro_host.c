/* Stand-alone check of the hydrostatic balance's host rule (jur_scene.c: jur_scene_hydrostatic, jur_scene_ray_slices),
 * meant for a sanitizer build on the CPU; no GPU, no library:
 *
 *   gcc -std=gnu99 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=undefined -D__HIP_PLATFORM_AMD__ \
 *       -I/opt/rocm/include -Iinclude -Ijurassic-gpu_amd/csrc -DJUR_ND=100 -DJUR_NG=30 \
 *       -o check_hydro_host tools/check_hydro_host.c jurassic-gpu_amd/csrc/jur_scene.c -lm && ./check_hydro_host
 *
 * Seeded atmospheres of 2 ... 12 profiles of 1 ... 40 levels, ascending and descending, with one time stamp each; the
 * segment lists malloc'ed to their exact size so that a read or write beyond them is an error of the sanitizer (the
 * atmosphere's own arrays are JUR_NP long: the balance must leave every point outside the segments, and everything but p,
 * bit for bit).  Checked per atmosphere: the ray slices of rays at every profile's time stamp are the profiles of two
 * levels or more, in the rays' order; a balance moves pressures, keeps the reference parcel's, and a second one returns the
 * same bytes; in place equals out of place; every refusal comes with its words. */
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

static int refused(int rc, char const *words, char const *what) {
  if (rc == JUR_EINVAL && strstr(g_msg, words)) return 1;
  printf("%s: expected JUR_EINVAL with \"%s\", got %d: %s\n", what, words, rc, g_msg);
  return 0;
}

int main(void) {
  ctl_t *ctl = (ctl_t *)calloc(1, sizeof(ctl_t));
  atm_t *atm = (atm_t *)calloc(1, sizeof(atm_t)), *out = (atm_t *)calloc(1, sizeof(atm_t)), *twice = (atm_t *)calloc(1, sizeof(atm_t));
  if (!ctl || !atm || !out || !twice) return 2;
  ctl->ng = 2; ctl->nd = 1; ctl->nw = 1;
  strcpy(ctl->emitter[0], "CO2"); strcpy(ctl->emitter[1], "H2O");
  long balanced = 0;
  for (int trial = 0; trial < 400; trial++) {
    int const npro = 2 + (int)(rnd() % 11);
    ctl->ctm_h2o = (int)(rnd() % 2);
    int *pfirst = (int *)malloc(sizeof(int) * (size_t)npro), *plen = (int *)malloc(sizeof(int) * (size_t)npro);
    double *time = (double *)malloc(sizeof(double) * (size_t)npro);
    if (!pfirst || !plen || !time) return 2;
    memset(atm, 0, sizeof *atm);
    int np = 0, nlive = 0;
    for (int k = 0; k < npro; k++) {
      /* (a profile of one level at either end would join its neighbour's slice: kept to the inner profiles) */
      int const n = (k == 0 || k == npro - 1) ? 2 + (int)(rnd() % 39) : 1 + (int)(rnd() % 40), down = (int)(rnd() % 2);
      double const z0 = uni(0, 10), dz = uni(0.3, 3.0), lon = uni(-180, 180), lat = uni(-90, 90);
      pfirst[k] = np; plen[k] = n; time[k] = 0.5 * k;
      for (int i = 0; i < n; i++, np++) {
        double const z = z0 + dz * (down ? n - 1 - i : i);
        atm->time[np] = time[k]; atm->z[np] = z; atm->lon[np] = lon; atm->lat[np] = lat;
        atm->p[np] = 1013.25 * exp(-z / uni(6.5, 7.5)); atm->t[np] = uni(180, 300);
        atm->q[0][np] = 370e-6; atm->q[1][np] = uni(1e-6, 2e-2); atm->k[0][np] = uni(0, 1e-4);
      }
      nlive += n >= 2;
    }
    atm->np = np;
    /* rays at every profile's time stamp, last profile first, each twice */
    long const nr = 2L * npro;
    double *rt = (double *)malloc(sizeof(double) * (size_t)nr);
    int *sfirst = (int *)malloc(sizeof(int) * (size_t)nr), *slen = (int *)malloc(sizeof(int) * (size_t)nr);
    if (!rt || !sfirst || !slen) return 2;
    for (long r = 0; r < nr; r++) rt[r] = time[npro - 1 - r / 2];
    long const ns = jur_scene_ray_slices(ctl, atm, nr, rt, sfirst, slen);
    if (ns != nlive || jur_scene_ray_slices(ctl, atm, nr, rt, NULL, NULL) != ns) { printf("trial %d: %ld ray slices, %d profiles of two levels or more: %s\n", trial, ns, nlive, g_msg); return 1; }
    for (long q = 0, k = npro - 1; q < ns; q++, k--) {
      while (plen[k] < 2) k--;
      if (sfirst[q] != pfirst[k] || slen[q] != plen[k]) { printf("trial %d: ray slice %ld is [%d, +%d), profile %ld [%d, +%d)\n", trial, q, sfirst[q], slen[q], k, pfirst[k], plen[k]); return 1; }
    }
    /* exact-size copies of the list for the balance */
    int *sf = (int *)malloc(sizeof(int) * (size_t)(ns ? ns : 1)), *sn = (int *)malloc(sizeof(int) * (size_t)(ns ? ns : 1));
    if (!sf || !sn) return 2;
    memcpy(sf, sfirst, sizeof(int) * (size_t)ns); memcpy(sn, slen, sizeof(int) * (size_t)ns);
    double const hydz = rnd() % 4 == 0 ? 0.0 : uni(0, 120);
    memcpy(out, atm, sizeof *atm);
    if (jur_scene_hydrostatic(ctl, hydz, atm, ns, sf, sn, out)) { printf("trial %d: refused: %s\n", trial, g_msg); return 1; }
    memcpy(twice, out, sizeof *out);
    if (jur_scene_hydrostatic(ctl, hydz, out, ns, sf, sn, twice) || memcmp(twice, out, sizeof *out)) { printf("trial %d: a second balance changes bytes\n", trial); return 1; }
    memcpy(twice, atm, sizeof *atm);
    if (jur_scene_hydrostatic(ctl, hydz, twice, ns, sf, sn, twice) || memcmp(twice, out, sizeof *out)) { printf("trial %d: in place differs\n", trial); return 1; }
    memcpy(twice, out, sizeof *out);
    memcpy(twice->p, atm->p, sizeof atm->p);
    if (memcmp(twice, atm, sizeof *atm)) { printf("trial %d: something other than p was written\n", trial); return 1; }
    for (int k = 0; k < npro; k++) {
      int same = 0, ipref = 0;
      for (int i = 0; i < plen[k]; i++) {
        same += out->p[pfirst[k] + i] == atm->p[pfirst[k] + i];
        if (fabs(atm->z[pfirst[k] + i] - hydz) < fabs(atm->z[pfirst[k] + ipref] - hydz)) ipref = i;
      }
      if (plen[k] < 2 ? same != plen[k] : (same != 1 || out->p[pfirst[k] + ipref] != atm->p[pfirst[k] + ipref])) {
        printf("trial %d, profile %d of %d levels: %d pressures kept, parcel %d\n", trial, k, plen[k], same, ipref);
        return 1;
      }
      balanced += plen[k] >= 2;
    }
    /* the refusals, on lists of their exact size */
    if (!refused(jur_scene_hydrostatic(ctl, -1.0, atm, ns, sf, sn, out), "negative or not finite", "hydz = -1")) return 1;
    if (!refused(jur_scene_hydrostatic(ctl, NAN, atm, ns, sf, sn, out), "negative or not finite", "hydz = NaN")) return 1;
    if (!refused(jur_scene_hydrostatic(ctl, INFINITY, atm, ns, sf, sn, out), "negative or not finite", "hydz = inf")) return 1;
    int const keep = sn[ns - 1];
    sn[ns - 1] = np - sf[ns - 1] + 1;
    if (!refused(jur_scene_hydrostatic(ctl, hydz, atm, ns, sf, sn, out), "lies outside", "a segment beyond np")) return 1;
    sn[ns - 1] = keep;
    sf[0] -= np + 1;
    if (!refused(jur_scene_hydrostatic(ctl, hydz, atm, ns, sf, sn, out), "lies outside", "a segment before 0")) return 1;
    sf[0] += np + 1;
    if (ns >= 2) {
      int const f = sf[1], l = sn[1];
      sf[1] = sf[0] + sn[0] - 1; sn[1] = 2;
      if (sf[1] + 2 <= np && !refused(jur_scene_hydrostatic(ctl, hydz, atm, ns, sf, sn, out), "share point", "two segments that overlap")) return 1;
      sf[1] = f; sn[1] = l;
    }
    free(pfirst); free(plen); free(time); free(rt); free(sfirst); free(slen); free(sf); free(sn);
  }
  printf("check_hydro_host: %ld profiles balanced, every refusal with its words\n", balanced);
  free(ctl); free(atm); free(out); free(twice);
  return 0;
}
