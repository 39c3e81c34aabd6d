/* Stand-alone check of the host function behind every atmosphere upload under IP 2 (jur_track.c: jur_track_rows,
 * jur_track_profiles), meant for a sanitizer build on the CPU; no GPU, no library:
 *
 *   gcc -std=gnu99 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=undefined -D__HIP_PLATFORM_AMD__ \
 *       -I/opt/rocm/include -Iinclude -Ijurassic-gpu_amd/csrc -DJUR_ND=100 -DJUR_NG=30 \
 *       -o check_track_host tools/check_track_host.c jurassic-gpu_amd/csrc/jur_track.c -lm && ./check_track_host
 *
 * 2000 seeded atmospheres of 1 .. 60 points in 1 .. 4 time blocks of 1 .. 5 profiles of 1 .. 9 levels (profiles of one
 * level and steps of more than 10 degrees among them), every row and every output malloc'ed to its exact size -- n points,
 * n / 2 + 1 profiles -- so that a read or write beyond it is an error of the sanitizer.  Checked per atmosphere against a
 * direct count: the number of profiles or the refusal and its words, first, len, block_of, dir, prof_of, x1 finite and
 * on the sphere; the outputs behind the last profile untouched; every output NULL in turn. */
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

#define SENT (-77)

static int check_one(int trial) {
  /* plan: blocks of profiles of levels */
  int plen[32], pblock[32], pdir[32], np_ = 0, n = 0, expect_lone = 0, expect_far = 0;
  double plat[32], plon[32];
  int const nblock = 1 + (int)(rnd() % 4);
  for (int b = 0; b < nblock; b++) {
    int const nprof = 1 + (int)(rnd() % 5);
    double lat = -40.0 + (double)(rnd() % 80);
    for (int k = 0; k < nprof; k++) {
      plen[np_] = 1 + (int)(rnd() % 9);
      if (rnd() % 4) plen[np_] += 1;                       /* most profiles have two levels or more */
      pblock[np_] = b;
      pdir[np_] = (int)(rnd() % 3) - 1;
      lat += (rnd() % 12 == 0) ? 10.5 : 0.5 + (double)(rnd() % 9);
      plat[np_] = lat;
      plon[np_] = (double)(rnd() % 360) - 180.0;
      n += plen[np_];
      np_++;
    }
  }
  double *time = malloc(sizeof(double) * n), *z = malloc(sizeof(double) * n), *lon = malloc(sizeof(double) * n), *lat = malloc(sizeof(double) * n);
  int at = 0, first_bad = -1, bad_kind = 0;
  for (int p = 0; p < np_; p++) {
    for (int l = 0; l < plen[p]; l++, at++) {
      time[at] = 100.0 * pblock[p];
      lon[at] = plon[p];
      lat[at] = plat[p];
      z[at] = (pdir[p] > 0) ? l : (pdir[p] < 0) ? 100.0 - l : (l % 2 ? 3.0 : 5.0);
    }
    /* the scan refuses at the first profile that is wrong, a profile of one level before its distance */
    if (first_bad < 0) {
      if (plen[p] <= 1) { first_bad = p; bad_kind = 1; }
      else if (p > 0 && pblock[p] == pblock[p - 1] && fabs(plat[p - 1] - plat[p]) > 10) { first_bad = p; bad_kind = 2; }
    }
  }
  expect_lone = bad_kind == 1; expect_far = bad_kind == 2;
  int const cap = n / 2 + 1;
  int fails = 0;
  for (int variant = 0; variant < 7; variant++) {          /* 0: all outputs, 1 .. 6: one of them NULL */
    int *first = malloc(sizeof(int) * cap), *len = malloc(sizeof(int) * cap), *block = malloc(sizeof(int) * cap), *dir = malloc(sizeof(int) * cap);
    int *prof = malloc(sizeof(int) * n);
    double (*x1)[3] = malloc(sizeof(double) * 3 * cap);
    for (int i = 0; i < cap; i++) { first[i] = len[i] = block[i] = dir[i] = SENT; x1[i][0] = x1[i][1] = x1[i][2] = SENT; }
    for (int i = 0; i < n; i++) prof[i] = SENT;
    g_msg[0] = 0;
    long const rc = jur_track_rows(n, time, z, lon, lat, variant == 1 ? NULL : first, variant == 2 ? NULL : len, variant == 3 ? NULL : x1,
                                   variant == 4 ? NULL : block, variant == 5 ? NULL : dir, variant == 6 ? NULL : prof);
    if (expect_lone || expect_far) {
      char const *words = expect_lone ? "Cannot identify profiles. Check ordering of data points!" : "Distance of profiles is too large!";
      if (rc != JUR_EINVAL || strcmp(g_msg, words)) { printf("trial %d variant %d: expected \"%s\", got %ld: %s\n", trial, variant, words, rc, g_msg); fails++; }
      for (int i = first_bad; i < cap; i++)
        if (first[i] != SENT || len[i] != SENT || block[i] != SENT || dir[i] != SENT || x1[i][0] != SENT) { printf("trial %d: output %d written by a refused call\n", trial, i); fails++; break; }
    } else {
      if (rc != np_) { printf("trial %d variant %d: %ld profiles, expected %d (%s)\n", trial, variant, rc, np_, g_msg); fails++; }
      else {
        int a0 = 0;
        for (int p = 0; p < np_; p++) {
          int const want_dir = plen[p] == 2 && pdir[p] == 0 ? -1 : pdir[p];     /* two levels 5, 3 descend */
          if ((variant != 1 && first[p] != a0) || (variant != 2 && len[p] != plen[p]) || (variant != 4 && block[p] != pblock[p]) ||
              (variant != 5 && dir[p] != want_dir)) { printf("trial %d variant %d: profile %d wrong\n", trial, variant, p); fails++; break; }
          if (variant != 3) {
            double const r = sqrt(x1[p][0] * x1[p][0] + x1[p][1] * x1[p][1] + x1[p][2] * x1[p][2]);
            if (!(fabs(r - JUR_RE) < 1e-9 * JUR_RE)) { printf("trial %d: x1 of profile %d off the sphere (%g)\n", trial, p, r); fails++; break; }
          }
          if (variant != 6) for (int l = 0; l < plen[p]; l++) if (prof[a0 + l] != p) { printf("trial %d: prof_of[%d] wrong\n", trial, a0 + l); fails++; break; }
          a0 += plen[p];
        }
        for (int i = np_; i < cap; i++)
          if (first[i] != SENT || len[i] != SENT || block[i] != SENT || dir[i] != SENT || x1[i][0] != SENT) { printf("trial %d: output %d beyond the last profile written\n", trial, i); fails++; break; }
      }
    }
    free(first); free(len); free(block); free(dir); free(prof); free(x1);
  }
  free(time); free(z); free(lon); free(lat);
  return fails;
}

int main(void) {
  int fails = 0, refused = 0;
  for (int t = 0; t < 2000; t++) { fails += check_one(t); refused += g_msg[0] != 0; }
  if (jur_track_rows(0, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL) != JUR_EINVAL) { printf("an empty atmosphere was accepted\n"); fails++; }
  printf("check_track_host: 2000 atmospheres, %d refused, %d failures\n", refused, fails);
  return fails ? 1 : 0;
}
