/* Stand-alone check of the map from the rays that remain to the blocks a Jacobian iteration left (jur_scene.c:
 * jur_scene_recomp_offsets) and of the forward-only passes of a reuse iteration against the reserve
 * (jur_trial_passes(n, 1, cap) within jur_scene_pass_reserve), meant for a sanitizer build on the CPU; no GPU, no library:
 *
 *   gcc -std=gnu99 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=undefined -D__HIP_PLATFORM_AMD__ \
 *       -I/opt/rocm/include -Iinclude -Ijurassic-gpu_amd/csrc -DJUR_ND=100 -DJUR_NG=30 \
 *       -o check_recomp_host tools/check_recomp_host.c jurassic-gpu_amd/csrc/jur_scene.c -lm && ./check_recomp_host
 *
 * Seeded scenes of up to 40 rays in scans of 1 ... 6 (one time stamp, one slice, one width each; some rays without state
 * elements) in up to 7 slices, a seeded set of slices that had ended at the Jacobian iteration and a seeded larger set that
 * has ended now, every array malloc'ed to its exact size so that a read or write beyond it is an error of the sanitizer.
 * Every offset must be the one a search over the rays written then gives, every block must lie inside what was written,
 * and a slice that is active now but was not then must be refused. */
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

int main(void) {
  long maps = 0, refused = 0, cuts = 0;
  for (int trial = 0; trial < 4000; trial++) {
    long const nr = (long)(rnd() % 41);
    int const ns = 1 + (int)(rnd() % 7), nd = 1 + (int)(rnd() % 4), with_time = (int)(rnd() % 2), ntrial = 1 + (int)(rnd() % 8);
    size_t const n1 = (size_t)(nr ? nr : 1);
    long *rp = (long *)malloc(sizeof(long) * (size_t)(nr + 1));
    int *sid = (int *)malloc(sizeof(int) * n1);
    double *time = (double *)malloc(sizeof(double) * n1);
    long *width = (long *)malloc(sizeof(long) * (size_t)ns);
    int *then = (int *)malloc(sizeof(int) * (size_t)ns), *now = (int *)malloc(sizeof(int) * (size_t)ns);
    if (!rp || !sid || !time || !width || !then || !now) return 2;
    for (int q = 0; q < ns; q++) {
      width[q] = 1 + (long)(rnd() % 9);
      then[q] = rnd() % 4 == 0 ? 1 + (int)(rnd() % 3) : JUR_RET_ACTIVE;          /* ended in some way, or active */
      now[q] = (then[q] != JUR_RET_ACTIVE || rnd() % 3 == 0) ? 1 + (int)(rnd() % 3) : JUR_RET_ACTIVE;
    }
    rp[0] = 0;
    for (long r = 0, left = 0, q = 0, scan = 0; r < nr; r++, left--) {
      if (left == 0) { left = 1 + (long)(rnd() % 6); scan++; q = rnd() % 6 == 0 ? -1 : (long)(rnd() % (unsigned)ns); }
      time[r] = (double)scan; sid[r] = (int)q;
      rp[r + 1] = rp[r] + (q < 0 ? 0 : width[q]);
    }
    /* the rays that remain and, by a search, where the Jacobian iteration wrote their blocks */
    long m = 0, written = 0;
    for (long r = 0; r < nr; r++) {
      m += sid[r] >= 0 && now[sid[r]] == JUR_RET_ACTIVE;
      if (sid[r] >= 0 && then[sid[r]] == JUR_RET_ACTIVE) written += (rp[r + 1] - rp[r]) * nd;
    }
    long *koff = (long *)malloc(sizeof(long) * (size_t)(m ? m : 1));
    double *time2 = (double *)malloc(sizeof(double) * (size_t)(m ? m : 1));
    if (!koff || !time2) return 2;
    long const got = jur_scene_recomp_offsets(nr, rp, sid, then, now, nd, koff);
    if (got != m) { printf("trial %d: %ld rays mapped, %ld remain: %s\n", trial, got, m, g_msg); return 1; }
    for (long r = 0, i = 0; r < nr; r++) {
      if (sid[r] < 0 || now[sid[r]] != JUR_RET_ACTIVE) continue;
      long at = 0;
      for (long r2 = 0; r2 < r; r2++)
        if (sid[r2] >= 0 && then[sid[r2]] == JUR_RET_ACTIVE) at += (rp[r2 + 1] - rp[r2]) * nd;
      if (koff[i] != at || at + (rp[r + 1] - rp[r]) * nd > written) {
        printf("trial %d: block of ray %ld at %ld, the search says %ld of %ld doubles written\n", trial, r, koff[i], at, written);
        return 1;
      }
      time2[i++] = time[r];
    }
    maps++;
    /* a slice that is active now but had ended then: refused, naming it, with nothing written beyond the rays before it */
    for (int q = 0; q < ns; q++)
      if (then[q] != JUR_RET_ACTIVE) {
        int has = 0;
        for (long r = 0; r < nr; r++) has |= sid[r] == q;
        if (!has) continue;
        now[q] = JUR_RET_ACTIVE;
        long *small = (long *)malloc(sizeof(long) * (size_t)(m + 1));   /* (at most the rays that remain, and the first of the slice) */
        if (!small) return 2;
        long const rc = jur_scene_recomp_offsets(nr, rp, sid, then, now, nd, small);
        free(small);
        if (rc != JUR_EINVAL || !strstr(g_msg, "was not when the Jacobian was computed")) { printf("trial %d: slice %d not refused (%ld): %s\n", trial, q, rc, g_msg); return 1; }
        now[q] = then[q];
        refused++;
        break;
      }
    /* the forward-only passes of the rays that remain within the reserve of the call, for every cap */
    long *pass = (long *)malloc(sizeof(long) * (size_t)(m + 1));
    if (!pass) return 2;
    for (long cap = 1; cap <= rp[nr] + nr + 1; cap++) {
      long slots = -1, cols = -1, fmax = -1;
      if (jur_scene_pass_reserve(nr, rp, cap, ntrial, with_time ? time : NULL, &slots, &cols)) { printf("reserve refused: %s\n", g_msg); return 1; }
      long const np = jur_trial_passes(m, 1, cap, with_time ? time2 : NULL, pass, &fmax);
      if (np < 0 || pass[0] != 0 || pass[np] != m || fmax > slots) {
        printf("trial %d, cap %ld, ntrial %d: forward-only passes of %ld slots, %ld reserved\n", trial, cap, ntrial, fmax, slots);
        return 1;
      }
      cuts++;
    }
    free(pass); free(koff); free(time2); free(rp); free(sid); free(time); free(width); free(then); free(now);
  }
  printf("check_recomp_host: %ld maps agree with the search, %ld stale slices refused, %ld forward-only cuts within the reserve\n", maps, refused, cuts);
  return 0;
}
