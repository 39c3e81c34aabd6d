/* Stand-alone check of the pass rules of the scene entries (jur_scene.c: jur_scene_passes, jur_trial_passes,
 * jur_scene_pass_reserve), meant for a sanitizer build on the CPU; no GPU, no library:
 *
 *   gcc -std=gnu99 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=undefined -D__HIP_PLATFORM_AMD__ \
 *       -I/opt/rocm/include -Iinclude -Ijurassic-gpu_amd/csrc -DJUR_ND=100 -DJUR_NG=30 \
 *       -o check_passes_host tools/check_passes_host.c jurassic-gpu_amd/csrc/jur_scene.c -lm && ./check_passes_host
 *
 * Seeded calls of up to 40 rays in scans of 1 ... 6 with widths 0 ... 9 and one wide ray, with and without time stamps,
 * every array malloc'ed to its exact size so that a read or write beyond it is an error of the sanitizer.  Every pass
 * of every cut, and of the cut of the rays that a seeded set of ended scans leaves, must fit the reserve. */
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
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

static int fits(char const *what, int trial, long cap, int ntrial, long nr, long const *rp, double const *time, long slots, long cols) {
  long *pass = (long *)malloc(sizeof(long) * (size_t)(nr + 1));
  long n1 = -1, k1 = -1, t1 = -1;
  if (!pass) return 0;
  long const np = jur_scene_passes(nr, rp, cap, time, pass, &n1, &k1);
  int ok = np >= 0 && pass[0] == 0 && pass[np] == nr;
  long const nt = jur_trial_passes(nr, ntrial, cap, time, pass, &t1);
  ok = ok && nt >= 0 && pass[0] == 0 && pass[nt] == nr;
  free(pass);
  if (!ok) { printf("trial %d, cap %ld, %s cut refused or out of step: %s\n", trial, cap, what, g_msg); return 0; }
  if (n1 > slots || t1 > slots || k1 > cols) {
    printf("trial %d, cap %ld, ntrial %d, %s time stamps, %s cut: %ld slots, %ld trial slots, %ld columns beyond the reserve of %ld slots, %ld columns\n",
           trial, cap, ntrial, time ? "with" : "no", what, n1, t1, k1, slots, cols);
    return 0;
  }
  return 1;
}

int main(void) {
  long cuts = 0;
  for (int trial = 0; trial < 4000; trial++) {
    long const nr = (long)(rnd() % 41);
    int const with_time = (int)(rnd() % 2), ntrial = 1 + (int)(rnd() % 8);
    size_t const n1 = (size_t)(nr ? nr : 1);
    long *rp = (long *)malloc(sizeof(long) * (size_t)(nr + 1));
    double *time = (double *)malloc(sizeof(double) * n1);
    int *gone = (int *)malloc(sizeof(int) * n1);
    if (!rp || !time || !gone) return 2;
    /* scans of 1 ... 6 rays: one time stamp, one width, gone or not as a whole; without time stamps every ray its own */
    rp[0] = 0;
    long m = 0;
    for (long r = 0, left = 0, w = 0, g = 0, scan = 0; r < nr; r++, left--) {
      if (left == 0 || !with_time) {
        left = 1 + (long)(rnd() % 6); scan++;
        w = rnd() % 16 == 0 ? 60 : (long)(rnd() % 10);
        g = rnd() % 3 == 0;
      }
      time[r] = (double)scan; rp[r + 1] = rp[r] + w; gone[r] = (int)g;
      m += !g;
    }
    /* the rays that remain, in arrays of their own */
    long *rp2 = (long *)malloc(sizeof(long) * (size_t)(m + 1));
    double *time2 = (double *)malloc(sizeof(double) * (size_t)(m ? m : 1));
    if (!rp2 || !time2) return 2;
    rp2[0] = 0;
    for (long r = 0, k = 0; r < nr; r++)
      if (!gone[r]) { time2[k] = time[r]; rp2[k + 1] = rp2[k] + (rp[r + 1] - rp[r]); k++; }
    for (long cap = 1; cap <= rp[nr] + nr + 1; cap++) {
      long slots = -1, cols = -1;
      if (jur_scene_pass_reserve(nr, rp, cap, ntrial, with_time ? time : NULL, &slots, &cols)) { printf("reserve refused: %s\n", g_msg); return 1; }
      if (!fits("first", trial, cap, ntrial, nr, rp, with_time ? time : NULL, slots, cols)) return 1;
      if (!fits("second", trial, cap, ntrial, m, rp2, with_time ? time2 : NULL, slots, cols)) return 1;
      cuts += 2;
    }
    free(rp); free(time); free(gone); free(rp2); free(time2);
  }
  printf("check_passes_host: %ld cuts within their reserve\n", cuts);
  return 0;
}
