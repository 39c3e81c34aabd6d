/* Stand-alone check of the host side of the full prior precision (jur_scene.c: jur_prior_check_R, jur_prior_check_layout,
 * jur_prior_check_corr), meant for a sanitizer build on the CPU; no GPU, no library:
 *
 *   gcc -std=gnu99 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=undefined -D__HIP_PLATFORM_AMD__ \
 *       -I/opt/rocm/include -Iinclude -Ijurassic-gpu_amd/csrc -DJUR_ND=100 -DJUR_NG=30 \
 *       -o check_prior_host tools/check_prior_host.c jurassic-gpu_amd/csrc/jur_scene.c -lm && ./check_prior_host
 *
 * Seeded layouts of up to 8 systems with widths 0, 1, 15 ... 17, 63 ... 65 and up to 299, every array malloc'ed to its
 * exact size so that a read beyond what the layout allows is an error of the sanitizer.  Every refusal is provoked and
 * held to its message; an accepted call must leave the message alone. */
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
static double uniform(void) { return (double)(rnd() >> 11) / 9007199254740992.0; }

static long const WIDTHS[] = {0, 1, 15, 16, 17, 63, 64, 65};
static long width(void) {
  unsigned long long const k = rnd() % 10;
  return k < 8 ? WIDTHS[k] : (long)(rnd() % 300);
}

static long count[16];
#define EXPECT(rc, want, text, slot)                                                                  \
  do {                                                                                                \
    if ((rc) != (want) || ((want) != JUR_OK && !strstr(g_msg, (text)))) {                              \
      printf("line %d: rc %d, message '%s', expected %d with '%s'\n", __LINE__, (rc), g_msg, (want), (text)); \
      return 1;                                                                                       \
    }                                                                                                 \
    count[slot]++;                                                                                    \
  } while (0)

int main(void) {
  char text[128];
  for (int trial = 0; trial < 3000; trial++) {
    long const ns = 1 + (long)(rnd() % 8);
    long *wptr = (long *)malloc(sizeof(long) * (size_t)(ns + 1));
    wptr[0] = 0;
    for (long q = 0; q < ns; q++) wptr[q + 1] = wptr[q] + width();
    size_t na = 0;
    for (long q = 0; q < ns; q++) na += (size_t)((wptr[q + 1] - wptr[q]) * (wptr[q + 1] - wptr[q]));
    long const nb = wptr[ns];
    double *R = (double *)malloc(sizeof(double) * (na ? na : 1));
    /* symmetric, diagonally heavy, NaN above the diagonal where nothing may read */
    size_t at = 0;
    for (long q = 0; q < ns; q++) {
      size_t const w = (size_t)(wptr[q + 1] - wptr[q]);
      for (size_t i = 0; i < w; i++)
        for (size_t j = 0; j < w; j++) R[at + i * w + j] = j > i ? NAN : j == i ? 1.0 + uniform() : uniform() - 0.5;
      at += w * w;
    }
    g_msg[0] = 0;
    int rc = jur_prior_check_R("t", ns, wptr, R);
    EXPECT(rc, JUR_OK, "", 0);
    if (g_msg[0]) { printf("an accepted call left a message: %s\n", g_msg); return 1; }
    /* one bad entry in the read triangle of a system that has one */
    long qs = -1;
    for (long k = 0; k < ns; k++) { long const q = (long)(rnd() % (unsigned long long)ns); if (wptr[q + 1] > wptr[q]) { qs = q; break; } }
    if (qs >= 0) {
      size_t const w = (size_t)(wptr[qs + 1] - wptr[qs]);
      size_t a0 = 0;
      for (long q = 0; q < qs; q++) a0 += (size_t)((wptr[q + 1] - wptr[q]) * (wptr[q + 1] - wptr[q]));
      size_t const i = (size_t)(rnd() % w), j = (size_t)(rnd() % (i + 1));
      double const kept = R[a0 + i * w + j], bad = (trial & 1) ? NAN : (trial & 2) ? INFINITY : -INFINITY;
      R[a0 + i * w + j] = bad;
      snprintf(text, sizeof text, "R of slice %ld, element (%zu, %zu) is", qs, i, j);
      rc = jur_prior_check_R("t", ns, wptr, R);
      EXPECT(rc, JUR_EINVAL, text, 1);
      if (!strstr(g_msg, "not finite")) { printf("message: %s\n", g_msg); return 1; }
      R[a0 + i * w + j] = kept;
      double const keptd = R[a0 + i * w + i];
      R[a0 + i * w + i] = -keptd;
      snprintf(text, sizeof text, "R of slice %ld, element (%zu, %zu) is", qs, i, i);
      rc = jur_prior_check_R("t", ns, wptr, R);
      EXPECT(rc, JUR_EINVAL, text, 2);
      if (!strstr(g_msg, "negative diagonal")) { printf("message: %s\n", g_msg); return 1; }
      R[a0 + i * w + i] = keptd;
    }
    /* wptr that does not ascend, or does not start at 0 */
    {
      long *bad = (long *)malloc(sizeof(long) * (size_t)(ns + 1));
      memcpy(bad, wptr, sizeof(long) * (size_t)(ns + 1));
      long const q = (long)(rnd() % (unsigned long long)ns);
      if (trial % 3 == 0) bad[0] = 1; else bad[q + 1] = bad[q] - 1 - (long)(rnd() % 5);
      rc = jur_prior_check_R("t", ns, bad, R);
      EXPECT(rc, JUR_EINVAL, "wptr is not an ascending running sum", 3);
      free(bad);
    }
    rc = jur_prior_check_R("t", ns, wptr, NULL);
    EXPECT(rc, na ? JUR_EINVAL : JUR_OK, "null argument (R)", 4);
    /* layouts: the same, another count, another width */
    rc = jur_prior_check_layout("t", ns, wptr, ns, wptr);
    EXPECT(rc, JUR_OK, "", 5);
    snprintf(text, sizeof text, "the call has %ld slices, the prior precision of the model was set for %ld", ns - 1, ns);
    rc = jur_prior_check_layout("t", ns, wptr, ns - 1, wptr);
    EXPECT(rc, JUR_EINVAL, text, 6);
    {
      long *other = (long *)malloc(sizeof(long) * (size_t)(ns + 1));
      memcpy(other, wptr, sizeof(long) * (size_t)(ns + 1));
      long const q = (long)(rnd() % (unsigned long long)ns);
      for (long k = q + 1; k <= ns; k++) other[k] += 1;
      snprintf(text, sizeof text, "slice %ld of the call has %ld elements, the prior precision of the model was set for %ld", q,
               other[q + 1] - other[q], wptr[q + 1] - wptr[q]);
      rc = jur_prior_check_layout("t", ns, wptr, ns, other);
      EXPECT(rc, JUR_EINVAL, text, 7);
      free(other);
    }
    /* jur_prior_corr_host's arguments */
    int const nq = 1 + (int)(rnd() % 6);
    double *cz = (double *)malloc(sizeof(double) * (size_t)nq);
    for (int k = 0; k < nq; k++) cz[k] = (rnd() & 1) ? 0.0 : 20.0 * uniform();
    int *iq = (int *)malloc(sizeof(int) * (size_t)(nb ? nb : 1));
    double *z = (double *)malloc(sizeof(double) * (size_t)(nb ? nb : 1)), *sg = (double *)malloc(sizeof(double) * (size_t)(nb ? nb : 1));
    for (long e = 0; e < nb; e++) { iq[e] = (int)(rnd() % (unsigned long long)nq); z[e] = 100.0 * uniform(); sg[e] = 0.01 + uniform(); }
    rc = jur_prior_check_corr("t", ns, wptr, iq, z, sg, nq, cz);
    EXPECT(rc, JUR_OK, "", 8);
    {
      int const k = (int)(rnd() % (unsigned long long)nq);
      double const kept = cz[k];
      cz[k] = (trial & 1) ? -1.0 : NAN;
      snprintf(text, sizeof text, "cz of quantity %d is", k);
      rc = jur_prior_check_corr("t", ns, wptr, iq, z, sg, nq, cz);
      EXPECT(rc, JUR_EINVAL, text, 9);
      cz[k] = kept;
    }
    if (nb > 0) {
      long const e = (long)(rnd() % (unsigned long long)nb);
      long q = 0;
      while (wptr[q + 1] <= e) q++;
      double const kept = sg[e];
      sg[e] = (trial % 3 == 0) ? 0.0 : (trial % 3 == 1) ? NAN : INFINITY;
      snprintf(text, sizeof text, "sigma of slice %ld, element %ld is", q, e - wptr[q]);
      rc = jur_prior_check_corr("t", ns, wptr, iq, z, sg, nq, cz);
      EXPECT(rc, JUR_EINVAL, text, 10);
      sg[e] = kept;
      int const kq = iq[e];
      iq[e] = (trial & 1) ? nq : -1;
      snprintf(text, sizeof text, "iq of slice %ld, element %ld is %d: outside 0..%d", q, e - wptr[q], iq[e], nq - 1);
      rc = jur_prior_check_corr("t", ns, wptr, iq, z, sg, nq, cz);
      EXPECT(rc, JUR_EINVAL, text, 11);
      iq[e] = kq;
      double const kz = z[e];
      z[e] = NAN;
      snprintf(text, sizeof text, "z of slice %ld, element %ld is", q, e - wptr[q]);
      rc = jur_prior_check_corr("t", ns, wptr, iq, z, sg, nq, cz);
      EXPECT(rc, JUR_EINVAL, text, 12);
      z[e] = kz;
    }
    free(wptr); free(R); free(cz); free(iq); free(z); free(sg);
  }
  printf("check_prior_host: 3000 layouts;");
  for (int k = 0; k < 13; k++) printf(" %ld", count[k]);
  printf("\n");
  return 0;
}
