/* Stand-alone check of the host arithmetic of the box on the state (jur_scene.c: jur_state_bound, jur_state_bounds_expand,
 * jur_state_bounds_check, jur_state_bounds_upstream, jur_state_on_bounds), meant for a sanitizer build on the CPU; no GPU,
 * no library:
 *
 *   gcc -std=gnu99 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=undefined -D__HIP_PLATFORM_AMD__ \
 *       -I/opt/rocm/include -Iinclude -Ijurassic-gpu_amd/csrc -DJUR_ND=100 -DJUR_NG=30 \
 *       -o check_bounds_host tools/check_bounds_host.c jurassic-gpu_amd/csrc/jur_scene.c -lm && ./check_bounds_host
 *
 * Seeded layouts of 0 ... 300 elements over 2 + ng + nw quantities, every array malloc'ed to its exact size so that a read
 * or write beyond it is an error of the sanitizer.  Checked per layout: the expansion puts the quantity's interval at every
 * element (the rows are those of jur_scene_trial_t's erow: 4 p, 5 T, 6 + g q, 6 + ng + w k); the rule against its two
 * lines written out here, NaN, infinities and signed zeros among the values; a bounded value lies in its interval and a
 * second bound returns the same bits; jur_state_on_bounds against a count made here; every refusal comes with its words. */
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

int main(void) {
  ctl_t *ctl = (ctl_t *)calloc(1, sizeof(ctl_t));
  if (!ctl) return 2;
  long bounded = 0, held = 0;
  for (int trial = 0; trial < 600; trial++) {
    int const ng = 1 + (int)(rnd() % 5), nw = (int)(rnd() % (JUR_NW + 1)), nq = 2 + ng + nw;
    long const n = (long)(rnd() % 301);
    double *lo = (double *)malloc(sizeof(double) * (size_t)nq), *hi = (double *)malloc(sizeof(double) * (size_t)nq);
    int *erow = (int *)malloc(sizeof(int) * (size_t)(n ? n : 1)), *iq = (int *)malloc(sizeof(int) * (size_t)(n ? n : 1));
    double *elo = (double *)malloc(sizeof(double) * (size_t)(n ? n : 1)), *ehi = (double *)malloc(sizeof(double) * (size_t)(n ? n : 1));
    double *x = (double *)malloc(sizeof(double) * (size_t)(n ? n : 1));
    signed char *side = (signed char *)malloc((size_t)(n ? n : 1));
    if (!lo || !hi || !erow || !iq || !elo || !ehi || !x || !side) return 2;
    ctl->ng = ng; ctl->nw = nw;
    if (trial % 3 == 0) {
      if (jur_state_bounds_upstream(ctl, lo, hi) != nq || jur_state_bounds_upstream(ctl, NULL, NULL) != nq) { printf("trial %d: upstream's box: %s\n", trial, g_msg); return 1; }
      if (lo[0] != 5e-7 || hi[0] != 5e4 || lo[1] != 100 || hi[1] != 400) { printf("trial %d: upstream's p, T\n", trial); return 1; }
      for (int q = 2; q < nq; q++)
        if (lo[q] != 0 || !same(hi[q], q < 2 + ng ? 1.0 : INFINITY)) { printf("trial %d: upstream's quantity %d\n", trial, q); return 1; }
    } else
      for (int q = 0; q < nq; q++) {
        lo[q] = rnd() % 5 == 0 ? -INFINITY : uni(-10, 10);
        hi[q] = rnd() % 5 == 0 ? INFINITY : rnd() % 5 == 0 ? lo[q] : lo[q] + uni(0, 5);
        if (hi[q] != hi[q] || hi[q] < lo[q]) hi[q] = lo[q];
      }
    if (jur_state_bounds_check("check", ng, nw, nq, lo, hi)) { printf("trial %d: a good box is refused: %s\n", trial, g_msg); return 1; }
    for (long e = 0; e < n; e++) {
      iq[e] = (int)(rnd() % (unsigned)nq);
      erow[e] = 4 + iq[e];
      unsigned const k = (unsigned)(rnd() % 12);
      double const l = lo[iq[e]], h = hi[iq[e]];
      x[e] = k == 0 ? NAN : k == 1 ? INFINITY : k == 2 ? -INFINITY : k == 3 ? 0.0 : k == 4 ? -0.0 : k == 5 ? l : k == 6 ? h :
             k == 7 ? nextafter(l, -INFINITY) : k == 8 ? nextafter(h, INFINITY) : uni(-20, 20);
    }
    jur_state_bounds_expand(lo, hi, n, erow, elo, ehi);
    long count = 0;
    for (long e = 0; e < n; e++) {
      if (!same(elo[e], lo[iq[e]]) || !same(ehi[e], hi[iq[e]])) { printf("trial %d: element %ld of quantity %d expanded to [%g, %g]\n", trial, e, iq[e], elo[e], ehi[e]); return 1; }
      double c = x[e] > elo[e] ? x[e] : elo[e];
      c = c < ehi[e] ? c : ehi[e];
      double const got = jur_state_bound(x[e], elo[e], ehi[e]);
      if (!same(got, c)) { printf("trial %d: bound(%g, %g, %g) = %g, the rule gives %g\n", trial, x[e], elo[e], ehi[e], got, c); return 1; }
      if (!(got >= elo[e] && got <= ehi[e])) { printf("trial %d: bound(%g, %g, %g) = %g outside the interval\n", trial, x[e], elo[e], ehi[e], got); return 1; }
      if (!same(jur_state_bound(got, elo[e], ehi[e]), got) && !(got == 0 && (elo[e] == 0 || ehi[e] == 0))) {
        printf("trial %d: a second bound of %g in [%g, %g] changes bits\n", trial, got, elo[e], ehi[e]); return 1;
      }
      bounded += !same(got, x[e]);
      x[e] = got;
      count += got == elo[e] || got == ehi[e];
    }
    long const nb = jur_state_on_bounds(nq, lo, hi, n, iq, x, side);
    if (nb != count || jur_state_on_bounds(nq, lo, hi, n, iq, x, NULL) != count) { printf("trial %d: %ld elements on their bounds, %ld counted here: %s\n", trial, nb, count, g_msg); return 1; }
    for (long e = 0; e < n; e++) {
      int const want = x[e] == elo[e] ? -1 : x[e] == ehi[e] ? 1 : 0;
      if (side[e] != want) { printf("trial %d: side[%ld] = %d, %d expected\n", trial, e, side[e], want); return 1; }
    }
    held += count;
    /* the refusals, on arrays of their exact size */
    if (!refused(jur_state_bounds_check("check", ng, nw, nq + 1, lo, hi), "the model has", "nq + 1")) return 1;
    int const q = (int)(rnd() % (unsigned)nq);
    double const kl = lo[q], kh = hi[q];
    char words[64];
    snprintf(words, sizeof words, "of quantity %d (", q);
    lo[q] = NAN;
    if (!refused(jur_state_bounds_check("check", ng, nw, nq, lo, hi), words, "lo NaN") || !strstr(g_msg, "NaN")) return 1;
    lo[q] = kl; hi[q] = NAN;
    if (!refused(jur_state_bounds_check("check", ng, nw, nq, lo, hi), words, "hi NaN") || !strstr(g_msg, "NaN")) return 1;
    lo[q] = 2.0; hi[q] = 1.0;
    snprintf(words, sizeof words, "quantity %d (", q);
    if (!refused(jur_state_bounds_check("check", ng, nw, nq, lo, hi), words, "lo > hi") || !strstr(g_msg, "lo = 2 > hi = 1")) return 1;
    lo[q] = kl; hi[q] = kh;
    if (n > 0) {
      int const keep = iq[n - 1];
      iq[n - 1] = nq;
      if (!refused((int)jur_state_on_bounds(nq, lo, hi, n, iq, x, side), "the box has", "an element of no quantity")) return 1;
      iq[n - 1] = keep;
    }
    free(lo); free(hi); free(erow); free(iq); free(elo); free(ehi); free(x); free(side);
  }
  if (bounded == 0 || held == 0) { printf("nothing was bounded (%ld) or held (%ld)\n", bounded, held); return 1; }
  printf("check_bounds_host: %ld values moved into their intervals, %ld elements on a bound, every refusal with its words\n", bounded, held);
  free(ctl);
  return 0;
}
