/* Stand-alone check of what the scene entries' set-up keeps in pure host functions (jur_scene.c): the segment lists of the
 * hydrostatic balance (jur_scene_hydro_segments) with their sub-ranges (jur_hyseg_sub), the box on the state laid out per
 * element (jur_state_bounds_expand) and the default cap on the slots of a pass (jur_scene_default_cap).  Meant for a
 * sanitizer build on the CPU; no GPU, no library:
 *
 *   gcc -std=gnu99 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=undefined -D__HIP_PLATFORM_AMD__ \
 *       -I/opt/rocm/include -Iinclude -Ijurassic-gpu_amd/csrc -DJUR_ND=100 -DJUR_NG=30 \
 *       -o check_trial_setup_host tools/check_trial_setup_host.c jurassic-gpu_amd/csrc/jur_scene.c -lm && ./check_trial_setup_host
 *
 * 400 seeded scenes of 0 ... 40 rays in 0 ... 6 slices with state elements, nlam in {1, 3, 8}, the balance and the box on
 * and off.  Every array is malloc'ed to the size the scene entries give it, so that a read or write beyond it is an error
 * of the sanitizer.  Each function must give what the formulas give that stood inline in jur_model.c's two bodies before
 * they were shared, restated below as they stood: the lists of jur_kernel_scene_host's family (ray slices, raised copies
 * of p, T and H2O, trial copies in the retrieval) and of jur_trial_scene_host (ray slices, every trial copy), the box as
 * lo[erow - 4] | hi[erow - 4], and the cap as the budget less the parts of the slab one by one, in long. */
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

#define NRMAX 40
#define NSMAX 6

/* the lists as the two bodies built them; returns the segments written, *nhc and *ntc as they counted */
static long old_segments(size_t NH, long nr, long nrs, int const *hyf, long ncopy, long const *off, int const *prow, int row_h2o,
                         int trial_body, int looping, long tncopy, long const *toff, long *hyat, long *nhc_out, long *ntc_out) {
  int *const hylen = (int *)(hyat + NH);
  size_t const NR = (size_t)nr;
  long nhc = 0, ntc = 0;
  for (long q = 0; q < nrs; q++) { hyat[q] = hyf[q]; hylen[q] = hyf[NR + (size_t)q]; }
  if (trial_body) {
    for (long j = 1; j < tncopy; j++) { hyat[nrs + j - 1] = toff[j]; hylen[nrs + j - 1] = (int)(toff[j + 1] - toff[j]); ntc++; }
  } else {
    for (long j = 1; j < ncopy; j++)
      if (prow[j] == 4 || prow[j] == 5 || prow[j] == row_h2o) { hyat[nrs + nhc] = off[j]; hylen[nrs + nhc] = (int)(off[j + 1] - off[j]); nhc++; }
    if (looping)
      for (long j = 1; j < tncopy; j++) { hyat[nrs + nhc + ntc] = toff[j]; hylen[nrs + nhc + ntc] = (int)(toff[j + 1] - toff[j]); ntc++; }
  }
  *nhc_out = nhc; *ntc_out = ntc;
  return nrs + nhc + ntc;
}

int main(void) {
  static int const nlams[3] = {1, 3, 8};
  long lists = 0, boxes = 0, caps = 0;
  for (int trial = 0; trial < 400; trial++) {
    long const nr = (long)(rnd() % (NRMAX + 1)), nslice = nr ? (long)(rnd() % (NSMAX + 1)) : 0;
    int const nlam = nlams[rnd() % 3], hyd = (int)(rnd() % 4 != 0), box = (int)(rnd() % 2), ng = 1 + (int)(rnd() % 3), nw = (int)(rnd() % 3);
    int const row_h2o = rnd() % 3 ? 6 + (int)(rnd() % (unsigned)ng) : -1;
    int const nrow = 6 + ng + nw;

    /* slices of 2 ... 9 points, back to back in the base atmosphere; w[q] state elements each, one raised copy per element */
    long len[NSMAX + 1], first[NSMAX + 1], w[NSMAX + 1], np0 = 0, ncopies = 0, nb = 0;
    for (long q = 0; q < nslice; q++) { first[q] = np0; len[q] = 2 + (long)(rnd() % 8); np0 += len[q]; w[q] = 1 + (long)(rnd() % 12); ncopies += w[q]; nb += w[q]; }
    if (np0 < 2) np0 = 2;
    long const ncopy = 1 + ncopies, tncopy = 1 + nslice * nlam;
    long *off = (long *)malloc(sizeof(long) * (size_t)(ncopy + 1)), *toff = (long *)malloc(sizeof(long) * (size_t)(tncopy + 1));
    int *prow = (int *)malloc(sizeof(int) * (size_t)ncopy), *erow = (int *)malloc(sizeof(int) * (size_t)(nb ? nb : 1));
    if (!off || !toff || !prow || !erow) return 2;
    off[0] = 0; off[1] = np0; prow[0] = -1;
    toff[0] = 0; toff[1] = np0;
    long j = 1, e = 0;
    for (long q = 0; q < nslice; q++) {
      for (long i = 0; i < w[q]; i++, j++, e++) {
        prow[j] = erow[e] = 4 + (int)(rnd() % (unsigned)(2 + ng + nw));
        off[j + 1] = off[j] + len[q];
      }
      for (int t = 0; t < nlam; t++) { long const c = 1 + q * nlam + t; toff[c + 1] = toff[c] + len[q]; }
    }

    /* the ray slices of the balance: a seeded subset of the slices, or a slice of the base beyond them, first | len nr apart */
    long const nrs = (hyd && nr) ? (long)(rnd() % (unsigned long long)((nslice < nr ? nslice : nr) + 1)) : 0;
    int *hyf = (int *)malloc(sizeof(int) * 2 * (size_t)(nr ? nr : 1));
    if (!hyf) return 2;
    for (long q = 0; q < nrs; q++) { hyf[q] = (int)first[q]; hyf[nr + q] = (int)len[q]; }

    for (int body = 0; body < 3; body++) {          /* the single-shot entries, the retrieval, jur_trial_scene_host */
      int const trial_body = body == 2, looping = body == 1 && nslice > 0;
      size_t const NH = !hyd ? 0 : trial_body ? (size_t)nrs + (size_t)(nlam * nslice) : (size_t)nrs + (size_t)ncopies + (body == 1 ? (size_t)(nlam * nslice) : 0);
      if (!hyd) continue;                           /* (the balance is off: neither body builds a list) */
      long *want = (long *)malloc((sizeof(long) + sizeof(int)) * (NH ? NH : 1));
      if (!want) return 2;
      long whc = 0, wtc = 0, nhc = -1, ntc = -1;
      long const nw_seg = old_segments(NH, nr, nrs, hyf, ncopy, off, prow, row_h2o, trial_body, looping, tncopy, toff, want, &whc, &wtc);
      long *got = trial_body ? jur_scene_hydro_segments(NH, nr, nrs, hyf, 0, NULL, NULL, -1, tncopy, toff, &nhc, &ntc)
                             : jur_scene_hydro_segments(NH, nr, nrs, hyf, ncopy, off, prow, row_h2o, looping ? tncopy : 0, toff, &nhc, &ntc);
      if (!got) return 2;
      if (nhc != whc || ntc != wtc) { printf("trial %d, body %d: %ld raised and %ld trial copies listed, %ld and %ld expected\n", trial, body, nhc, ntc, whc, wtc); return 1; }
      if ((size_t)nw_seg > NH) { printf("trial %d, body %d: %ld segments, room for %zu\n", trial, body, nw_seg, NH); return 1; }
      int const *const glen = (int const *)(got + NH), *const wlen = (int const *)(want + NH);
      for (long i = 0; i < nw_seg; i++)
        if (got[i] != want[i] || glen[i] != wlen[i]) { printf("trial %d, body %d: segment %ld is (%ld, %d), (%ld, %d) expected\n", trial, body, i, got[i], glen[i], want[i], wlen[i]); return 1; }
      /* the three sub-ranges as the callers take them: where the pointer arithmetic d_hyat + nrs (+ nhc) stood */
      jur_hyseg_t const all = {(long)NH, got, glen};
      jur_hyseg_t const rays = jur_hyseg_sub(all, 0, nrs), raised = jur_hyseg_sub(all, nrs, nhc), trials = jur_hyseg_sub(all, nrs + nhc, ntc);
      if (rays.n != nrs || rays.at != got || rays.len != glen || raised.n != nhc || raised.at != got + nrs || raised.len != glen + nrs ||
          trials.n != ntc || trials.at != got + nrs + nhc || trials.len != glen + nrs + nhc) { printf("trial %d, body %d: sub-ranges out of step\n", trial, body); return 1; }
      for (long i = 0; i < trials.n; i++)
        if (trials.at[i] != toff[1 + i] || trials.len[i] != (int)(toff[2 + i] - toff[1 + i])) { printf("trial %d, body %d: trial copy %ld out of step\n", trial, body, i); return 1; }
      free(want); free(got);
      lists++;
    }

    /* the box per element: lo | hi in one array of 2 nb doubles, as the plan keeps it */
    if (box && nb > 0) {
      int const nq = 2 + ng + nw;
      double *lo = (double *)malloc(sizeof(double) * (size_t)nq), *hi = (double *)malloc(sizeof(double) * (size_t)nq);
      double *bx = (double *)malloc(sizeof(double) * 2 * (size_t)nb);
      if (!lo || !hi || !bx) return 2;
      for (int q = 0; q < nq; q++) { lo[q] = rnd() % 5 == 0 ? -INFINITY : -(double)(rnd() % 1000); hi[q] = rnd() % 5 == 0 ? INFINITY : (double)(rnd() % 1000); }
      jur_state_bounds_expand(lo, hi, nb, erow, bx, bx + nb);
      for (long i = 0; i < nb; i++)
        if (bx[i] != lo[erow[i] - 4] || bx[nb + i] != hi[erow[i] - 4]) { printf("trial %d: box of element %ld out of step\n", trial, i); return 1; }
      free(lo); free(hi); free(bx);
      boxes++;
    }

    /* the default cap: from the running total of the budget ladder (summed in double, part by part, as scene_fits does)
     * less the loop's part, against the budget less the parts one by one in long */
    {
      long const budget = (long)(1 + rnd() % 64) << (20 + (int)(rnd() % 14));
      size_t part[10];                              /* atm | side | hy | fov | acc | sv | dg | rt_atm | rt | kret */
      double used = 0;
      long rest = budget / 2;
      for (int i = 0; i < 10; i++) {
        part[i] = (rnd() % 3 == 0 || rest <= 0) ? 0 : (size_t)(rnd() % (unsigned long long)(rest / 3 + 1));
        rest -= (long)part[i];
        used += (double)part[i];
      }
      size_t const slot_bytes = sizeof(double) * (10 + (size_t)(3 + rnd() % 2) * (size_t)(1 + rnd() % 2378)) + sizeof(int);
      long const avail = (budget - (long)part[0] - (long)part[2] - (long)part[3] - (long)part[4] - (long)part[5] - (long)part[6] - (long)part[9] - (long)part[1]) / 16;
      long want = avail / (long)slot_bytes;
      if (want < 4096) want = 4096;
      long const got = jur_scene_default_cap(budget, (long)used - (long)part[7] - (long)part[8], slot_bytes);
      if (got != want) { printf("trial %d: cap %ld, %ld expected\n", trial, got, want); return 1; }
      /* jur_trial_scene_host's: the trial copies and its accumulators */
      long want2 = (budget - (long)part[0] - (long)part[4]) / 16 / (long)slot_bytes;
      if (want2 < 4096) want2 = 4096;
      if (jur_scene_default_cap(budget, (long)part[0] + (long)part[4], slot_bytes) != want2) { printf("trial %d: cap of the trial entry out of step\n", trial); return 1; }
      caps++;
    }
    free(off); free(toff); free(prow); free(erow); free(hyf);
    (void)nrow;
  }
  printf("check_trial_setup_host: 400 scenes, %ld segment lists, %ld boxes and %ld caps as the inline formulas gave them\n", lists, boxes, caps);
  return 0;
}
