/* Stand-alone check of the lists of rays by slice (jur_scene.c: jur_scene_rays_by_slice) and of the gather of the rays
 * that remain once slices of a retrieval have ended (jur_scene_gather_active), meant for a sanitizer build on the CPU; no
 * GPU, no library:
 *
 *   gcc -std=gnu99 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=undefined -D__HIP_PLATFORM_AMD__ \
 *       -I/opt/rocm/include -Iinclude -Ijurassic-gpu_amd/csrc -DJUR_ND=100 -DJUR_NG=30 \
 *       -o check_gather_host tools/check_gather_host.c jurassic-gpu_amd/csrc/jur_scene.c -lm && ./check_gather_host
 *
 * 400 seeded scenes of 0 ... 40 rays of widths 0 ... 9 in 0 ... 6 slices, some rays without state elements (in no slice),
 * and for each every subset of its slices still active, the others ended in a seeded state.  Every array is malloc'ed to
 * the size the scene entries give it (jur_model.c: sptr[nslice + 1], srays[nr]; act[nr], pos[nr], sraysc[nlist + 1],
 * rpc[nr + 1], sptrc[nslice + 1]), so that a read or write beyond it is an error of the sanitizer.  Both functions must
 * give what the restatement below gives, which searches all rays for every slice. */
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

#define NRMAX 40
#define NSMAX 6

int main(void) {
  long subsets = 0;
  for (int trial = 0; trial < 400; trial++) {
    long const nr = (long)(rnd() % (NRMAX + 1)), nslice = (long)(rnd() % (NSMAX + 1));
    int sid0[NRMAX + 1];
    long rp0[NRMAX + 1];
    rp0[0] = 0;
    for (long r = 0; r < nr; r++) {
      sid0[r] = (nslice == 0 || rnd() % 4 == 0) ? -1 : (int)(rnd() % (unsigned long long)nslice);
      rp0[r + 1] = rp0[r] + (sid0[r] < 0 ? 0 : (long)(rnd() % 10));
    }
    int *sid = (int *)malloc(sizeof(int) * (size_t)nr), *srays = (int *)malloc(sizeof(int) * (size_t)nr);
    long *rp = (long *)malloc(sizeof(long) * (size_t)(nr + 1)), *sptr = (long *)malloc(sizeof(long) * (size_t)(nslice + 1));
    if (!sid || !srays || !rp || !sptr) return 2;
    for (long r = 0; r < nr; r++) sid[r] = sid0[r];
    for (long r = 0; r <= nr; r++) rp[r] = rp0[r];

    /* the lists: slice by slice, its rays ascending */
    long const nlist = jur_scene_rays_by_slice(nr, nslice, sid, sptr, srays);
    long at = 0;
    for (long q = 0; q < nslice; q++) {
      if (sptr[q] != at) { printf("trial %d: sptr[%ld] = %ld, %ld expected\n", trial, q, sptr[q], at); return 1; }
      for (long r = 0; r < nr; r++)
        if (sid0[r] == q) {
          if (srays[at] != r) { printf("trial %d: entry %ld of the lists is ray %d, %ld expected\n", trial, at, srays[at], r); return 1; }
          at++;
        }
    }
    if (nlist != at || sptr[nslice] != at) { printf("trial %d: %ld listed, sptr ends at %ld, %ld expected\n", trial, nlist, sptr[nslice], at); return 1; }

    /* the rays that remain, for every set of slices that are still active */
    for (long mask = 0; mask < (1L << nslice); mask++, subsets++) {
      int *state = (int *)malloc(sizeof(int) * (size_t)nslice);
      int *act = (int *)malloc(sizeof(int) * (size_t)nr), *pos = (int *)malloc(sizeof(int) * (size_t)nr);
      int *sraysc = (int *)malloc(sizeof(int) * (size_t)(nlist + 1));
      long *rpc = (long *)malloc(sizeof(long) * (size_t)(nr + 1)), *sptrc = (long *)malloc(sizeof(long) * (size_t)(nslice + 1));
      if (!state || !act || !pos || !sraysc || !rpc || !sptrc) return 2;
      for (long q = 0; q < nslice; q++) state[q] = (mask >> q) & 1 ? JUR_RET_ACTIVE : JUR_RET_CONVERGED + (int)(rnd() % 3);
      long const n = jur_scene_gather_active(nr, nslice, rp, sid, state, sptr, srays, act, pos, rpc, sptrc, sraysc);
      long m = 0, cols = 0;
      int where[NRMAX + 1];
      for (long r = 0; r < nr; r++) {
        int const stays = sid0[r] >= 0 && ((mask >> sid0[r]) & 1);
        where[r] = stays ? (int)m : -1;
        if (pos[r] != where[r]) { printf("trial %d, set %ld: pos[%ld] = %d, %d expected\n", trial, mask, r, pos[r], where[r]); return 1; }
        if (!stays) continue;
        if (m >= n || act[m] != r || rpc[m] != cols) { printf("trial %d, set %ld: remaining ray %ld out of step\n", trial, mask, m); return 1; }
        cols += rp0[r + 1] - rp0[r];
        m++;
      }
      if (n != m || rpc[n] != cols) { printf("trial %d, set %ld: %ld rays remain with %ld columns, %ld with %ld expected\n", trial, mask, n, rpc[n], m, cols); return 1; }
      long nl = 0;
      for (long q = 0; q < nslice; q++) {
        if (sptrc[q] != nl) { printf("trial %d, set %ld: sptrc[%ld] = %ld, %ld expected\n", trial, mask, q, sptrc[q], nl); return 1; }
        for (long r = 0; r < nr && ((mask >> q) & 1); r++)
          if (sid0[r] == q) {
            if (sraysc[nl] != where[r]) { printf("trial %d, set %ld: entry %ld of the gathered lists is %d, %d expected\n", trial, mask, nl, sraysc[nl], where[r]); return 1; }
            nl++;
          }
      }
      if (sptrc[nslice] != nl || nl > nlist) { printf("trial %d, set %ld: the gathered lists end at %ld, %ld expected\n", trial, mask, sptrc[nslice], nl); return 1; }
      free(state); free(act); free(pos); free(sraysc); free(rpc); free(sptrc);
    }
    free(sid); free(srays); free(rp); free(sptr);
  }
  printf("check_gather_host: 400 scenes, %ld sets of active slices as the search gives them\n", subsets);
  return 0;
}
