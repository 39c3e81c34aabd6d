/* Stand-alone check of the host arithmetic of jur_param_scene_host's passes (jur_scene.c: jur_param_pass_range,
 * jur_param_pass_maps), meant for a sanitizer build on the CPU; no GPU, no library:
 *
 *   gcc -std=gnu99 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=undefined -D__HIP_PLATFORM_AMD__ \
 *       -I/opt/rocm/include -Iinclude -Ijurassic-gpu_amd/csrc -DJUR_ND=100 -DJUR_NG=30 \
 *       -o check_param_scene_host tools/check_param_scene_host.c jurassic-gpu_amd/csrc/jur_scene.c -lm && ./check_param_scene_host
 *
 * 400 seeded scenes of 0 .. 60 rays in 1 .. 7 slices whose rays are interleaved, rays without a slice and slices without
 * rays among them, widths w and wb of 0, 1, 63, 64, 65 and 130; cut into passes of random lengths, passes of one ray
 * among them; every array malloc'ed to its exact size so that a read or write beyond it is an error of the sanitizer.
 * Checked per scene: the stretch of every slice in every pass against a direct count; the stretches of a slice over the
 * passes follow one another and cover its list exactly once; the map of a pass holds the tiles of exactly the slices
 * that have rays in it, each slice once, its tiles those of jur_param_maps, with the stretch of the pass; the marks
 * carried from pass to pass never hide a slice. */
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "jur_internal.h"

void jur_set_error(char const *fmt, ...) { (void)fmt; }

static unsigned long long g_state = 88172645463325252ULL;
static unsigned long long rnd(void) { g_state ^= g_state << 13; g_state ^= g_state >> 7; g_state ^= g_state << 17; return g_state; }

static long const EDGES[] = {0, 1, 63, 64, 65, 130};
#define NEDGE ((long)(sizeof EDGES / sizeof EDGES[0]))

static long *longs(long n) { return (long *)malloc(sizeof(long) * (size_t)(n > 0 ? n : 1)); }

static int check_scene(int trial) {
  long const nslice = 1 + (long)(rnd() % 7), nr = (long)(rnd() % 61);
  long *wptr = longs(nslice + 1), *bwptr = longs(nslice + 1), *sptr = longs(nslice + 1), *mark = longs(nslice), *next = longs(nslice);
  int *sid = (int *)malloc(sizeof(int) * (size_t)(nr ? nr : 1)), *srays = (int *)malloc(sizeof(int) * (size_t)(nr ? nr : 1));
  int ok = 1;
  wptr[0] = bwptr[0] = 0;
  for (long q = 0; q < nslice; q++) {
    wptr[q + 1] = wptr[q] + EDGES[1 + rnd() % (NEDGE - 1)];
    bwptr[q + 1] = bwptr[q] + EDGES[rnd() % NEDGE];
    mark[q] = 0;
  }
  for (long r = 0; r < nr; r++) sid[r] = (int)(rnd() % (unsigned long long)(nslice + 1)) - 1;
  long const nlist = jur_scene_rays_by_slice(nr, nslice, sid, sptr, srays);
  long const ntile_all = jur_param_maps(nslice, wptr, bwptr, NULL);
  int *cmap = (int *)malloc(sizeof(int) * 3 * (size_t)(ntile_all ? ntile_all : 1));
  int *pmap = (int *)malloc(sizeof(int) * 5 * (size_t)(ntile_all ? ntile_all : 1));
  (void)jur_param_maps(nslice, wptr, bwptr, cmap);
  for (long q = 0; q < nslice; q++) next[q] = sptr[q];
  for (long r0 = 0; r0 < nr;) {
    long r1 = r0 + 1 + (long)(rnd() % 3 == 0 ? 0 : rnd() % 17);
    if (r1 > nr) r1 = nr;
    long expect = 0;
    for (long q = 0; q < nslice; q++) {
      long lo, hi, n = 0, at = -1;
      jur_param_pass_range(sptr, srays, q, r0, r1, &lo, &hi);
      for (long i = sptr[q]; i < sptr[q + 1]; i++)
        if (srays[i] >= r0 && srays[i] < r1) { if (at < 0) at = i; n++; }
      if (hi - lo != n || (n > 0 && lo != at) || lo < sptr[q] || hi > sptr[q + 1]) { printf("trial %d: slice %ld in [%ld, %ld): stretch [%ld, %ld), counted %ld from %ld\n", trial, q, r0, r1, lo, hi, n, at); ok = 0; }
      if (lo != next[q]) { printf("trial %d: slice %ld: the stretch of [%ld, %ld) starts at %ld, the last ended at %ld\n", trial, q, r0, r1, lo, next[q]); ok = 0; }
      next[q] = hi;
      if (n > 0) expect += ((wptr[q + 1] - wptr[q] + 63) / 64) * ((bwptr[q + 1] - bwptr[q] + 63) / 64);
    }
    long const nt = jur_param_pass_maps(wptr, bwptr, sptr, srays, sid, r0, r1, mark, pmap);
    if (nt != expect) { printf("trial %d: pass [%ld, %ld): %ld tiles, expected %ld\n", trial, r0, r1, nt, expect); ok = 0; }
    /* the tiles of a slice are one run, equal to its run in jur_param_maps, and no slice has two runs */
    for (long t = 0; t < nt && ok;) {
      long const q = pmap[5 * t];
      long lo, hi, c = 0;
      jur_param_pass_range(sptr, srays, q, r0, r1, &lo, &hi);
      while (c < ntile_all && cmap[3 * c] != q) c++;
      long u = t;
      for (; u < nt && pmap[5 * u] == q; u++, c++) {
        if (c >= ntile_all || cmap[3 * c] != q || cmap[3 * c + 1] != pmap[5 * u + 1] || cmap[3 * c + 2] != pmap[5 * u + 2]) { printf("trial %d: pass [%ld, %ld): tile %ld is not jur_param_maps'\n", trial, r0, r1, u); ok = 0; break; }
        if (pmap[5 * u + 3] != lo || pmap[5 * u + 4] != hi || hi == lo) { printf("trial %d: pass [%ld, %ld): tile %ld carries [%d, %d), the stretch is [%ld, %ld)\n", trial, r0, r1, u, pmap[5 * u + 3], pmap[5 * u + 4], lo, hi); ok = 0; break; }
      }
      if (c < ntile_all && cmap[3 * c] == q) { printf("trial %d: pass [%ld, %ld): slice %ld is short of tiles\n", trial, r0, r1, q); ok = 0; }
      for (long v = u; v < nt; v++) if (pmap[5 * v] == q) { printf("trial %d: pass [%ld, %ld): slice %ld twice\n", trial, r0, r1, q); ok = 0; break; }
      t = u;
    }
    r0 = r1;
  }
  for (long q = 0; q < nslice; q++)
    if (next[q] != sptr[q + 1]) { printf("trial %d: slice %ld: the passes covered its rays up to %ld of %ld\n", trial, q, next[q], sptr[q + 1]); ok = 0; }
  if (nlist > nr) ok = 0;
  free(wptr); free(bwptr); free(sptr); free(mark); free(next); free(sid); free(srays); free(cmap); free(pmap);
  return ok;
}

int main(void) {
  int bad = 0;
  for (int trial = 0; trial < 400; trial++) bad += !check_scene(trial);
  size_t sizes[2];
  jur_param_scene_abi_sizes(sizes);
  if (sizes[0] != sizeof(jur_param_scene_in_t) || sizes[1] != sizeof(jur_param_scene_out_t)) { printf("the struct sizes\n"); bad++; }
  printf(bad ? "check_param_scene_host: %d scenes FAILED\n" : "check_param_scene_host: 400 scenes ok\n", bad);
  return bad != 0;
}
